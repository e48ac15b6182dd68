// c2_launch.hpp -- the host side of a launch, once.  Every path of csrc/*.hip that gives C2_ERR_HIP goes through hip_check,
// so c2_last_error() (include/celerite2_amd.h; the text lives in c2_ops.hip) always names the HIP error behind the code.
// The library's stream-ordered temporaries live here too (temp_alloc, StreamTemp): the one place that clears a sticky error.
#pragma once
#include <mutex>
#include <type_traits>
#include "c2_common.hpp"
#include "c2_internal.hpp"

namespace c2 {

inline int hip_check(hipError_t e) {   // C2_OK, or C2_ERR_HIP with the error's text recorded for this thread
  if (e == hipSuccess) return C2_OK;
  c2_internal_set_error(hipGetErrorString(e));
  return C2_ERR_HIP;
}
inline int launch_ok() { return hip_check(hipGetLastError()); }   // after one or more launches
// a clean-up call behind work whose status rc is being carried: the first error wins, its text included
inline int keep_first(int rc, hipError_t e) { return rc != C2_OK ? rc : hip_check(e); }

// Stream-ordered temporaries of the library.  They come from a memory pool the LIBRARY owns (one per device, created on
// first use, release threshold 1 GiB so that up to that much stays cached between calls: the default pool hands its memory
// back to the driver at every synchronisation and each call would pay a fresh allocation -- 0.2 ms for the 17 MB of a
// 64 x 4096 x 64 many-rhs solve that itself takes 0.4 ms).  The device's DEFAULT pool, which the process shares with
// everybody else, is left as it is; if the pool cannot be created the temporaries fall back to it, uncached.  Thread-safe
// (std::call_once per device); hipFreeAsync releases either kind.
inline hipError_t temp_alloc(void **p, size_t bytes, hipStream_t s) {
  constexpr int kMaxDev = 64;
  static std::once_flag once[kMaxDev];
  static hipMemPool_t pools[kMaxDev] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return hipMallocAsync(p, bytes, s);
  std::call_once(once[dev], [dev] {
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) == hipSuccess && pool) {
      uint64_t keep = 1ull << 30;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
      pools[dev] = pool;
    }
    (void)hipGetLastError();
  });
  if (pools[dev]) return hipMallocFromPoolAsync(p, bytes, pools[dev], s);
  return hipMallocAsync(p, bytes, s);
}

// The scratch memory of one form of an entry point: the caller's `scratch` if there is one, else `bytes` from temp_alloc
// on stream s.  There is NO ROOM -- the object tests false, get() is nullptr -- when bytes == 0 (the form does not take
// this shape), when the stream is being captured in a graph (unless the site says kAlsoInCaptures: a temporary in a
// capture becomes an allocation node of the graph), or when the allocation is refused; error() then says why (hipSuccess
// for the first two) and no sticky HIP error is left behind.  What the site does without room is the site's business:
// the next form, C2_ERR_UNSUPPORTED, or hip_check(error()).
//   StreamTemp tmp(s, nd * sizeof(double));
//   if (tmp) return tmp.release(form(..., tmp.get(), stream));
// release(rc) frees on the same stream and folds the status of the free into rc (keep_first).  A temporary still held at
// scope exit -- an early `return e;` -- is freed there, its status dropped: the error being returned came first.
class StreamTemp {
 public:
  enum Captures { kNotInCaptures, kAlsoInCaptures };
  StreamTemp(hipStream_t s, size_t bytes, void *scratch = nullptr, Captures captures = kNotInCaptures) : s_(s) {
    if (bytes == 0) return;
    if (scratch) { p_ = scratch; return; }
    if (captures == kNotInCaptures) {
      hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(s, &capturing);
      if (capturing != hipStreamCaptureStatusNone) return;
    }
    err_ = temp_alloc(&p_, bytes, s);
    if (err_ != hipSuccess) {
      p_ = nullptr;
      (void)hipGetLastError();
    } else {
      owned_ = true;
    }
  }
  StreamTemp(const StreamTemp &) = delete;
  StreamTemp &operator=(const StreamTemp &) = delete;
  ~StreamTemp() {
    if (owned_) (void)hipFreeAsync(p_, s_);
  }
  explicit operator bool() const { return p_ != nullptr; }
  double *get() const { return static_cast<double *>(p_); }
  hipError_t error() const { return err_; }
  int release(int rc) {
    if (owned_) {
      owned_ = false;
      rc = keep_first(rc, hipFreeAsync(p_, s_));
    }
    return rc;
  }

 private:
  hipStream_t s_;
  void *p_ = nullptr;
  hipError_t err_ = hipSuccess;
  bool owned_ = false;
};

// f(std::integral_constant<int, G>{}) for G = group_size(J) in 1 .. 32 (J <= C2_FAST_WIDTH); returns what f returns
template <class F>
inline auto dispatch_group(int64_t J, F &&f) {
  switch (group_size(J)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 32>{});
  }
}

// the kernels that keep a J- or Q-long vector in registers pad it to 4, 8, 16 or 32 (k_gram, k_trial_sweep)
inline int padded(int64_t n) { return n <= 4 ? 4 : group_size(n); }

// f(std::integral_constant<int, R>{}) for R = padded(n); f(... group_size(n)) for n <= 8 columns (1, 2, 4 or 8)
template <class F>
inline void dispatch_padded(int64_t n, F &&f) {
  switch (padded(n)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}
template <class F>
inline void dispatch_columns(int64_t n, F &&f) {
  switch (group_size(n)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

}  // namespace c2
