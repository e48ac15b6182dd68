// c2_launch.hpp -- the host side of a launch, once.  Every path of csrc/*.hip that gives C2_ERR_HIP goes through hip_check,
// so c2_last_error() (include/celerite2_amd.h; the text lives in c2_ops.hip) always names the HIP error behind the code.
#pragma once
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
