// c2_invdiag.hip -- the DIAGONAL OF THE INVERSE of the factored matrix, q_n = [(K + D)^-1]_nn, in one backward sweep over
// d, W (c2_inverse_diag, include/celerite2_amd.h), optionally with the one-column upper solve alpha = L^-T (z / d) carried
// by the same pass.  What the predictive variance at the observed times (var_n = D_n - D_n^2 q_n) and leave-one-out
// (mean y_n - alpha_n / q_n, variance 1 / q_n) need; no counterpart in the reference, which forms the N x N
// cross-covariance for the former and has no entry point for the latter.
//
// With L = I + tril(U W^T o decay), K + D = L diag(d) L^T (forward.hpp:69-135) and p_n = exp(-c (t_{n+1} - t_n)), the
// trailing block of (K + D)^-1 behind row n enters row n only through the symmetric J x J state
//   M_n = sum_{k,l > n} (decay_{n->k} o u_k) [(K+D)^-1]_kl (decay_{n->l} o u_l)^T,
// and one row costs O(J^2):
//   G = (p_n p_n^T) o M      (M = 0 behind the last row)
//   h = M (p_n o w_n)        (so that g = G w_n = p_n o h),   s = w_n^T g
//   q_n = 1 / d_n + s
//   M <- G - u_n g^T - g u_n^T + q_n u_n u_n^T
// i.e. M'_ij = p_i (p_j M_ij - h_i u_j) + u_i (q_n u_j - p_j h_j).  M stays symmetric positive semidefinite and
// q_n <= 1 / D_n bounds it.  The upper solve is internal::backward (internal.hpp:148-189) with one right-hand side:
//   F <- p_n o (F + u_{n+1} alpha_{n+1}),   alpha_n = z_n / d_n - w_n^T F.
//
// Two mappings, chosen by width alone (a one-lane mapping was measured, lost at every batch and was removed: DESIGN.md
// section 3):
//   k_invdiag_group  J <= 32: a GROUP of G lanes per series, lane j owns column j of M (= row j: M is
//                    symmetric, so h_j = sum_i M_ij v_i is a lane-local dot product against the vector v, which the
//                    group shares through LDS); s and the solve's w^T F are one interleaved DPP butterfly (gsum2).
//                    Scalar streams move transposed in time, 16 rows per block, as in k_sweep1.
//   k_invdiag_wide   33 <= J <= 128: a workgroup per series, M in LDS (128 KiB at J = 128), as csrc/c2_wide.hip.
// There is no time-parallel form: at one series the sweep is latency-bound like the other row-by-row kernels.
// No atomics anywhere: two calls give identical bits.  B is in grid.x for both.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace c2 {
namespace invdiag {

constexpr int kRows = 16;   // rows per block of the scalar streams: 128 bytes per series

// ---------------------------------------------------------------------------------------------------------------------
// A group of G lanes per series; lane j owns column j of M.  J <= G (lanes j >= J idle: zero rows, c = 0).
// LDS: the four width-G vectors of a step (v = p o w, p, u, h) and the transposed scalar streams of two blocks.
// ---------------------------------------------------------------------------------------------------------------------
// WS: row n also stores the state ENTERING it, before its decay is applied -- column j of M into Mws[b, n, j, :] (lane j
// writes its own J consecutive doubles, the group J^2) and, with z, F_j into Fws[b, n, j]: what c2_inverse_diag_rev reads.
template <int G, bool HASZ, bool WS = false>
__global__ __launch_bounds__(kWave) void k_invdiag_group(int64_t B, int64_t N, int J, const double *__restrict__ t,
                                                         int64_t t_bs, const double *__restrict__ c, int64_t c_bs,
                                                         const double *__restrict__ U, const double *__restrict__ W,
                                                         const double *__restrict__ d, const double *z, double *__restrict__ q,
                                                         double *alpha, double *__restrict__ Mws = nullptr,
                                                         double *__restrict__ Fws = nullptr) {
  constexpr int SPW = kWave / G, R = kRows, NV = (R + G - 1) / G, RD = G >= 32 ? 4 : 8;   // RD: rows of U, W in flight
  __shared__ __attribute__((aligned(16))) double sv[kWave], sp[kWave], su[kWave], sh[kWave];
  __shared__ __attribute__((aligned(16))) double sc[2][3][SPW][R];
  const Geo<G> L(B, J);
  const int j = L.j, grp = L.lane / G, g0 = grp * G;
  const bool act = L.act;
  const double *tb = t + L.b * t_bs, *db = d + L.b * N, *zb = HASZ ? z + L.b * N : nullptr;
  const double *Ub = U + L.b * N * J + L.jj, *Wb = W + L.b * N * J + L.jj;
  double *qb = q + L.b * N, *ab = HASZ ? alpha + L.b * N : nullptr;
  const double cj = act ? c[L.b * c_bs + j] : 0.0;

  double Mc[G];
#pragma unroll
  for (int i = 0; i < G; ++i) Mc[i] = 0.0;
  double F = 0.0, tnext = tb[N - 1];   // F: with u_{n+1} alpha_{n+1} already added

  // transposed scalar streams: lane j of a group takes rows n0 + j, n0 + G + j, ... of a block
  double vt[NV], vd[NV], vz[NV];
  auto vload = [&](int64_t n0) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      int64_t n = n0 + m * G + j;
      n = n < N - 1 ? n : N - 1;
      n = n > 0 ? n : 0;
      vt[m] = tb[n]; vd[m] = db[n];
      vz[m] = HASZ ? zb[n] : 0.0;
    }
  };
  auto vstage = [&](int buf) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int idx = m * G + j;
      if (G * NV == R || idx < R) { sc[buf][0][grp][idx] = vt[m]; sc[buf][1][grp][idx] = vd[m]; sc[buf][2][grp][idx] = vz[m]; }
    }
  };
  double ru[RD], rw[RD];
  auto load_row = [&](int r, int64_t n) {
    n = n < N - 1 ? n : N - 1;
    n = n > 0 ? n : 0;
    const double x = Ub[n * J], y = Wb[n * J];   // (an idle lane reads column 0 and drops it)
    ru[r] = act ? x : 0.0;
    rw[r] = act ? y : 0.0;
  };

  const int64_t nblk = (N + R - 1) / R;
  int64_t n0 = (nblk - 1) * R;
  vload(n0); vstage(0);
#pragma unroll
  for (int k = 0; k < RD; ++k) load_row(k, (N - 1) - (((N - 1) - k) % RD + RD) % RD);   // slot k: the last row n <= N - 1 with n mod RD == k
  lds_order();
  int buf = 0;
  double qv[NV], av[NV];

  auto block = [&](auto checked_tag) {
    constexpr bool CHECKED = decltype(checked_tag)::value;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const int r = R - 1 - rr;
      const int64_t n = n0 + r;
      if (!CHECKED || n < N) {
        const double tn = sc[buf][0][grp][r], dn = sc[buf][1][grp][r], zn = sc[buf][2][grp][r];
        const double un = ru[r % RD], wn = rw[r % RD];
        load_row(r % RD, n - RD);
        if constexpr (WS) {
          if (L.valid && act) {
            double *mw = Mws + ((L.b * N + n) * J + j) * J;
#pragma unroll
            for (int i = 0; i < G; ++i)
              if (i < J) mw[i] = Mc[i];
            if constexpr (HASZ) Fws[(L.b * N + n) * J + j] = F;
          }
        }
        const double p = exp_decay(cj * (tn - tnext));
        tnext = tn;
        const double v = p * wn;
        sv[L.lane] = v; sp[L.lane] = p; su[L.lane] = un;
        lds_order();
        double h = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          h = fma(Mc[i], sv[g0 + i], h);
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (eight columns at a time: look-ahead costs registers)
        }
        double s = v * h, red = 0.0;
        if constexpr (HASZ) {
          F = p * F;   // internal.hpp:186
          red = wn * F;
          gsum2<G>(s, red);
        } else {
          s = gsum<G>(s);
        }
        const double rd = rcp_nr(dn);
        const double qn = rd + s;
        const double an = fma(zn, rd, -red);   // internal.hpp:187
        if constexpr (HASZ) F = fma(un, an, F);  // :183, for the row below
        sh[L.lane] = h;
        lds_order();
        const double e = fma(qn, un, -(p * h));
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const double x = fma(-sh[g0 + i], un, p * Mc[i]);
          Mc[i] = fma(su[g0 + i], e, sp[g0 + i] * x);
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
        lds_order();   // (the next step overwrites the vectors)
        if ((r & (G - 1)) == j) { qv[r / G] = qn; av[r / G] = an; }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (L.valid) {
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        const int idx = m * G + j;
        if ((G * NV == R || idx < R) && (!CHECKED || n0 + idx < N)) {
          qb[n0 + idx] = qv[m];
          if constexpr (HASZ) ab[n0 + idx] = av[m];
        }
      }
    }
  };

  for (int64_t blk = nblk - 1; blk >= 0; --blk, n0 -= R) {
    if (blk > 0) vload(n0 - R);   // (alpha == z: these rows lie below everything stored so far)
    if (blk == nblk - 1) block(std::true_type{});
    else block(std::false_type{});
    if (blk > 0) { vstage(buf ^ 1); lds_order(); buf ^= 1; }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Wide models: a workgroup of 256 threads per series.  LDS: M[J*J] (M(i,j) at i + J*j; symmetric), p, u, v, h, e [J], red[8].
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kWideThreads = 256;

__device__ __forceinline__ double block_sum(double x, double *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, kWave);
  __syncthreads();   // (earlier readers of red are done)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kWideThreads) void k_invdiag_wide(int64_t N, int J, const double *__restrict__ t, int64_t t_bs,
                                                               const double *__restrict__ c, int64_t c_bs,
                                                               const double *__restrict__ U, const double *__restrict__ W,
                                                               const double *__restrict__ d, const double *z,
                                                               double *__restrict__ q, double *alpha) {
  extern __shared__ double sm[];
  double *M = sm, *p = M + J * J, *u = p + J, *v = u + J, *hh = v + J, *ee = hh + J, *red = ee + J;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double *tb = t + b * t_bs, *cb = c + b * c_bs, *db = d + b * N, *Ub = U + b * N * J, *Wb = W + b * N * J;
  const double *zb = z ? z + b * N : nullptr;
  double *qb = q + b * N, *ab = alpha ? alpha + b * N : nullptr;
  for (int e = tid; e < J * J; e += kWideThreads) M[e] = 0.0;
  const double cj = tid < J ? cb[tid] : 0.0;
  double F = 0.0, tnext = tb[N - 1];
  __syncthreads();
  for (int64_t n = N - 1; n >= 0; --n) {
    const double tn = tb[n], dn = db[n], zn = zb ? zb[n] : 0.0;
    double vj = 0.0, redj = 0.0, pj = 0.0, uj = 0.0;
    if (tid < J) {
      pj = exp(cj * (tn - tnext));
      uj = Ub[n * J + tid];
      const double wj = Wb[n * J + tid];
      vj = pj * wj;
      p[tid] = pj; u[tid] = uj; v[tid] = vj;
      F = pj * F;
      redj = wj * F;
    }
    tnext = tn;
    __syncthreads();
    double h = 0.0;
    if (tid < J)
      for (int i = 0; i < J; ++i) h = fma(M[tid + J * i], v[i], h);   // row tid of the symmetric M: consecutive addresses
    const double s = block_sum(vj * h, red);
    const double rsum = block_sum(redj, red);
    const double qn = 1.0 / dn + s;
    const double an = zn / dn - rsum;
    F = fma(uj, an, F);
    if (tid < J) { hh[tid] = h; ee[tid] = fma(qn, uj, -(pj * h)); }
    if (tid == 0) {
      qb[n] = qn;
      if (ab) ab[n] = an;   // (alpha == z: every thread read z[n] before the barriers of block_sum)
    }
    __syncthreads();
    for (int k = tid >> 6; k < J; k += kWideThreads / kWave)
      for (int i = tid & 63; i < J; i += kWave) {
        const double x = fma(-hh[i], u[k], p[k] * M[i + J * k]);
        M[i + J * k] = fma(u[i], ee[k], p[i] * x);
      }
    __syncthreads();
  }
}

// The wide kernel's dynamic LDS beyond 64 KiB needs the function attribute raised: once per device, to what the widest model
// takes, on the first wide call -- not on every call (a later call may sit inside a stream capture).
inline size_t wide_lds_bytes(int64_t J) { return sizeof(double) * ((size_t)J * J + 5 * J + 8); }
inline int wide_lds_ready() {
  constexpr int kMaxDev = 64;
  static std::once_flag once[kMaxDev];
  static hipError_t err[kMaxDev];
  int dev = 0;
  if (int e = hip_check(hipGetDevice(&dev))) return e;
  if (dev < 0 || dev >= kMaxDev) return hip_check(hipErrorInvalidDevice);
  std::call_once(once[dev], [dev] {
    err[dev] = hipFuncSetAttribute(reinterpret_cast<const void *>(k_invdiag_wide), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)wide_lds_bytes(C2_MAX_WIDTH));
  });
  return hip_check(err[dev]);
}

template <int G>
inline void launch_group_ws(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                            const double *U, const double *W, const double *d, const double *z, double *q, double *alpha,
                            double *Mws, double *Fws, hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  if (z)
    hipLaunchKernelGGL((k_invdiag_group<G, true, true>), grid, dim3(kWave), 0, s, B, N, (int)J, t, t_bs, c, c_bs, U, W, d, z, q,
                       alpha, Mws, Fws);
  else
    hipLaunchKernelGGL((k_invdiag_group<G, false, true>), grid, dim3(kWave), 0, s, B, N, (int)J, t, t_bs, c, c_bs, U, W, d, z, q,
                       alpha, Mws, Fws);
}

template <int G>
inline void launch_group(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                         const double *U, const double *W, const double *d, const double *z, double *q, double *alpha,
                         hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  if (z)
    hipLaunchKernelGGL((k_invdiag_group<G, true>), grid, dim3(kWave), 0, s, B, N, (int)J, t, t_bs, c, c_bs, U, W, d, z, q, alpha,
                       (double *)nullptr, (double *)nullptr);
  else
    hipLaunchKernelGGL((k_invdiag_group<G, false>), grid, dim3(kWave), 0, s, B, N, (int)J, t, t_bs, c, c_bs, U, W, d, z, q, alpha,
                       (double *)nullptr, (double *)nullptr);
}

}  // namespace invdiag
}  // namespace c2

using namespace c2;
using namespace c2::invdiag;

extern "C" int c2_inverse_diag(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                               const double *U, const double *W, const double *d, const double *z, double *q, double *alpha,
                               c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_MAX_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !q || ((z == nullptr) != (alpha == nullptr))) return C2_ERR_INVALID;
  if ((B + kWave - 1) / kWave > 0x7fffffffLL || (J > C2_FAST_WIDTH && B > 0x7fffffffLL)) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (J > C2_FAST_WIDTH) {
    const size_t bytes = wide_lds_bytes(J);
    if (bytes > 64 * 1024)
      if (int e = wide_lds_ready()) return e;
    hipLaunchKernelGGL(k_invdiag_wide, dim3((unsigned)B), dim3(kWideThreads), bytes, s, N, (int)J, t, t_bs, c, c_bs, U, W, d,
                       z, q, alpha);
    return launch_ok();
  }
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  dispatch_group(J, [&](auto g) { launch_group<decltype(g)::value>(B, N, J, t, t_bs, c, c_bs, U, W, d, z, q, alpha, s); });
  return launch_ok();
}

extern "C" int c2_inverse_diag_fwd(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                   int64_t c_bs, const double *U, const double *W, const double *d, const double *z, double *q,
                                   double *alpha, double *Mws, double *Fws, c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;   // (J^2 doubles per row: 131 KB at J = 128)
  if (!t || !c || !U || !W || !d || !q || !Mws || ((z == nullptr) != (alpha == nullptr)) || ((z == nullptr) != (Fws == nullptr)))
    return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) { launch_group_ws<decltype(g)::value>(B, N, J, t, t_bs, c, c_bs, U, W, d, z, q, alpha, Mws, Fws, s); });
  return launch_ok();
}
