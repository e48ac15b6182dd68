// c2_term_params.hip -- term HYPER-PARAMETERS on the device: parameters -> celerite coefficients and the reverse of
// that map, plus the two hyper-parameters every model has (a jitter added to the white-noise diagonal, a constant mean).
//
// What a sampler or optimiser differentiates is S0, w0, Q (or sigma, rho, tau) of an SHO term, sigma, rho of a Matern-3/2
// term, sigma, period, Q0, dQ, f of a rotation term -- not the six coefficient arrays c2_loglik_terms takes.  The reference
// obtains that derivative by autodiff through its term classes (python/celerite2/jax/terms.py, pymc/terms.py); here the
// formulas of python/celerite2/terms.py:515-521 (RealTerm), 554-569 (ComplexTerm), 658-691 (SHOTerm), 729-745
// (Matern32Term) and 791-812 (RotationTerm) and their hand-written reverse are one kernel each, one thread per series.
// (The formulas themselves live in c2_term_leaf.hpp, shared with the term algebra of c2_term_expr.hip.)
//
// The model is a "program" (c2_term_program, celerite2_amd.h): the flattened sum of terms.  It travels to the kernels BY
// VALUE as a kernel argument -- no device allocation, no host read of device data -- so the wavefront walks it with
// scalar loads and uniform branches; only the per-series branch of the mixed SHO regime diverges.
//
// Mapping: k_coefficients / k_coefficients_rev one LANE per series (B x (NP + 2 Jr + 4 Jc) doubles in all: tens of
// megabytes at 65536 series, nothing to tune).  k_noise_mean_apply one block per 512-element row segment, 16 bytes per
// lane; k_noise_mean_rev one WAVEFRONT per series row, 16 bytes per lane per load, lane-strided partial sums in a fixed
// order and a __shfl_xor butterfly -- no atomics, so two runs give identical bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/celerite2_amd.h"
#include "c2_term_leaf.hpp"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace {

using namespace c2leaf;

__global__ __launch_bounds__(256) void k_coefficients(c2_term_program prog, int64_t B, const double *__restrict__ P,
                                                      int64_t p_bs, double *__restrict__ ar, double *__restrict__ cr,
                                                      double *__restrict__ ac, double *__restrict__ bc,
                                                      double *__restrict__ cc, double *__restrict__ dc,
                                                      int32_t *__restrict__ flag) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *p = P + b * p_bs;
  const int64_t Jr = prog.Jr, Jc = prog.Jc;
  double *R0 = ar + b * Jr, *R1 = cr + b * Jr;
  double *C0 = ac + b * Jc, *C1 = bc + b * Jc, *C2 = cc + b * Jc, *C3 = dc + b * Jc;
  int32_t bad = 0;
  for (int t = 0; t < prog.nterms; ++t) leaf_forward<double *>(prog.term[t], t, p, R0, R1, C0, C1, C2, C3, bad);
  flag[b] = bad;
}

// The reverse.  Lane b owns row b of bP: it zeroes the row, then adds each term's contribution in program order (columns
// may be shared between terms), so the sum has one fixed order.  A series whose regime flag or factorisation flag is set
// gets a zero row, ll = -inf and lflag = C2_FLAG_REGIME (regime) -- the verdict never leaves the device.
__global__ __launch_bounds__(256) void k_coefficients_rev(c2_term_program prog, int64_t B, const double *__restrict__ P,
                                                          int64_t p_bs, const double *__restrict__ bar,
                                                          const double *__restrict__ bcr, const double *__restrict__ bac,
                                                          const double *__restrict__ bbc, const double *__restrict__ bcc,
                                                          const double *__restrict__ bdc, const int32_t *__restrict__ tflag,
                                                          int32_t *__restrict__ lflag, double *__restrict__ ll,
                                                          double *__restrict__ bP) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *p = P + b * p_bs;
  double *g = bP + b * prog.np;
  for (int k = 0; k < prog.np; ++k) g[k] = 0.0;
  if (tflag && tflag[b] != 0) {
    if (ll) ll[b] = -INFINITY;
    if (lflag) lflag[b] = C2_FLAG_REGIME;
    return;
  }
  if (lflag && lflag[b] != 0) return;
  const int64_t Jr = prog.Jr, Jc = prog.Jc;
  const double *R0 = bar + b * Jr, *R1 = bcr + b * Jr;
  const double *C0 = bac + b * Jc, *C1 = bbc + b * Jc, *C2 = bcc + b * Jc, *C3 = bdc + b * Jc;
  for (int t = 0; t < prog.nterms; ++t) leaf_reverse<const double *>(prog.term[t], p, R0, R1, C0, C1, C2, C3, g);
}

// ---- jitter and mean ------------------------------------------------------------------------------------------------
constexpr int kSeg = 512;   // elements of one row segment: 256 lanes x 16 bytes

// diag = (sq ? yerr^2 : yerr) + jitter^2, r = y - mean.  Block = one segment of one row (flat grid: B * nseg blocks, no
// grid.y, so B is not limited to 65535).  VEC: N even -> every row starts 16-byte aligned and each lane moves a double2.
// SHIFT: one more per-series term, diag += shift[b] (the diagonal shift of an exposure-time convolution: negative, so it
// cannot be folded into jitter^2); added LAST, so that shift = 0 leaves the bits of the kernel without it.
template <bool VEC, bool SHIFT>
__global__ __launch_bounds__(256) void k_noise_mean_apply(int64_t N, int nseg, int sq, const double *__restrict__ yerr,
                                                          const double *__restrict__ jitter, const double *__restrict__ mean,
                                                          const double *__restrict__ shift, const double *__restrict__ y,
                                                          double *__restrict__ diag, double *__restrict__ r) {
  const int64_t b = blockIdx.x / nseg;
  const int64_t n0 = (int64_t)(blockIdx.x % nseg) * kSeg;
  const double j = jitter ? jitter[b] : 0.0, m = mean ? mean[b] : 0.0;
  const double j2 = j * j;
  double sh = 0.0;
  if constexpr (SHIFT) sh = shift[b];
  const int64_t row = b * N;
  if constexpr (VEC) {
    const int64_t n = n0 + 2 * threadIdx.x;
    if (n >= N) return;
    const double2 e = *reinterpret_cast<const double2 *>(yerr + row + n);
    const double2 v = *reinterpret_cast<const double2 *>(y + row + n);
    double2 d, o;
    d.x = (sq ? e.x * e.x : e.x) + j2;
    d.y = (sq ? e.y * e.y : e.y) + j2;
    if constexpr (SHIFT) {
      d.x += sh;
      d.y += sh;
    }
    o.x = v.x - m;
    o.y = v.y - m;
    *reinterpret_cast<double2 *>(diag + row + n) = d;
    *reinterpret_cast<double2 *>(r + row + n) = o;
  } else {
    for (int k = 0; k < 2; ++k) {
      const int64_t n = n0 + threadIdx.x + 256 * k;
      if (n >= N) return;
      const double e = yerr[row + n];
      double d = (sq ? e * e : e) + j2;
      if constexpr (SHIFT) d += sh;
      diag[row + n] = d;
      r[row + n] = y[row + n] - m;
    }
  }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// bjitter[b] = 2 jitter[b] sum_n bdiag[b, n], bmean[b] = -sum_n by[b, n] (and bshift[b] = sum_n bdiag[b, n]): one wavefront per row, ONE pass over both arrays.
// Summation order: lane l adds its elements n = 2 l, 2 l + 1, 2 l + 128, ... in increasing n, then the butterfly -- fixed.
template <bool VEC>
__global__ __launch_bounds__(256) void k_noise_mean_rev(int64_t B, int64_t N, const double *__restrict__ jitter,
                                                        const double *__restrict__ bdiag, const double *__restrict__ by,
                                                        const int32_t *__restrict__ flag,
                                                        const int32_t *__restrict__ tflag, double *__restrict__ bjitter,
                                                        double *__restrict__ bmean, double *__restrict__ bshift) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;   // (whole wavefronts leave together)
  const double *pd = bdiag + b * N, *py = by + b * N;
  double sd = 0.0, sy = 0.0;
  if constexpr (VEC) {
    double sd1 = 0.0, sy1 = 0.0;
    for (int64_t n = 2 * lane; n < N; n += 128) {
      const double2 d = *reinterpret_cast<const double2 *>(pd + n);
      const double2 v = *reinterpret_cast<const double2 *>(py + n);
      sd += d.x; sd1 += d.y;
      sy += v.x; sy1 += v.y;
    }
    sd += sd1;
    sy += sy1;
  } else {
    for (int64_t n = lane; n < N; n += 64) {
      sd += pd[n];
      sy += py[n];
    }
  }
  sd = wave_sum(sd);
  sy = wave_sum(sy);
  if (lane == 0) {
    const bool dead = (flag && flag[b] != 0) || (tflag && tflag[b] != 0);
    if (bjitter) bjitter[b] = dead ? 0.0 : 2.0 * (jitter ? jitter[b] : 0.0) * sd;
    if (bmean) bmean[b] = dead ? 0.0 : -sy;
    if (bshift) bshift[b] = dead ? 0.0 : sd;   // d diag[b, n] / d shift[b] = 1: the row sum bjitter already needs
  }
}

inline unsigned blocks_for(int64_t B) { return (unsigned)((B + 255) / 256); }

}  // namespace

extern "C" {

int c2_term_coefficients(const c2_term_program *prog, int64_t B, const double *P, int64_t p_bs, double *ar, double *cr,
                         double *ac, double *bc, double *cc, double *dc, int32_t *flag, c2_stream_t stream) {
  if (const int rc = check_program(prog, 32)) return rc;
  if (B < 1 || !P || !flag || (p_bs != 0 && p_bs != prog->np)) return C2_ERR_INVALID;
  if ((prog->Jr && (!ar || !cr)) || (prog->Jc && (!ac || !bc || !cc || !dc))) return C2_ERR_INVALID;
  hipLaunchKernelGGL(k_coefficients, dim3(blocks_for(B)), dim3(256), 0, (hipStream_t)stream, *prog, B, P, p_bs, ar, cr, ac,
                     bc, cc, dc, flag);
  return c2::launch_ok();
}

int c2_term_coefficients_rev(const c2_term_program *prog, int64_t B, const double *P, int64_t p_bs, const double *bar,
                             const double *bcr, const double *bac, const double *bbc, const double *bcc,
                             const double *bdc, const int32_t *tflag, int32_t *lflag, double *ll, double *bP,
                             c2_stream_t stream) {
  if (const int rc = check_program(prog, 32)) return rc;
  if (B < 1 || !P || !bP || (p_bs != 0 && p_bs != prog->np)) return C2_ERR_INVALID;
  if ((prog->Jr && (!bar || !bcr)) || (prog->Jc && (!bac || !bbc || !bcc || !bdc))) return C2_ERR_INVALID;
  hipLaunchKernelGGL(k_coefficients_rev, dim3(blocks_for(B)), dim3(256), 0, (hipStream_t)stream, *prog, B, P, p_bs, bar, bcr,
                     bac, bbc, bcc, bdc, tflag, lflag, ll, bP);
  return c2::launch_ok();
}

int c2_noise_mean_shift_apply(int64_t B, int64_t N, const double *yerr, int yerr_is_sigma, const double *jitter,
                              const double *mean, const double *shift, const double *y, double *diag, double *r,
                              c2_stream_t stream) {
  if (B < 1 || N < 1 || !yerr || !y || !diag || !r) return C2_ERR_INVALID;
  const int64_t nseg = (N + kSeg - 1) / kSeg;
  if (B * nseg > 0x7fffffffLL) return C2_ERR_INVALID;
  const dim3 grid((unsigned)(B * nseg));
  const hipStream_t s = (hipStream_t)stream;
#define C2_NM_APPLY(VEC, SHIFT)                                                                                      \
  hipLaunchKernelGGL((k_noise_mean_apply<VEC, SHIFT>), grid, dim3(256), 0, s, N, (int)nseg, yerr_is_sigma, yerr, jitter, \
                     mean, shift, y, diag, r)
  if (N % 2 == 0) {
    if (shift) C2_NM_APPLY(true, true);
    else C2_NM_APPLY(true, false);
  } else {
    if (shift) C2_NM_APPLY(false, true);
    else C2_NM_APPLY(false, false);
  }
#undef C2_NM_APPLY
  return c2::launch_ok();
}

int c2_noise_mean_apply(int64_t B, int64_t N, const double *yerr, int yerr_is_sigma, const double *jitter,
                        const double *mean, const double *y, double *diag, double *r, c2_stream_t stream) {
  return c2_noise_mean_shift_apply(B, N, yerr, yerr_is_sigma, jitter, mean, nullptr, y, diag, r, stream);
}

int c2_noise_mean_shift_rev(int64_t B, int64_t N, const double *jitter, const double *bdiag, const double *by,
                            const int32_t *flag, const int32_t *tflag, double *bjitter, double *bmean, double *bshift,
                            c2_stream_t stream) {
  if (B < 1 || N < 1 || !bdiag || !by || (!bjitter && !bmean && !bshift)) return C2_ERR_INVALID;
  const dim3 grid((unsigned)((B + 3) / 4));
  if (N % 2 == 0)
    hipLaunchKernelGGL(k_noise_mean_rev<true>, grid, dim3(256), 0, (hipStream_t)stream, B, N, jitter, bdiag, by, flag, tflag,
                       bjitter, bmean, bshift);
  else
    hipLaunchKernelGGL(k_noise_mean_rev<false>, grid, dim3(256), 0, (hipStream_t)stream, B, N, jitter, bdiag, by, flag, tflag,
                       bjitter, bmean, bshift);
  return c2::launch_ok();
}

int c2_noise_mean_rev(int64_t B, int64_t N, const double *jitter, const double *bdiag, const double *by,
                      const int32_t *flag, double *bjitter, double *bmean, c2_stream_t stream) {
  if (!bjitter && !bmean) return C2_ERR_INVALID;
  return c2_noise_mean_shift_rev(B, N, jitter, bdiag, by, flag, nullptr, bjitter, bmean, nullptr, stream);
}

}  // extern "C"
