/* =============================================================================
 * celerite2_amd_harmonics.h -- the multi-harmonic periodogram under correlated
 * noise on the factored covariance: the eighth public header of
 * libcelerite2_amd.so (the first, celerite2_amd.h, is included for c2_stream_t
 * and the error codes; the third, celerite2_amd_periodogram.h, has the
 * one-term sweep whose rules this one repeats per harmonic).  Same
 * conventions: float64, row-major, contiguous DEVICE pointers, a leading batch
 * dimension B of independent series, batch strides in elements (0 when shared
 * by the batch), the launch goes on `stream` and the call returns without
 * synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_HARMONICS_H_
#define CELERITE2_AMD_HARMONICS_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define C2_HARMONICS_MAX 4   /* harmonics of a trial frequency (H) one call takes */

/* Whitened harmonics of a frequency grid: with d, W of c2_factor (K + D = L diag(d) L^T), Z0 = L^-1 [A0 | y - mean]
 * (B,N,Q0) of c2_solve_lower and the ANGULAR trial frequencies freq, shared by the batch (F,) (f_bs == 0) or (B,F)
 * (f_bs == F), for every series b, frequency f and H harmonics, the NC = 2 H columns ordered (c_1, s_1, ..., c_H, s_H),
 *   a_{2h-2} = cos x_h,   a_{2h-1} = sin x_h   (h = 1 .. H),   z_i = L^-1 a_i,   <a, b> = sum_n a_n b_n / d_n
 *   T[b,f,:] = [<z_i,z_j> for 0 <= i <= j < NC, row-major over the upper triangle,          (NC (NC + 1) / 2 values)
 *               <z_i,Z0[:,q]> for i < NC (major), q < Q0]                                    (NC Q0 values)
 * in ONE forward sweep that forms the columns in registers and writes neither them nor the z_i (csrc/c2_harmonics.hip).
 * At H = 1 this is c2_whitened_sinusoids' T exactly.  With S0 = Z0^T diag(1/d) Z0 these are all the products a generalized
 * least-squares fit of y = mean + A0 beta0 + sum_h (alpha_h cos x_h + beta_h sin x_h) + GP reads, per frequency.  The sweep
 * is internal::forward with 2 H right-hand sides (internal.hpp:107-146):
 *   F <- p_n o (F + w_{n-1} z_{n-1}^T),  p_n = exp(-c (t_n - t_{n-1}))  (:139-143);   z_n = a_n - F^T u_n  (:144).
 * THE COLUMN RULE, line by line, for harmonic h of the trial frequency w_f:
 *   w_h = fl(h * w_f)            h an exact double; ONE rounding, made once when the lane builds its trial
 *   dt  = fl(t_n - t_ref)        rounded once
 *   x_h = fl(w_h * dt)           rounded once; neither line is contracted into a later fma
 *   (cos x_h, sin x_h)           the library's reduction-and-polynomial sincos for |x_h| below 1.6e6, the device
 *                                library's beyond it
 * that is: harmonic h's two columns ARE c2_whitened_sinusoids' two columns at the frequency fl(h * w_f), and everything this
 * sweep computes about one harmonic alone (its three products and its 2 Q0 products with Z0) is, bit for bit, what
 * c2_whitened_sinusoids writes at that frequency.  There is no recurrence between harmonics.  Times with a large offset
 * (Julian dates) keep their phase accuracy with t_ref at the offset.
 * A trial takes H neighbouring lanes, one harmonic each, rounded up to 2 or 4 (2 H lanes, one column each, rounded up to
 * 4 or 8 above J = 16); the products between columns of different lanes move through lane permutes, never through memory.
 * Each element of T is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  1 <= H <= C2_HARMONICS_MAX, 1 <= J <= C2_FAST_WIDTH and 1 <= Q0 <= 8 (beyond any: C2_ERR_UNSUPPORTED); B, N, F >= 1;
 * B * ceil(F / trials per wavefront) < 2^31 blocks (C2_ERR_UNSUPPORTED), with 64 / (2 or 4) trials per wavefront up to
 * J = 16 and 64 / (4 or 8) above; H = 1 is forwarded to c2_whitened_sinusoids.  A null pointer or a bad size: C2_ERR_INVALID
 * before any launch.  T must not alias an input.  Rows of a series whose factorisation failed hold garbage (never another
 * series'). */
int c2_whitened_harmonics(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t F, int64_t H, const double *t, int64_t t_bs,
                          const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                          const double *Z0 /* (B, N, Q0) */, const double *freq /* angular */, int64_t f_bs /* 0: shared (F,) */,
                          double t_ref, double *T /* (B, F, H (2 H + 1) + 2 H Q0) */, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_HARMONICS_H_ */
