/* =============================================================================
 * celerite2_amd_periodogram.h -- the periodogram under correlated noise on the
 * factored covariance: the third public header of libcelerite2_amd.so (the
 * first, celerite2_amd.h, is included for c2_stream_t and the error codes; the
 * second is celerite2_amd_linear.h).  Same conventions: float64, row-major,
 * contiguous DEVICE pointers, a leading batch dimension B of independent
 * series, batch strides in elements (0 when shared by the batch), the launch
 * goes on `stream` and the call returns without synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_PERIODOGRAM_H_
#define CELERITE2_AMD_PERIODOGRAM_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Whitened sinusoids of a frequency grid: with d, W of c2_factor (K + D = L diag(d) L^T), Z0 = L^-1 [A0 | y - mean]
 * (B,N,Q0) of c2_solve_lower and the ANGULAR trial frequencies freq, shared by the batch (F,) (f_bs == 0) or (B,F)
 * (f_bs == F), for every series b and frequency f
 *   z_c = L^-1 cos(w_f (t - t_ref)),   z_s = L^-1 sin(w_f (t - t_ref)),   <a, b> = sum_n a_n b_n / d_n
 *   T[b,f,:] = [<z_c,z_c>, <z_c,z_s>, <z_s,z_s>, <z_c,Z0[:,k]> for k < Q0, <z_s,Z0[:,k]> for k < Q0]      (3 + 2 Q0 values)
 * in ONE forward sweep that forms both columns in registers, one lane per frequency (two above J = 16), and writes neither
 * them nor z_c, z_s (csrc/c2_periodogram.hip; O(N F J) arithmetic on 8 N (2 J + Q0 + 2) bytes per series and 64 frequencies).
 * With S0 = Z0^T diag(1/d) Z0 these are all the products a generalized least-squares fit of
 * y = mean + A0 beta0 + alpha cos + beta sin + GP reads, per frequency.  The sweep is internal::forward with two
 * right-hand sides (internal.hpp:107-146):
 *   F <- p_n o (F + w_{n-1} z_{n-1}^T),  p_n = exp(-c (t_n - t_{n-1}))  (:139-143);   z_n = a_n - F^T u_n  (:144).
 * THE PHASE is x = fl(w_f * fl(t_n - t_ref)): the difference is rounded once, then the product is rounded once, and
 * neither is contracted into a later fma -- the way numpy forms w * (t - t_ref), so a host restatement has the argument of
 * the sine and cosine bit for bit.  Times with a large offset (Julian dates) keep their phase accuracy with t_ref at the
 * offset.  |x| below 1.6e6 takes the library's own reduction-and-polynomial sincos, beyond it the device library's.
 * Each element of T is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  1 <= J <= C2_FAST_WIDTH and 1 <= Q0 <= 8 (beyond either: C2_ERR_UNSUPPORTED); B, N, F >= 1;
 * B * ceil(F / 64) < 2^31 blocks, B * ceil(F / 32) above J = 16 (C2_ERR_UNSUPPORTED).  A null pointer or a bad size:
 * C2_ERR_INVALID before any launch.  T must not alias an input.  Rows of a series whose factorisation failed hold garbage
 * (never another series'). */
int c2_whitened_sinusoids(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t F, const double *t, int64_t t_bs,
                          const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                          const double *Z0 /* (B, N, Q0) */, const double *freq /* angular */, int64_t f_bs /* 0: shared (F,) */,
                          double t_ref, double *T /* (B, F, 3 + 2 * Q0) */, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_PERIODOGRAM_H_ */
