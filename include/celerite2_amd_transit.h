/* =============================================================================
 * celerite2_amd_transit.h -- the transit search (box least squares) under
 * correlated noise on the factored covariance: the fourth public header of
 * libcelerite2_amd.so (the first, celerite2_amd.h, is included for c2_stream_t
 * and the error codes; the second and third are celerite2_amd_linear.h and
 * celerite2_amd_periodogram.h).  Same conventions: float64, row-major,
 * contiguous DEVICE pointers, a leading batch dimension B of independent
 * series, batch strides in elements (0 when shared by the batch), the launch
 * goes on `stream` and the call returns without synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_TRANSIT_H_
#define CELERITE2_AMD_TRANSIT_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Whitened transit templates of a trial grid: with d, W of c2_factor (K + D = L diag(d) L^T), Z0 = L^-1 [A0 | y - mean]
 * (B,N,Q0) of c2_solve_lower and the trials (period P, epoch t0, duration w, ingress tau), four doubles each, shared by the
 * batch (K,4) (tr_bs == 0) or (B,K,4) (tr_bs == 4 K), for every series b and trial k
 *   z = L^-1 b_k(t),   <a, b> = sum_n a_n b_n / d_n,   T[b,k,:] = [<z,z>, <z,Z0[:,j]> for j < Q0]            (1 + Q0 values)
 * in ONE forward sweep that forms the template in registers, one lane per trial, and writes neither it nor z
 * (csrc/c2_transit.hip; O(N K J) arithmetic on 8 N (2 J + Q0 + 2) bytes per series and 64 trials).  With
 * S0 = Z0^T diag(1/d) Z0 these are all the products a generalized least-squares fit of y = mean + A0 beta0 + delta b_k + GP
 * reads, per trial.  The sweep is internal::forward with one right-hand side (internal.hpp:107-146):
 *   f <- p_n o (f + w_{n-1} z_{n-1}),  p_n = exp(-c (t_n - t_{n-1}))  (:139-143);   z_n = b_n - f^T u_n  (:144).
 * THE TEMPLATE b_k is a box (tau = 0) or a trapezoid of full width w with ramps of length tau, centred on t0 and, for
 * P > 0, on every t0 + m P; P = 0 is a single event.  Every line below is rounded once and none is contracted into an fma,
 * so a host restatement in IEEE double precision takes the same discrete decisions bit for bit:
 *   invP = 1 / P            (once per trial; correctly rounded division; unused when P == 0)
 *   x    = t_n - t0
 *   q    = rint(x * invP)   (round-half-even; 0 when P == 0)
 *   phi  = x - q * P        (the product rounded, then the difference; phi = x when P == 0)
 *   u    = 0.5 * w - |phi|
 *   b_n  = 0 if u < 0;   1 if u >= tau;   u / tau otherwise        (tau = 0: the box, closed at both edges)
 * Times with a large offset (Julian dates) keep their accuracy because x is formed first.  The rule is evaluated as written
 * for any trial; a caller masks the results of trials outside w > 0, 0 <= tau <= w / 2, P >= 0, w <= P when P > 0.
 * Each element of T is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  1 <= J <= C2_FAST_WIDTH and 1 <= Q0 <= 8 (beyond either: C2_ERR_UNSUPPORTED); B, N, K >= 1;
 * B * ceil(K / 64) < 2^31 blocks (C2_ERR_UNSUPPORTED).  A null pointer or a bad size: C2_ERR_INVALID before any launch.
 * T must not alias an input.  Rows of a series whose factorisation failed hold garbage (never another series'). */
int c2_whitened_transits(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                         const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                         const double *Z0 /* (B, N, Q0) */, const double *trials /* (K, 4) | (B, K, 4) */,
                         int64_t tr_bs /* 0: shared (K, 4) */, double *T /* (B, K, 1 + Q0) */, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_TRANSIT_H_ */
