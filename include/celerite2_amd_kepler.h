/* =============================================================================
 * celerite2_amd_kepler.h -- the Keplerian search (the radial-velocity
 * periodogram of an eccentric orbit) under correlated noise on the factored
 * covariance: the fifth public header of libcelerite2_amd.so (the first,
 * celerite2_amd.h, is included for c2_stream_t and the error codes; the second
 * to fourth are celerite2_amd_linear.h, celerite2_amd_periodogram.h and
 * celerite2_amd_transit.h).  Same conventions: float64, row-major, contiguous
 * DEVICE pointers, a leading batch dimension B of independent series, batch
 * strides in elements (0 when shared by the batch), the launch goes on `stream`
 * and the call returns without synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_KEPLER_H_
#define CELERITE2_AMD_KEPLER_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest eccentricity of the domain: the solver below reaches rounding level up to it. */
#define C2_KEPLER_MAX_ECC 0.99

/* Whitened Keplerian columns of a trial grid: with d, W of c2_factor (K + D = L diag(d) L^T), Z0 = L^-1 [A0 | y - mean]
 * (B,N,Q0) of c2_solve_lower and the trials (angular frequency w = 2 pi / P, eccentricity e, time of periastron tp), three
 * doubles each, shared by the batch (K,3) (tr_bs == 0) or (B,K,3) (tr_bs == 3 K), for every series b and trial k, with nu(t)
 * the true anomaly of the orbit (w, e, tp) at time t,
 *   z_c = L^-1 cos nu,   z_s = L^-1 sin nu,   <a, b> = sum_n a_n b_n / d_n
 *   T[b,k,:] = [<z_c,z_c>, <z_c,z_s>, <z_s,z_s>, <z_c,Z0[:,j]> for j < Q0, <z_s,Z0[:,j]> for j < Q0]      (3 + 2 Q0 values)
 * -- the layout of c2_whitened_sinusoids -- in ONE forward sweep that solves Kepler's equation and forms both columns in
 * registers, one lane per trial (two above J = 16), and writes neither them nor z_c, z_s (csrc/c2_kepler.hip).  The model
 * y = mean + A0 beta0 + K [cos(nu + omega) + e cos omega] + GP is linear in (alpha, beta) = (K cos omega, -K sin omega) on
 * these two columns, its constant K e cos omega absorbed by a constant column of A0: with S0 = Z0^T diag(1/d) Z0 these are
 * all the products its generalized least-squares fit reads, per trial.  The sweep is internal::forward with two right-hand
 * sides (internal.hpp:107-146):
 *   F <- p_n o (F + w_{n-1} z_{n-1}^T),  p_n = exp(-c (t_n - t_{n-1}))  (:139-143);   z_n = a_n - F^T u_n  (:144).
 *
 * THE COLUMNS.  The mean anomaly is reduced exactly; every line is rounded once and nothing is contracted except the fma
 * that is named:
 *   x  = fl(w * fl(t_n - tp))            (the periodogram's phase: Julian dates keep their accuracy with tp at the offset)
 *   q  = rint(fl(x * INV_2PI))           (INV_2PI = fl(1 / fl(2 pi)) = 0x1.45f306dc9c883p-3; round-half-even)
 *   r  = fma(-q, TWO_PI, x)              (TWO_PI = fl(2 pi) = 0x1.921fb54442d18p+2; EXACT: the IEEE remainder of x by the
 *                                         double TWO_PI -- next to a half turn possibly its other side: q carries the
 *                                         rounding of x * INV_2PI, so |r| <= pi (1 + (|q| + 1) 2^-51), which is
 *                                         pi (1 + 2^-50) for |q| <= 1 and below pi (1 + 1e-9) for |x| <= 1e7; a host
 *                                         restatement has r bit for bit)
 *   a  = |r|
 * Kepler's equation E - e sin E = a is solved by a fixed sequence, the same for every row and trial (no loop whose length
 * depends on the data); se = sin e, ce = cos e and b = sqrt(fl(1 - e e)) are formed once per trial:
 *   (sa, ca) = sincos(a)
 *   E  = min(a + e,  a + e sa / ((1 - (sa ce + ca se)) + sa))                        (the starter)
 *   three times:   (s, c) = sincos(E);   E = E + delta(E, s, c)                      (Danby's quartic step)
 *   (s, c) <- (s cd + c sd,  c cd - s sd),  sd = delta (1 + delta^2 (-1/6 + delta^2 / 120)),
 *                                           cd = 1 + delta^2 (-1/2 + delta^2 / 24)    (delta: the third step's, < 2e-3)
 *   E  = E + delta(E, s, c)                                                          (the fourth step, on the rotated pair)
 *   (s, c) <- (s + c delta,  c - s delta)                                            (delta: the fourth step's, < 1e-11)
 * where, with f = (E - e s) - a, f1 = 1 - e c, f2 = e s, f3 = e c,
 *   d1 = -f / f1;   d2 = -f / (f1 + d1 f2 / 2);   delta = -f / (f1 + d2 f2 / 2 + d2^2 f3 / 6).
 * Then
 *   g = 1 / (1 - e c);   cos nu = (c - e) g;   sin nu = copysign(1, r) (b s g)
 * so cos nu is exactly even and sin nu exactly odd in r (the sign is applied, not forced: a may pass pi as above, and the
 * solver takes it there).  Reciprocals are taken to full precision (a hardware seed and two Newton steps), then multiplied.
 * Four steps reach rounding level for every e <= C2_KEPLER_MAX_ECC: |E - E*| (1 - e cos E*)
 * stays below 16 * 2^-52 against a bracketed extended-precision solution E*.
 * The rule is evaluated as written for any trial; a caller masks the results of trials outside w > 0,
 * 0 <= e <= C2_KEPLER_MAX_ECC, tp finite.
 * Each element of T is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  1 <= J <= C2_FAST_WIDTH and 1 <= Q0 <= 8 (beyond either: C2_ERR_UNSUPPORTED); B, N, K >= 1;
 * B * ceil(K / 64) < 2^31 blocks, B * ceil(K / 32) above J = 16 (C2_ERR_UNSUPPORTED).  A null pointer or a bad size:
 * C2_ERR_INVALID before any launch.  T must not alias an input.  Rows of a series whose factorisation failed hold garbage
 * (never another series'). */
int c2_whitened_keplerians(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                           const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                           const double *Z0 /* (B, N, Q0) */, const double *trials /* (K, 3) | (B, K, 3): (w, e, tp) */,
                           int64_t tr_bs /* 0: shared (K, 3) */, double *T /* (B, K, 3 + 2 * Q0) */, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_KEPLER_H_ */
