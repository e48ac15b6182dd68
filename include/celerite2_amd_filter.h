/* =============================================================================
 * celerite2_amd_filter.h -- streaming updates of a factored GP: the tenth public
 * header of libcelerite2_amd.so (the first, celerite2_amd.h, is included for
 * c2_stream_t and the error codes).  Same conventions: float64, row-major,
 * contiguous DEVICE pointers, a leading batch dimension B of independent series,
 * batch strides in elements (0 when shared by the batch), the launch goes on
 * `stream` and the call returns without synchronising.
 *
 * Everything rows 0 .. n-1 of a series contribute to row n of the reference's
 * factor and solve_lower (c++/include/celerite2/forward.hpp:69-135, 156-170)
 * passes through the J x J state S and the J-vector F of those two recursions.
 * A FILTER STATE keeps them, so that rows are appended in O(M J^2) without the
 * old rows; the d and z of an appended row are its one-step-ahead predictive
 * variance and its innovation.  No counterpart in the reference, which factors
 * whole series; parity is pinned by its factor + solve_lower of the whole series
 * and by dense conditioning.
 *
 * State layout (public): (B, SW) doubles, SW = c2_filter_state_words(J) =
 * 4 + J + J^2, series-major, per series
 *   [0] t_last   [1] n (rows absorbed, as a double)   [2] sum log d   [3] sum z^2 / d
 *   [4 .. 4+J)   F
 *   [4+J .. SW)  S, row-major, BOTH triangles, S[i,j] == S[j,i] to the bit
 * with F and S including the last row's own contribution and not yet propagated:
 *   S = sum_k d_k (e_k o w_k)(e_k o w_k)^T,  F = sum_k (e_k o w_k) z_k,  e_k = exp(-c (t_last - t_k)).
 * An all-zero state is the empty one (n = 0).  log-likelihood = -(1/2) ([3] + [2] + n log 2 pi).
 *
 * One row (t, a, u, v, y), with p = exp(-c (t - t_last)) and p := 0 when n == 0 (whatever t_last holds):
 *   S <- (p p^T) o S ;  F <- p o F
 *   g = S u ;  d = a - u^T g ;  w = (v - g) / d ;  z = y - u^T F                       (append)
 *   S <- S + d w w^T ;  F <- F + w z ;  t_last <- t ;  n += 1 ;  [2] += log d ;  [3] += z^2 / d
 *
 * Ragged updates: `count` (B,) int32, nullable (= M everywhere), 0 <= count[b] <= M (the caller's responsibility; a value
 * outside is clamped).  Rows m >= count[b] are not read and their outputs are not written; a series with count 0 keeps its
 * state bit for bit.  The times of a series must be non-decreasing and not before its t_last: not checked here.
 *
 * Aliasing: `state_out` may be `state_in` (in-place streaming); otherwise the two must not overlap.  No other output may
 * alias an input or another output.  1 <= J <= C2_FAST_WIDTH (beyond: C2_ERR_UNSUPPORTED), B, M >= 1, M < 2^31.
 * No atomics: two calls give identical bits.  csrc/c2_filter.hip.
 * ============================================================================= */
#ifndef CELERITE2_AMD_FILTER_H_
#define CELERITE2_AMD_FILTER_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles per series of a filter state, 4 + J + J^2; 0 outside 1 <= J <= C2_FAST_WIDTH. */
int64_t c2_filter_state_words(int64_t J);

/* Append up to M rows per series: t (B,M) (t_bs == M) or shared (M,) (t_bs == 0), c (B,J) or (J,), a, y (B,M), U, V (B,M,J)
 * -> d, z (B,M), W (B,M,J), the new state and flag (B,).  flag[b] is the 1-based index within this call of the first
 * appended row with d <= 0, or 0 (a NaN pivot passes the test, as in c2_factor); the rows before it are written to d, W, z
 * and the failing row's d, the failing series' state is left exactly as on entry, and no other series is affected. */
int c2_filter_append(int64_t B, int64_t M, int64_t J, const double *state_in, double *state_out, const double *t, int64_t t_bs,
                     const double *c, int64_t c_bs, const double *a, const double *U, const double *V, const double *y,
                     const int32_t *count, double *d, double *W, double *z, int32_t *flag, c2_stream_t stream);

/* Absorb rows of an EXISTING factorisation: d, z (B,M) and W (B,M,J) of c2_factor and c2_solve_lower; only the decay and the
 * update line above are applied (no division, no failure).  Absorbing a whole series into the empty state gives the state
 * the appends of its rows would have given, without refactoring. */
int c2_filter_absorb(int64_t B, int64_t M, int64_t J, const double *state_in, double *state_out, const double *t, int64_t t_bs,
                     const double *c, int64_t c_bs, const double *W, const double *d, const double *z, const int32_t *count,
                     c2_stream_t stream);

/* Forecast at M query rows per series, each independently from the same, unchanged state: a (B,M), U (B,M,J) ->
 *   mu = u^T (p o F),   var = a - u^T ((p p^T) o S) u,   p = exp(-c (t - t_last))
 * mu, var (B,M): for t >= t_last the full conditional of a row (a, u) at t given all absorbed rows.  A time before t_last is
 * not checked and its result is no conditional (the rows after it would enter with the roles of u and v exchanged).  An
 * empty state gives mu = 0, var = a. */
int c2_filter_forecast(int64_t B, int64_t M, int64_t J, const double *state, const double *t, int64_t t_bs, const double *c,
                       int64_t c_bs, const double *a, const double *U, const int32_t *count, double *mu, double *var,
                       c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_FILTER_H_ */
