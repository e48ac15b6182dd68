/* =============================================================================
 * celerite2_amd_linear.h -- linear mean models on the factored covariance: the
 * second public header of libcelerite2_amd.so (the first, celerite2_amd.h, is
 * included for c2_stream_t and the error codes).  Same conventions: float64,
 * row-major, contiguous DEVICE pointers, a leading batch dimension B of
 * independent series, batch strides in elements (0 when shared by the batch),
 * the launch goes on `stream` and the call returns without synchronising.
 *
 * No counterpart in the reference, whose callers compose generalized least
 * squares from solve_lower (c++/include/celerite2/forward.hpp:158-170) and a
 * dense product; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_LINEAR_H_
#define CELERITE2_AMD_LINEAR_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Whitened Gram matrix of a design matrix: with d, W of c2_factor (K + D = L diag(d) L^T), A (N,P) shared by the batch
 * (a_bs == 0) or (B,N,P) (a_bs == N * P) and optionally y (B,N),
 *   S[b] = [A | y]^T (K + D)^-1 [A | y] = sum_n z_n z_n^T / d_n,   z = L^-1 [A | y]      (Q = P + 1 columns, P if y is NULL)
 * in ONE forward sweep that accumulates S in registers and never writes Z (csrc/c2_gram.hip; O(N (J + Q) Q) per series,
 * 8 N (2 J + Q + 2) bytes read).  The sweep is internal::forward with Q right-hand sides (internal.hpp:107-146):
 *   F <- p_n o (F + w_{n-1} z_{n-1}^T),  p_n = exp(-c (t_n - t_{n-1}))  (:139-143);   z_n = y_n - F^T u_n  (:144).
 * S (B,Q,Q) holds both triangles, y's column last, S[b,i,k] == S[b,k,i] to the bit; two calls give identical bits (no
 * atomics).  The blocks are what generalized least squares reads: S_AA = S[:P,:P], s_Ay = S[:P,P], s_yy = S[P,P].
 * 1 <= J <= C2_FAST_WIDTH and Q <= 32 (beyond either: C2_ERR_UNSUPPORTED); B, N, P >= 1.  S must not alias an input.
 * Rows of a series whose factorisation failed hold garbage (never another series'). */
int c2_whitened_gram(int64_t B, int64_t N, int64_t J, int64_t P, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                     const double *U, const double *W, const double *d, const double *A, int64_t a_bs /* 0: shared (N, P) */,
                     const double *y /* (B, N) or NULL */, double *S /* (B, Q, Q) */, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_LINEAR_H_ */
