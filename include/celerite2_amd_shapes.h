/* =============================================================================
 * celerite2_amd_shapes.h -- the search for events of a TABULATED SHAPE under
 * correlated noise on the factored covariance, and the projection of many
 * vectors on the same columns (what its false-alarm probability reads).  The
 * seventh public header of libcelerite2_amd.so (the first, celerite2_amd.h, is
 * included for c2_stream_t and the error codes; the second to sixth are
 * celerite2_amd_linear.h, celerite2_amd_periodogram.h, celerite2_amd_transit.h,
 * celerite2_amd_kepler.h and celerite2_amd_trials.h).  Same conventions:
 * float64, row-major, contiguous DEVICE pointers, a leading batch dimension B
 * of independent series, batch strides in elements (0 when shared by the
 * batch), the launch goes on `stream` and the call returns without
 * synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_SHAPES_H_
#define CELERITE2_AMD_SHAPES_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles of a shape bank, NS * S, at most (beyond it: C2_ERR_UNSUPPORTED; a larger bank takes several calls). */
#define C2_SHAPE_MAX_NODES 1024

/* Vectors one wavefront of c2_shape_projections takes beside its 16 trials (a multiple of 16): the block of R in its grid. */
#define C2_SHAPE_DRAWS 32

/* THE COLUMN.  A shape bank `shapes` is (NS, S) doubles, shared by the batch (sh_bs == 0) or per series (B, NS, S)
 * (sh_bs == NS S); NS >= 1, S >= 2, NS S <= C2_SHAPE_MAX_NODES.  A shape is an event profile tabulated on a uniform grid
 * across its full width w: node i sits at the signed offset -w/2 + i w / (S - 1) from the event centre, node 0 at the leading
 * edge and node S - 1 at the trailing edge (asymmetric shapes are first class), and the profile between two nodes is their
 * linear interpolant.  A trial is four doubles (P, t0, w, s): period (0: a single event), epoch of the centre, full width,
 * and the shape's index as a double holding an integer in [0, NS); trials are shared by the batch (K,4) (tr_bs == 0) or
 * (B,K,4) (tr_bs == 4 K).  Every line below is rounded once and none is contracted into an fma, so a host restatement in
 * IEEE double precision takes the same discrete decisions bit for bit; the lines up to u are those of
 * celerite2_amd_transit.h, so which side of an edge or of a fold a sample falls on is that header's decision to the bit:
 *   invP = 1 / P                                  (once per trial; correctly rounded division; 0 when P == 0)
 *   ginv = fl(S - 1) / w                          (once per trial; correctly rounded division)
 *   is   = (s >= 0 && s < NS) ? (int)s : 0        (truncation; a NaN s takes 0: the index is CLAMPED, never trusted)
 *   x    = t_n - t0
 *   q    = rint(x * invP)                         (round-half-even; 0 when P == 0)
 *   phi  = x - q * P                              (the product rounded, then the difference; phi = x when P == 0)
 *   u    = 0.5 * w - |phi|
 *   v    = phi + 0.5 * w
 *   g    = v * ginv;   g = g > 0 ? g : 0;   g = g < S - 1 ? g : S - 1          (a NaN g takes 0)
 *   i    = min((int)floor(g), S - 2);   fr = g - i                            (exact)
 *   dlt  = shape[is][i + 1] - shape[is][i]
 *   b_n  = 0 if u < 0;   otherwise shape[is][i] + fr * dlt                    (the product rounded, then the sum)
 * (closed at both edges, like the box; a NaN u is not below 0).  The rule is evaluated as written for any trial, and no
 * trial content can make it read outside the bank: is is in [0, NS) and i in [0, S - 2] whatever the trial holds.  A caller
 * masks the results of trials outside w > 0, P >= 0, w <= P when P > 0, t0 finite and s an integer in [0, NS).  With an
 * all-ones S = 2 bank b_n is the box of celerite2_amd_transit.h (tau = 0) bit for bit; with w = P the shape is a full
 * phase-folded periodic template.  Times with a large offset (Julian dates) keep their accuracy because x is formed first. */

/* Whitened shapes of a trial grid: with d, W of c2_factor (K + D = L diag(d) L^T), Z0 = L^-1 [A0 | y - mean] (B,N,Q0) of
 * c2_solve_lower, for every series b and trial k
 *   z = L^-1 b_k(t),   <a, b> = sum_n a_n b_n / d_n,   T[b,k,:] = [<z,z>, <z,Z0[:,j]> for j < Q0]            (1 + Q0 values)
 * -- the layout and meaning of c2_whitened_transits -- in ONE forward sweep that forms the column in registers, one lane per
 * trial, and writes neither it nor z (csrc/c2_shapes.hip).  The sweep is internal::forward with one right-hand side
 * (internal.hpp:107-146):  f <- p_n o (f + w_{n-1} z_{n-1}),  p_n = exp(-c (t_n - t_{n-1}));   z_n = b_n - f^T u_n.
 * Each element of T is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  1 <= J <= C2_FAST_WIDTH and 1 <= Q0 <= 8, NS S <= C2_SHAPE_MAX_NODES (beyond any: C2_ERR_UNSUPPORTED); B, N, K,
 * NS >= 1, S >= 2; B * ceil(K / 64) < 2^31 blocks (C2_ERR_UNSUPPORTED).  A null pointer or a bad size: C2_ERR_INVALID before
 * any launch.  T must not alias an input.  Rows of a series whose factorisation failed hold garbage (never another
 * series'). */
int c2_whitened_shapes(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                       const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                       const double *Z0 /* (B, N, Q0) */, const double *trials /* (K, 4) | (B, K, 4) */,
                       int64_t tr_bs /* 0: shared (K, 4) */, double *T /* (B, K, 1 + Q0) */,
                       const double *shapes /* (NS, S) | (B, NS, S) */, int64_t sh_bs /* 0: shared (NS, S) */, int64_t NS,
                       int64_t S, c2_stream_t stream);

/* Projections on the columns of the same trials: for alpha (B,N,R), every series b, trial k and vector r
 *   P[b,k,r] = sum_n b_k(t[b,n]) * alpha[b,n,r]                                                       (R innermost)
 * in ONE pass that forms the column in registers -- by the rule above, bit for bit the values c2_whitened_shapes whitens --
 * and contracts it with alpha on the matrix cores (csrc/c2_shape_project.hip): c2_trial_projections
 * (celerite2_amd_trials.h) for a one-column kind, which has the identities.  With alpha[:, r] = (K + D)^-1 (y_r - mean),
 * P[b,k,r] is the entry T[1 + P0] of the sweep for y_r.  Each element of P is written by exactly one lane: no atomics, two
 * calls give identical bits.  No allocation and no host read.  B, N, K, R, NS >= 1, S >= 2; NS S <= C2_SHAPE_MAX_NODES and
 * B * ceil(K / 16) * ceil(R / C2_SHAPE_DRAWS) < 2^31 blocks (C2_ERR_UNSUPPORTED).  A null pointer or a bad size:
 * C2_ERR_INVALID before any launch.  P must not alias an input. */
int c2_shape_projections(int64_t B, int64_t N, int64_t K, int64_t R, const double *t, int64_t t_bs,
                         const double *trials /* (K, 4) | (B, K, 4) */, int64_t tr_bs /* 0: shared */,
                         const double *alpha /* (B, N, R) */, double *P /* (B, K, R) */,
                         const double *shapes /* (NS, S) | (B, NS, S) */, int64_t sh_bs /* 0: shared (NS, S) */, int64_t NS,
                         int64_t S, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_SHAPES_H_ */
