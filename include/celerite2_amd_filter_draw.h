/* =============================================================================
 * celerite2_amd_filter_draw.h -- forecast sample paths: joint draws of the future
 * from a filter state; the thirteenth public header of libcelerite2_amd.so (the
 * tenth, celerite2_amd_filter.h, is included for the state layout and the
 * conventions: float64, row-major, contiguous DEVICE pointers, a leading batch
 * dimension B of independent series, batch strides in elements (0 when shared by
 * the batch), the launch goes on `stream` and the call returns without
 * synchronising).
 *
 * c2_filter_forecast gives a mean and a variance per query row, each on its own.
 * The future of a correlated process is a path: drawing the M query rows one after
 * the other is the append run "backwards in y".  Per row, after the decay
 *   S <- (p p^T) o S ;  F_k <- p o F_k                      (p := 0 when n == 0)
 *   g = S u ;  d = a - u^T g ;  w = (v - g) / d              as in c2_filter_append
 *   per draw k:  z_k = sqrt(d) eps_k ;  y_k = u^T F_k + z_k ;  F_k <- F_k + w z_k
 *   S <- S + d w w^T
 * so S, d and w are shared by the K draws and only the J-vector F is per draw:
 * O(M (J^2 + J K)) per series.  y = mu_c + L_c D_c^(1/2) eps is mu_c + chol(Sigma_c) eps
 * for the dense conditional mean and covariance of the M rows given every absorbed
 * row.  a = k(0) + diag gives draws of would-be observations, a = k(0) draws of the
 * latent process (a repeated query time then has d = 0 and is flagged).
 *
 * d and flag come out with the bits c2_filter_append writes for the same rows
 * (neither depends on y); sqrt is the correctly rounded one; draw k's path has the
 * same bits whatever K is.  No atomics: two calls give identical bits.  The state is
 * read and never written.  No output may alias an input or another output.
 * csrc/c2_filter_draw.hip.
 * ============================================================================= */
#ifndef CELERITE2_AMD_FILTER_DRAW_H_
#define CELERITE2_AMD_FILTER_DRAW_H_

#include "celerite2_amd_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Draws one pass of the kernel carries at width J (further draws go to further blocks, which repeat the O(J^2) part of a
 * row); 0 outside 1 <= J <= C2_FAST_WIDTH. */
int64_t c2_filter_draw_chunk(int64_t J);

/* K joint draws at M query rows per series: state (B, SW), t (B,M) (t_bs == M) or shared (M,) (t_bs == 0), c (B,J) or (J,),
 * a (B,M), U, V (B,M,J) the celerite matrices of the query rows, eps (B,M,K) standard normals, draw-fastest
 * -> paths (B,M,K), d (B,M), flag (B,).  `count` as in c2_filter_append: rows m >= count[b] are neither read nor written.
 * flag[b] is the 1-based row with d <= 0, else 0 (a NaN pivot passes); a failed series keeps the rows of paths and d written
 * before the failing one, the failing row's d is written and nothing behind it.  The times must be non-decreasing and not
 * before t_last: not checked here.  B, M, J, K >= 1 (else C2_ERR_INVALID); J > C2_FAST_WIDTH, M >= 2^31 or
 * K > 65535 c2_filter_draw_chunk(J) give C2_ERR_UNSUPPORTED; a null among the pointers other than `count` C2_ERR_INVALID. */
int c2_filter_draw(int64_t B, int64_t M, int64_t J, int64_t K, const double *state, const double *t, int64_t t_bs,
                   const double *c, int64_t c_bs, const double *a, const double *U, const double *V, const double *eps,
                   const int32_t *count, double *paths, double *d, int32_t *flag, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_FILTER_DRAW_H_ */
