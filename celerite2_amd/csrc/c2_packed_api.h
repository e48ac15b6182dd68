/* =============================================================================
 * c2_packed_api.h -- RAGGED BATCHES: the exact log-likelihood, and its gradient,
 * of B series of different lengths stored row-packed with offsets.  A PROVISIONAL
 * interface of libcelerite2_amd.so: the three functions below are exported by the
 * library and bound by celerite2_amd/packed.py, which parses this file as
 * celerite2_amd/_lib.py parses the public headers, but the file is not under
 * include/ and its prototypes may still change (INTEGRATION.md says what promotion
 * takes).  Conventions of the public headers otherwise: float64, row-major,
 * contiguous DEVICE pointers, the launches go on `stream` and the call returns
 * without synchronising.  celerite2_amd.h is included for c2_stream_t and the
 * error codes.
 *
 * Layout.  offsets (B+1,) int64 with offsets[0] = 0, offsets[B] = R; series b owns rows offsets[b] .. offsets[b+1]-1 of
 * t, a, y (R,) and U, V (R, J).  c is (J,) (c_bs == 0) or (B, J) (c_bs == J).  Times are sorted within a series; nothing is
 * assumed across a series boundary: the first row of a series starts from S = 0, F = 0 with p := 0 (the recursion of
 * celerite2_amd_filter.h from the empty state), and no difference to the previous series' last time is formed.  A series
 * of length 0 gives ll = 0, flag = 0 and touches no row.  The kernels take a series' rows as
 * [max(offsets[b], 0), min(offsets[b+1], R)) and a negative length as 0: malformed offsets give wrong numbers, but no access
 * outside the arrays.
 *
 * order (B,) int32, nullable: grid slot s works on series order[s] (a permutation of 0 .. B-1; lengths in descending order
 * put series of similar length into one wavefront, whose trip count is its longest series).  No result depends on it by
 * a bit.
 *
 * Values.  ll[b] = -1/2 sum_n (z_n^2 / d_n + log d_n) - 1/2 N_b log 2 pi, with d, W of c2_factor and z of c2_solve_lower
 * of that series.  flag[b] is the 1-based row WITHIN THE SERIES of the first d <= 0, or 0 (a NaN pivot passes, as in
 * c2_factor).  A failed series has ll = -inf and NaN in its rows of every gradient and in its row of bc; of d, W, z it
 * keeps the rows before the failing one and the failing row's d (the pivot that failed), and has NaN in W, z of the failing
 * row and in d, W, z of every row behind it.  No element of any output is left unwritten, and no other series is affected.
 *
 * 1 <= J <= C2_FAST_WIDTH (beyond: C2_ERR_UNSUPPORTED), B >= 1, R >= 0, 0 <= Nmax <= 2^30 (a series is
 * cut at 2^30 rows, R itself is not limited).  A null among the required
 * pointers, or work_bytes below the query, gives C2_ERR_INVALID before anything is launched.  Every output element has
 * one writer; no atomics, no allocation, no host read (the calls can be captured in a graph); two calls give identical
 * bits and nothing depends on what the outputs or `work` held before.  No output may alias an input or another output.
 * csrc/c2_packed.hip.
 * ============================================================================= */
#ifndef CELERITE2_AMD_PACKED_API_H_
#define CELERITE2_AMD_PACKED_API_H_

#include "../../include/celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of `work` for c2_packed_loglik_grad, with C = max(1, ceil(sqrt(Nmax))) the checkpoint interval:
 *   8 * (R * (J + 2) + 2 * B * C * (J^2 + J) + 32)
 * -- d, z and W of every row, then per series C checkpoints (F, S) (one per C rows) and a ring of C states (the ones the
 * rows of the segment in hand start from), and 32 doubles that the last row of the ring may be read into.  Nmax is an upper bound of the lengths (a longer series is cut at Nmax rows).
 * 0 outside 1 <= J <= C2_FAST_WIDTH, B >= 1, R >= 0, 0 <= Nmax <= 2^30. */
size_t c2_packed_loglik_grad_workspace_bytes(int64_t B, int64_t R, int64_t Nmax, int64_t J);

/* The log-likelihood of every series: ll (B,), flag (B,).  d (R,), W (R, J), z (R,) are nullable, each on its own: given,
 * the call is also the packed c2_factor + c2_solve_lower. */
int c2_packed_loglik(int64_t B, int64_t R, int64_t J, const int64_t *offsets, const int32_t *order, const double *t,
                     const double *c, int64_t c_bs, const double *a, const double *U, const double *V, const double *y,
                     double *ll, int32_t *flag, double *d, double *W, double *z, c2_stream_t stream);

/* ... and its gradient: bt, ba, by (R,), bU, bV (R, J), bc (B, J) -- per series also when c is shared (the caller sums).
 * The forward pass keeps d, W, z of every row and the state after every C-th row of a series in `work`; the reverse walks a
 * series' segments of C rows from the last to the first, replays a segment's states from its checkpoint into the ring and
 * then walks the segment's rows backwards (the reverse of c2_filter_append with the cotangent -1/2 on the two sums of the
 * final state and 0 elsewhere).  No state per row is kept. */
int c2_packed_loglik_grad(int64_t B, int64_t R, int64_t Nmax, int64_t J, const int64_t *offsets, const int32_t *order,
                          const double *t, const double *c, int64_t c_bs, const double *a, const double *U, const double *V,
                          const double *y, double *ll, double *bt, double *bc, double *ba, double *bU, double *bV, double *by,
                          int32_t *flag, void *work, size_t work_bytes, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_PACKED_API_H_ */
