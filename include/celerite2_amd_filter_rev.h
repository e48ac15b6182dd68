/* =============================================================================
 * celerite2_amd_filter_rev.h -- the reverse of c2_filter_append: the eleventh
 * public header of libcelerite2_amd.so (the first, celerite2_amd.h, is included
 * for c2_stream_t and the error codes; the tenth, celerite2_amd_filter.h, has the
 * forward call, the state layout and the row recursion).  Same conventions:
 * float64, row-major, contiguous DEVICE pointers, a leading batch dimension B of
 * independent series, batch strides in elements (0 when shared by the batch), the
 * launch goes on `stream` and the call returns without synchronising.
 *
 * A filter state is an argument AND a result of an append, so its cotangent is
 * carried from one call to the previous one: bstate_out (B, SW) in, bstate_in
 * (B, SW) out, in the layout of the state itself,
 *   [0] b t_last   [1] b n   [2] b sum log d   [3] b sum z^2 / d   [4 .. 4+J) b F   [4+J .. SW) b S.
 * With d and z the one-step-ahead predictive variance and the innovation of a row, a loss on words [2] and [3] of the last
 * state (-(1/2) ([3] + [2] + n log 2 pi) is the log-likelihood) flows back through as many calls as states were kept.
 *
 * Conventions of the state cotangent:
 *   - The S block is the SYMMETRIC REPRESENTATIVE.  A state's S is symmetric for every value of every parameter, so a
 *     cotangent B of it acts only through (B + B^T) / 2: the call replaces the incoming block by that and returns a symmetric
 *     one.  (Exact for every use; it lets one lane hold column j = row j of b S.)
 *   - Word [0] of bstate_out is added to bt of the last taken row (t_last is that row's time).  For the first row of a call
 *     the cotangent of the time before it goes to word [0] of bstate_in; an empty entry state (n == 0) gets 0 there, and 0 in
 *     its F and S blocks: its rows start from p = 0, whatever t_last holds.
 *   - Words [1], [2], [3] pass through to bstate_in; [2] and [3] also feed every row (b d += [2] / d - [3] z^2 / d^2,
 *     b z += 2 [3] z / d).
 *
 * Rows m >= count[b] of bt, ba, bU, bV, by are WRITTEN AS ZEROS, so the outputs may be uninitialised.  A series with
 * count 0 or flag != 0 was passed through by the forward call: it gets bstate_in = bstate_out (word for word), bc = 0 and
 * every row cotangent 0 -- nothing is propagated through the rows of a failed call.  bt is (B, M) and bc (B, J) PER SERIES
 * also when t or c are shared by the batch (the caller sums).
 *
 * No output may alias an input or another output.  1 <= J <= C2_FAST_WIDTH (beyond: C2_ERR_UNSUPPORTED), B, M >= 1,
 * M < 2^31.  No atomics: two calls give identical bits.  csrc/c2_filter_rev.hip.
 * ============================================================================= */
#ifndef CELERITE2_AMD_FILTER_REV_H_
#define CELERITE2_AMD_FILTER_REV_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Doubles of scratch per ROW of c2_filter_append_rev, J + J^2 (the F and S a row starts from); 0 outside
 * 1 <= J <= C2_FAST_WIDTH. */
int64_t c2_filter_rev_workspace_words(int64_t J);

/* Reverse of c2_filter_append.  state_in (B, SW): the state the forward call STARTED from; t, c, U, count as given to it;
 * W (B,M,J), d, z (B,M), flag (B,) as it returned them.  Cotangents in: bstate_out (B, SW), bd, bz (B,M), bW (B,M,J), the
 * last three nullable (= 0).  ws (B, M, J + J^2): scratch, filled and read by this call (the states are replayed from
 * state_in with the update line of the forward call -- no division, the same bits -- so neither a, V, y nor anything kept
 * by the forward call is needed).  Cotangents out: bstate_in (B, SW), bt (B,M), bc (B,J), ba, by (B,M), bU, bV (B,M,J). */
int c2_filter_append_rev(int64_t B, int64_t M, int64_t J, const double *state_in, const double *t, int64_t t_bs, const double *c,
                         int64_t c_bs, const double *U, const double *W, const double *d, const double *z, const int32_t *count,
                         const int32_t *flag, const double *bstate_out, const double *bd, const double *bW, const double *bz,
                         double *ws, double *bstate_in, double *bt, double *bc, double *ba, double *bU, double *bV, double *by,
                         c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_FILTER_REV_H_ */
