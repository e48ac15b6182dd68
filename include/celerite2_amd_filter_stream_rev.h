/* =============================================================================
 * celerite2_amd_filter_stream_rev.h -- the reverse of c2_filter_forecast and of
 * c2_filter_absorb: the twelfth public header of libcelerite2_amd.so (the first,
 * celerite2_amd.h, is included for c2_stream_t and the error codes; the tenth,
 * celerite2_amd_filter.h, has the forward calls, the state layout and the row
 * recursion; the eleventh, celerite2_amd_filter_rev.h, has the reverse of the
 * append and the conventions of a state cotangent, which hold here word for word).
 * Same conventions: float64, row-major, contiguous DEVICE pointers, a leading batch
 * dimension B of independent series, batch strides in elements (0 when shared by the
 * batch), the launch goes on `stream` and the call returns without synchronising.
 *
 * A state cotangent has the layout of the state,
 *   [0] b t_last   [1] b n   [2] b sum log d   [3] b sum z^2 / d   [4 .. 4+J) b F   [4+J .. SW) b S,
 * its S block the SYMMETRIC REPRESENTATIVE: what a call returns is symmetric to the bit, and an incoming block B acts as
 * (B + B^T) / 2.
 *
 * FORECAST reads a state and changes nothing, so its reverse RETURNS a state cotangent (to be added to whatever else the
 * state feeds): word [0] is minus the sum of bt over the taken rows, words [1], [2], [3] are 0, the F and S blocks are
 * sum_m bmu_m x_m and -sum_m bvar_m x_m x_m^T with x = exp(-c (t_m - t_last)) o u_m.  An empty state (n == 0) gives
 * ba = bvar and zeros everywhere else: its rows have p = 0 whatever t_last holds.  It needs neither a nor mu, var.
 *
 * ABSORB takes a state to a state, so its cotangent is carried like that of an append: bstate_out (B, SW) in, bstate_in
 * (B, SW) out.  Word [0] of bstate_out is added to bt of the last taken row; for the first row of a call the cotangent of
 * the time before it goes to word [0] of bstate_in (0, and 0 in the F and S blocks, for an empty entry state).  Words
 * [1], [2], [3] pass through; [2] and [3] also feed every row (bd = [2] / d - [3] z^2 / d^2 + ..., bz = 2 [3] z / d + ...).
 *
 * Rows m >= count[b] of the row cotangents are WRITTEN AS ZEROS, so the outputs may be uninitialised.  A series with
 * count 0 gets a zero bstate from the forecast reverse and bstate_in = bstate_out (word for word) from the absorb reverse,
 * bc = 0 from both.  bt is (B, M) and bc (B, J) PER SERIES also when t or c are shared by the batch (the caller sums).
 *
 * No output may alias an input or another output.  1 <= J <= C2_FAST_WIDTH (beyond: C2_ERR_UNSUPPORTED), B, M >= 1,
 * M < 2^31.  No atomics: two calls give identical bits.  csrc/c2_filter_stream_rev.hip.
 * ============================================================================= */
#ifndef CELERITE2_AMD_FILTER_STREAM_REV_H_
#define CELERITE2_AMD_FILTER_STREAM_REV_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Reverse of c2_filter_forecast.  state (B, SW), t, c, U (B,M,J), count (nullable) as given to the forward call.
 * Cotangents in: bmu, bvar (B,M).  Cotangents out: bstate (B, SW), bt (B,M), bc (B,J), ba (B,M), bU (B,M,J). */
int c2_filter_forecast_rev(int64_t B, int64_t M, int64_t J, const double *state, const double *t, int64_t t_bs, const double *c,
                           int64_t c_bs, const double *U, const int32_t *count, const double *bmu, const double *bvar,
                           double *bstate, double *bt, double *bc, double *ba, double *bU, c2_stream_t stream);

/* Reverse of c2_filter_absorb.  state_in (B, SW): the state the forward call STARTED from; t, c, W (B,M,J), d, z (B,M),
 * count (nullable) as given to it.  Cotangent in: bstate_out (B, SW).  ws (B, M, J + J^2), c2_filter_rev_workspace_words(J)
 * doubles per row: scratch, filled and read by this call (the states are replayed from state_in with the forward call's
 * own line -- the same bits).  Cotangents out: bstate_in (B, SW), bt (B,M), bc (B,J), bW (B,M,J), bd, bz (B,M). */
int c2_filter_absorb_rev(int64_t B, int64_t M, int64_t J, const double *state_in, const double *t, int64_t t_bs, const double *c,
                         int64_t c_bs, const double *W, const double *d, const double *z, const int32_t *count,
                         const double *bstate_out, double *ws, double *bstate_in, double *bt, double *bc, double *bW, double *bd,
                         double *bz, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_FILTER_STREAM_REV_H_ */
