// c2_trial_project.hip -- THE PROJECTIONS OF MANY VECTORS ON THE COLUMNS OF A TRIAL GRID (c2_trial_projections,
// include/celerite2_amd_trials.h; c2_shape_projections, include/celerite2_amd_shapes.h): for every series b, trial k,
// column c of that trial and vector r,
//   P[b, k, c, r] = sum_n col_c(trial k; t[b, n]) * alpha[b, n, r]
// with the columns of the four searches -- (cos, sin) of the periodogram's phase, the transit template, (cos nu, sin nu) of
// a Keplerian orbit, the tabulated shape -- formed in registers by the very column sources the whitening sweep uses
// (c2_trial_columns.hpp), so the column values are its bit for bit.  With alpha = (K + D)^-1 (y_r - mean) this is gty_r of a search for R series y_r at
// once: what the Monte-Carlo false-alarm probability reads (celerite2_amd/significance.py).  It is a (K x N) . (N x R)
// matrix product whose left operand is never in memory and has no recurrence: the cost of forming a column -- for the
// Keplerian, one solve of Kepler's equation -- is paid once for all R vectors.  No counterpart in the reference.
//
// k_project<Column, NQ> and its launcher are in c2_trial_project.hpp (the multi-harmonic entry points of
// c2_harmonic_trials.hip walk the same way); this file holds the entry points of the four searches.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_shapes.h"
#include "../../include/celerite2_amd_trials.h"
#include "c2_launch.hpp"
#include "c2_trial_columns.hpp"
#include "c2_trial_project.hpp"

using namespace c2;

extern "C" int c2_trial_projections(int kind, int64_t B, int64_t N, int64_t K, int64_t R, const double *t, int64_t t_bs,
                                    const double *trials, int64_t tr_bs, double t_ref, const double *alpha, double *P,
                                    c2_stream_t stream) {
  if (kind == C2_TRIAL_SINUSOID)
    return project::launch<trial::Sinusoid, C2_TRIAL_SINUSOID_DRAWS>(B, N, K, R, t, t_bs, trials, tr_bs, alpha, P, {t_ref}, stream);
  if (kind == C2_TRIAL_TRANSIT)
    return project::launch<trial::Transit, C2_TRIAL_TRANSIT_DRAWS>(B, N, K, R, t, t_bs, trials, tr_bs, alpha, P, {}, stream);
  if (kind == C2_TRIAL_KEPLERIAN)
    return project::launch<trial::Keplerian, C2_TRIAL_KEPLERIAN_DRAWS>(B, N, K, R, t, t_bs, trials, tr_bs, alpha, P, {}, stream);
  return C2_ERR_INVALID;
}

extern "C" int c2_shape_projections(int64_t B, int64_t N, int64_t K, int64_t R, const double *t, int64_t t_bs,
                                    const double *trials, int64_t tr_bs, const double *alpha, double *P, const double *shapes,
                                    int64_t sh_bs, int64_t NS, int64_t S, c2_stream_t stream) {
  return project::launch<trial::Shape, C2_SHAPE_DRAWS>(B, N, K, R, t, t_bs, trials, tr_bs, alpha, P, {shapes, sh_bs, (int)NS, (int)S},
                                                       stream, trial::bank_checks(shapes, sh_bs, NS, S));
}
