// c2_shapes.hip -- the WHITENED TABULATED SHAPES of a trial grid under the factored covariance (c2_whitened_shapes,
// include/celerite2_amd_shapes.h): for every series b and trial k = (period P, epoch t0, width w, shape index s), with d, W
// of c2_factor, Z0 = L^-1 [A0 | y - mean] (B, N, Q0) of c2_solve_lower and a bank of NS event profiles tabulated on S nodes,
//   z = L^-1 b_k(t),   <a, b> = sum_n a_n b_n / d_n,   T[b, k, :] = [<z, z>, <z, Z0[:, j]> (j < Q0)]
// in ONE forward sweep that forms b_k in registers -- the profile interpolated linearly between its two nodes around the
// sample -- and writes neither it nor z: what least squares with a limb-darkened transit, a flare or a measured template
// under correlated noise reads (celerite2_amd/shapes.py).  No counterpart in the reference.
//
// The recurrence is internal::forward (internal.hpp:107-146) as restated in c2_gram.hip, with one right-hand side:
//   f <- p_n o (f + w_{n-1} z_{n-1})        (f: J, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = b_n - f^T u_n                     (:144)
// THE COLUMN is the header's rule, every line rounded once and none contracted into an fma (trial::Shape,
// c2_trial_columns.hpp), so a numpy restatement takes the same discrete decisions bit for bit.  The kernel is
// trial::k_trial_sweep<trial::Shape, JR, QR> (c2_trial_sweep.hpp): one column, one lane per trial at every width.  The bank is
// not staged: a lane in an event gathers its two nodes, adjacent doubles, through the vector cache (trial::Shape says why).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/celerite2_amd_shapes.h"
#include "c2_trial_columns.hpp"
#include "c2_trial_sweep.hpp"

using namespace c2;

extern "C" int c2_whitened_shapes(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                                  const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                  const double *Z0, const double *trials, int64_t tr_bs, double *T, const double *shapes,
                                  int64_t sh_bs, int64_t NS, int64_t S, c2_stream_t stream) {
  return trial::launch_sweep<trial::Shape>(B, N, J, Q0, K, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T,
                                           {shapes, sh_bs, (int)NS, (int)S}, stream, trial::bank_checks(shapes, sh_bs, NS, S));
}
