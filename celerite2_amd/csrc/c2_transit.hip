// c2_transit.hip -- the WHITENED TRANSIT TEMPLATES of a trial grid under the factored covariance (c2_whitened_transits,
// include/celerite2_amd_transit.h): for every series b and trial k = (period P, epoch t0, duration w, ingress tau), with d, W
// of c2_factor and Z0 = L^-1 [A0 | y - mean] (B, N, Q0) of c2_solve_lower,
//   z = L^-1 b_k(t),   <a, b> = sum_n a_n b_n / d_n,   T[b, k, :] = [<z, z>, <z, Z0[:, j]> (j < Q0)]
// in ONE forward sweep that forms the box or trapezoid b_k in registers and writes neither it nor z: what box least squares
// under correlated noise reads (celerite2_amd/transit.py).  No counterpart in the reference.
//
// The recurrence is internal::forward (internal.hpp:107-146) as restated in c2_gram.hip, with one right-hand side:
//   f <- p_n o (f + w_{n-1} z_{n-1})        (f: J, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = b_n - f^T u_n                     (:144)
// THE TEMPLATE is the header's rule, every line rounded once and none contracted into an fma (trial::Transit,
// c2_trial_columns.hpp), so a numpy restatement takes the same discrete decisions -- which side of a fold, inside or outside
// an edge -- bit for bit.  The kernel is trial::k_trial_sweep<trial::Transit, JR, QR> (c2_trial_sweep.hpp): one column, one
// lane per trial at every width; a lane keeps its five trial constants (P, 1 / P, t0, w / 2, tau).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/celerite2_amd_transit.h"
#include "c2_trial_columns.hpp"
#include "c2_trial_sweep.hpp"

using namespace c2;

extern "C" int c2_whitened_transits(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                                    const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                    const double *Z0, const double *trials, int64_t tr_bs, double *T, c2_stream_t stream) {
  return trial::launch_sweep<trial::Transit>(B, N, J, Q0, K, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T, {}, stream);
}
