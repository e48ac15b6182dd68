// c2_kepler.hip -- the WHITENED KEPLERIAN COLUMNS of a trial grid under the factored covariance (c2_whitened_keplerians,
// include/celerite2_amd_kepler.h): for every series b and trial k = (angular frequency w, eccentricity e, time of periastron
// tp), with d, W of c2_factor, Z0 = L^-1 [A0 | y - mean] (B, N, Q0) of c2_solve_lower and nu(t) the true anomaly of the orbit,
//   z_c = L^-1 cos nu,   z_s = L^-1 sin nu,   <a, b> = sum_n a_n b_n / d_n
//   T[b, k, :] = [<z_c, z_c>, <z_c, z_s>, <z_s, z_s>, <z_c, Z0[:, j]> (j < Q0), <z_s, Z0[:, j]> (j < Q0)]
// in ONE forward sweep that solves Kepler's equation per row and lane in registers and writes neither the columns nor
// z_c, z_s: what the Keplerian periodogram under correlated noise reads (celerite2_amd/kepler.py).  The layout of T is
// c2_whitened_sinusoids', so periodogram.finish applies unchanged.  No counterpart in the reference.
//
// The recurrence is internal::forward (internal.hpp:107-146) as restated in c2_gram.hip, with two right-hand sides:
//   F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x 2, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = a_n - F^T u_n                     (:144),   a_n = (cos nu_n, sin nu_n)
// THE COLUMNS are the header's rule (kepler::columns, c2_trial_columns.hpp): the mean anomaly reduced exactly by the double 2 pi, then a fixed
// sequence -- the starter, three of Danby's quartic steps on a fresh sine and cosine, a fourth on the pair rotated by the
// third step, the final pair rotated by the fourth -- with no loop or branch on the data, no library call and no scratch:
// four sincos_cw_fast on arguments in [0, pi + 1], thirteen rcp_nr.  tests/kepler_ref.py restates it line by line.
//
// The kernel is trial::k_trial_sweep<trial::Keplerian, JR, QR> (c2_trial_sweep.hpp): two columns, so a trial takes two
// neighbouring lanes at J > 16, both solving the same equation; a lane keeps its six trial constants (w, e, tp,
// sqrt(1 - e^2), sin e, cos e).  Lanes beyond K carry the harmless trial w = 0, e = 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/celerite2_amd_kepler.h"
#include "c2_trial_columns.hpp"
#include "c2_trial_sweep.hpp"

using namespace c2;

extern "C" int c2_whitened_keplerians(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                                      const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                      const double *Z0, const double *trials, int64_t tr_bs, double *T, c2_stream_t stream) {
  return trial::launch_sweep<trial::Keplerian>(B, N, J, Q0, K, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T, {}, stream);
}
