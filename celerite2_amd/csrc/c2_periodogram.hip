// c2_periodogram.hip -- the WHITENED SINUSOIDS of a frequency grid under the factored covariance (c2_whitened_sinusoids,
// include/celerite2_amd_periodogram.h): for every series b and trial frequency f, with d, W of c2_factor and
// Z0 = L^-1 [A0 | y - mean] (B, N, Q0) of c2_solve_lower,
//   z_c = L^-1 cos(w_f (t - t_ref)),   z_s = L^-1 sin(w_f (t - t_ref)),   <a, b> = sum_n a_n b_n / d_n
//   T[b, f, :] = [<z_c, z_c>, <z_c, z_s>, <z_s, z_s>, <z_c, Z0[:, k]> (k < Q0), <z_s, Z0[:, k]> (k < Q0)]
// in ONE forward sweep that forms the two columns in registers and writes neither them nor z_c, z_s: what the generalized
// Lomb-Scargle periodogram under correlated noise reads (celerite2_amd/periodogram.py).  No counterpart in the reference.
//
// The recurrence is internal::forward (internal.hpp:107-146) as restated in c2_gram.hip, with two right-hand sides:
//   F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x 2, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = a_n - F^T u_n                     (:144),   a_n = (cos x, sin x),   x = fl(w_f * fl(t_n - t_ref))
// The phase is two roundings, the difference and then the product, neither contracted into a later fma: numpy forms it the
// same way, so a restatement has the argument bit for bit.  sincos_cw takes its fast path below kSincosFastMax.
//
// The kernel is trial::k_trial_sweep<trial::Sinusoid, JR, QR> (c2_trial_sweep.hpp), the column source trial::Sinusoid
// (c2_trial_columns.hpp): two columns, so a frequency takes two neighbouring lanes at J > 16.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/celerite2_amd_periodogram.h"
#include "c2_trial_columns.hpp"
#include "c2_trial_sweep.hpp"

using namespace c2;

extern "C" int c2_whitened_sinusoids(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t F, const double *t, int64_t t_bs,
                                     const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                     const double *Z0, const double *freq, int64_t f_bs, double t_ref, double *T,
                                     c2_stream_t stream) {
  return trial::launch_sweep<trial::Sinusoid>(B, N, J, Q0, F, t, t_bs, c, c_bs, U, W, d, Z0, freq, f_bs, T, {t_ref}, stream);
}
