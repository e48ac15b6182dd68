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
// THE COLUMNS are the header's rule (columns() below): the mean anomaly reduced exactly by the double 2 pi, then a fixed
// sequence -- the starter, three of Danby's quartic steps on a fresh sine and cosine, a fourth on the pair rotated by the
// third step, the final pair rotated by the fourth -- with no loop or branch on the data, no library call and no scratch:
// four sincos_cw_fast on arguments in [0, pi + 1], thirteen rcp_nr.  tests/kepler_ref.py restates it line by line.
//
// k_keplerians<JR, QR> (JR: J rounded up to 4, 8, 16 or 32; QR: Q0 rounded up to 1, 2, 4 or 8) has k_sinusoids' two forms
// (c2_periodogram.hip, whose row body is repeated here).  Up to JR = 16: ONE LANE PER TRIAL, a wavefront takes 64
// consecutive trials of one series; a lane holds the two columns of F (2 JR registers), the 3 + 2 QR sums and its six trial
// constants (w, e, tp, sqrt(1 - e^2), sin e, cos e).  At JR = 32 a trial takes TWO neighbouring lanes, one column each (32
// trials per wavefront): both solve the same equation, the cosine lane keeps <z_c, .>, the sine lane <z_s, .>, and the one
// value a row exchanges is the partner's z for <z_c, z_s> (a DPP move inside the quad).  Both forms make the same statements
// per value, so T does not depend on which one ran.
// Everything else about a row is the same for all 64 lanes and comes staged through LDS, R = 16 rows a block (8 in the
// two-lane form), by trial::sweep_rows (c2_trial_sweep.hpp).  Lanes with k >= K carry the harmless trial w = 0, e = 0 and
// store nothing.  Every element of T is written by exactly one lane: no atomics, two calls give identical bits.  Blocks:
// B * ceil(K / trials per wavefront) in grid.x, the trial blocks of a series next to each other.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_kepler.h"
#include "c2_launch.hpp"
#include "c2_trial_columns.hpp"
#include "c2_trial_sweep.hpp"

namespace c2 {
namespace kepler {

constexpr int trials_per_wave(int JR) { return JR >= 32 ? kWave / 2 : kWave; }

template <int JR, int QR>
__global__ __launch_bounds__(kWave) void k_keplerians(int64_t N, int J, int Q0, int64_t K, int64_t KB,
                                                      const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                      int64_t c_bs, const double *__restrict__ U, const double *__restrict__ W,
                                                      const double *__restrict__ d, const double *__restrict__ Z0,
                                                      const double *__restrict__ trials, int64_t tr_bs, double *__restrict__ T) {
  constexpr bool SPLIT = trials_per_wave(JR) < kWave;       // a lane holds one column (cos: even lane, sin: odd), not both
  constexpr int NC = SPLIT ? 1 : 2;
  constexpr int R = SPLIT ? 8 : 16;                         // rows per staged block
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / KB, k = (blockIdx.x % KB) * trials_per_wave(JR) + (SPLIT ? lane >> 1 : lane);
  const bool sine = SPLIT && (lane & 1);
  const double *tp = trials + b * tr_bs + (k < K ? k : 0) * 3;
  const Trial tr = make_trial(k < K ? tp[0] : 0.0, k < K ? tp[1] : 0.0, k < K ? tp[2] : 0.0);

  // column 0: the cosine's (SPLIT: this lane's own), column 1: the sine's
  double Fst[NC][JR], T0[NC][QR], Tsq[NC], z[NC], Tcs = 0.0;
#pragma unroll
  for (int a = 0; a < NC; ++a) {
#pragma unroll
    for (int i = 0; i < JR; ++i) Fst[a][i] = 0.0;
#pragma unroll
    for (int q = 0; q < QR; ++q) T0[a][q] = 0.0;
    Tsq[a] = z[a] = 0.0;
  }

  // one row: sx = (t_n, 1 / d_n) and the staged LDS rows p_n, w_{n-1}, u_n, Z0[n]
  auto row = [&](const double *sx, const double *sp, const double *sw, const double *su, const double *sz) {
    double rhs[2];
    columns(tr, sx[0], rhs[0], rhs[1]);
    const double rd = sx[1];
    if (SPLIT) rhs[0] = sine ? rhs[1] : rhs[0];
    double acc[NC][4];
#pragma unroll
    for (int a = 0; a < NC; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.0;
#pragma unroll
    for (int i = 0; i < JR; ++i) {
      const double p = sp[i], w = sw[i], u = su[i];
#pragma unroll
      for (int a = 0; a < NC; ++a) {
        const double fa = p * fma(w, z[a], Fst[a][i]);   // :140, :143
        Fst[a][i] = fa;
        acc[a][i & 3] = fma(fa, u, acc[a][i & 3]);
      }
    }
    double zd[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      z[a] = rhs[a] - ((acc[a][0] + acc[a][1]) + (acc[a][2] + acc[a][3]));   // :144
      zd[a] = z[a] * rd;
      Tsq[a] = fma(z[a], zd[a], Tsq[a]);
    }
    // <z_c, z_s> as (z_c / d) z_s: the sine's z is the partner lane's when a lane holds one column (kept by the cosine lane)
    Tcs = fma(zd[0], SPLIT ? dpp_mov<kDppXor1>(z[0]) : z[NC - 1], Tcs);
#pragma unroll
    for (int q = 0; q < QR; ++q) {
      const double z0 = sz[q];
#pragma unroll
      for (int a = 0; a < NC; ++a) T0[a][q] = fma(zd[a], z0, T0[a][q]);
    }
  };
  trial::sweep_rows<JR, QR, R>(N, J, Q0, b, t, t_bs, c, c_bs, U, W, d, Z0, row);

  if (k < K) {
    double *Tb = T + (b * K + k) * (3 + 2 * Q0);
    if (!sine) { Tb[0] = Tsq[0]; Tb[1] = Tcs; }
    if (!SPLIT || sine) Tb[2] = Tsq[NC - 1];
#pragma unroll
    for (int q = 0; q < QR; ++q)
      if (q < Q0) {
        if (!sine) Tb[3 + q] = T0[0][q];
        if (!SPLIT || sine) Tb[3 + Q0 + q] = T0[NC - 1][q];
      }
  }
}

}  // namespace kepler
}  // namespace c2

using namespace c2;
using namespace c2::kepler;

extern "C" int c2_whitened_keplerians(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                                      const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                      const double *Z0, const double *trials, int64_t tr_bs, double *T, c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1 || Q0 < 1 || K < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || Q0 > trial::kMaxQ0) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !Z0 || !trials || !T) return C2_ERR_INVALID;
  if (t_bs < 0 || c_bs < 0 || tr_bs < 0) return C2_ERR_INVALID;
  const int64_t tpw = trials_per_wave(padded(J)), KB = (K + tpw - 1) / tpw;
  if (KB > 0x7fffffffLL || B > 0x7fffffffLL / KB) return C2_ERR_UNSUPPORTED;   // 2^31 blocks or more
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * KB));
  dispatch_padded(J, [&](auto jr) {
    dispatch_columns(Q0, [&](auto qr) {
      hipLaunchKernelGGL((k_keplerians<decltype(jr)::value, decltype(qr)::value>), grid, dim3(kWave), 0, s, N, (int)J, (int)Q0,
                         K, KB, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T);
    });
  });
  return launch_ok();
}
