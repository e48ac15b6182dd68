// c2_harmonic_trials.hip -- MANY VECTORS ON THE 2 H COLUMNS OF A MULTI-HARMONIC FREQUENCY GRID (c2_harmonic_projections,
// c2_harmonic_null_chi2; include/celerite2_amd_harmonic_trials.h): what the Monte-Carlo false-alarm probability of the
// multi-harmonic periodogram reads (celerite2_amd/harmonics.py, null_statistics).  No counterpart in the reference.
//
// Both are the walk of c2_trial_project.hpp on trial::Harmonics<H> (c2_trial_columns.hpp): H sinusoids at the frequencies
// fl(h w), NC = 2 H columns, one double per trial.  c2_harmonic_projections is k_project on that source: P (B, F, 2 H, R).
// c2_harmonic_null_chi2 is k_harmonic_null: after the walk a lane holds, for each of its 4 x NQ (frequency, draw) pairs, all
// 2 H projections of the pair -- acc[0 .. 2 H - 1][q][reg] of frequency k0 + (l >> 4) + 4 reg and draw r0 + 16 q + (l & 15) --
// so it finishes the pair's statistic without an exchange: the header's lines, r = gty - X^T v, L w = r, dchi2 = |w|^2, with
// L (the factor of the frequency's M) and X read once per frequency and v once per draw.  The call writes D (B, F, R), one
// value where the projection writes 2 H, and reads alpha once where H one-term projections read it H times.
// H is a template parameter: the accumulators are register arrays.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "../../include/celerite2_amd_harmonic_trials.h"
#include "c2_trial_columns.hpp"
#include "c2_trial_project.hpp"

namespace c2 {
namespace harmonic_trials {

constexpr int kMaxP0 = 7;   // nuisance columns (Q0 - 1 of the sweeps)

template <int H, int NQ>
__global__ __launch_bounds__(kWave) void k_harmonic_null(int64_t N, int64_t F, int64_t R, int64_t KB, int64_t RBn, int P0,
                                                         const double *__restrict__ t, int64_t t_bs,
                                                         const double *__restrict__ freq, int64_t f_bs,
                                                         const double *__restrict__ alpha, const double *__restrict__ Lm,
                                                         const double *__restrict__ Xt, const double *__restrict__ V,
                                                         double *__restrict__ D, const trial::Sinusoid::Params prm) {
  typedef trial::Harmonics<H> Column;
  constexpr int NC = 2 * H, TRI = H * (2 * H + 1);
  const int l = threadIdx.x, lo = l & 15, hi = l >> 4;
  const int64_t kb = blockIdx.x % KB, rb = (blockIdx.x / KB) % RBn, b = blockIdx.x / (KB * RBn);
  const int64_t k0 = kb * 16, r0 = rb * (16 * NQ);
  const bool live = k0 + lo < F;
  const Column lane(freq + b * f_bs + (live ? k0 + lo : 0), live, b, prm);

  bool rlive[NQ];
  int64_t rcol[NQ];
  project::d4 acc[NC][NQ];
  project::walk<Column, NQ>(N, R, r0, lo, hi, lane, t + b * t_bs, alpha + b * N * R, rlive, rcol, acc);

  // v of this lane's draws (the clamped draw of a tile beyond R: loaded, never stored); 0 beyond P0
  double v[NQ][kMaxP0];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int p = 0; p < kMaxP0; ++p) v[q][p] = p < P0 ? V[(b * P0 + p) * R + rcol[q]] : 0.0;

  // The lane's four frequencies, one row of the factor at a time.  The scheduling barrier after a row keeps the compiler from
  // raising every load of the epilogue (4 frequencies x (H (2 H + 1) + 2 H P0) doubles) above the first row's arithmetic,
  // which took the kernel past 256 registers beside the accumulators; the epilogue is a few per cent of the walk.
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t k = k0 + hi + 4 * reg;
    if (k < F) {
      const double *Lk = Lm + (b * F + k) * TRI;
      double w[NQ][NC], dchi2[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) dchi2[q] = 0.0;
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        double x[kMaxP0], Li[NC];
#pragma unroll
        for (int p = 0; p < kMaxP0; ++p) x[p] = p < P0 ? Xt[((b * F + k) * NC + i) * P0 + p] : 0.0;
#pragma unroll
        for (int j = 0; j <= i; ++j) Li[j] = Lk[i * (i + 1) / 2 + j];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          double xv = x[0] * v[q][0];
#pragma unroll
          for (int p = 1; p < kMaxP0; ++p) xv = fma(x[p], v[q][p], xv);   // (beyond P0: + 0 * 0)
          double r = acc[i][q][reg] - xv;
#pragma unroll
          for (int j = 0; j < i; ++j) r = fma(-Li[j], w[q][j], r);
          w[q][i] = r / Li[i];
          dchi2[q] = fma(w[q][i], w[q][i], dchi2[q]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      double *Dk = D + (b * F + k) * R;
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (rlive[q]) Dk[rcol[q]] = dchi2[q];
    }
  }
}

// H's draws a wavefront (C2_HARMONIC_DRAWS_H)
template <int H> struct Draws;
template <> struct Draws<1> { static constexpr int value = C2_HARMONIC_DRAWS_1; };
template <> struct Draws<2> { static constexpr int value = C2_HARMONIC_DRAWS_2; };
template <> struct Draws<3> { static constexpr int value = C2_HARMONIC_DRAWS_3; };
template <> struct Draws<4> { static constexpr int value = C2_HARMONIC_DRAWS_4; };
static_assert(C2_HARMONICS_MAX == 4, "one instantiation per H");

// f(std::integral_constant<int, H>{}) for 1 <= H <= C2_HARMONICS_MAX
template <class Fn>
int with_harmonics(int64_t H, Fn &&f) {
  switch (H) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

}  // namespace harmonic_trials
}  // namespace c2

using namespace c2;
using namespace c2::harmonic_trials;

extern "C" int c2_harmonic_projections(int64_t B, int64_t N, int64_t F, int64_t H, int64_t R, const double *t, int64_t t_bs,
                                       const double *freq, int64_t f_bs, double t_ref, const double *alpha, double *P,
                                       c2_stream_t stream) {
  const trial::KindChecks kind{H < 1, H > C2_HARMONICS_MAX, false};
  return with_harmonics(H, [&](auto h) {
    constexpr int Hc = decltype(h)::value;
    return project::launch<trial::Harmonics<Hc>, Draws<Hc>::value>(B, N, F, R, t, t_bs, freq, f_bs, alpha, P, {t_ref}, stream, kind);
  });
}

extern "C" int c2_harmonic_null_chi2(int64_t B, int64_t N, int64_t F, int64_t H, int64_t R, int64_t P0, const double *t,
                                     int64_t t_bs, const double *freq, int64_t f_bs, double t_ref, const double *alpha,
                                     const double *Lm, const double *Xt, const double *V, double *D, c2_stream_t stream) {
  const trial::KindChecks kind{H < 1 || P0 < 0, H > C2_HARMONICS_MAX || P0 > kMaxP0, !Lm || (P0 > 0 && (!Xt || !V))};
  return with_harmonics(H, [&](auto h) {
    constexpr int Hc = decltype(h)::value, NQ = Draws<Hc>::value / 16;
    static_assert(Draws<Hc>::value % 16 == 0 && NQ >= 1, "the draws of a wavefront are a multiple of 16");
    int64_t KB, RBn;
    if (const int rc = project::grid<NQ>(B, N, F, R, t, t_bs, freq, f_bs, alpha, D, kind, KB, RBn)) return rc;
    hipLaunchKernelGGL((k_harmonic_null<Hc, NQ>), dim3((unsigned)(B * KB * RBn)), dim3(kWave), 0, (hipStream_t)stream, N, F, R, KB,
                       RBn, (int)P0, t, t_bs, freq, f_bs, alpha, Lm, Xt, V, D, trial::Sinusoid::Params{t_ref});
    return launch_ok();
  });
}
