// c2_harmonics.hip -- the WHITENED HARMONICS of a frequency grid under the factored covariance (c2_whitened_harmonics,
// include/celerite2_amd_harmonics.h): for every series b and trial frequency f, H harmonics, the NC = 2 H columns
//   a_{2h-2} = cos x_h,  a_{2h-1} = sin x_h,  x_h = fl(fl(h w_f) * fl(t - t_ref))  (h = 1 .. H),   z_i = L^-1 a_i
//   T[b, f, :] = [<z_i, z_j> (0 <= i <= j < NC, row-major over the upper triangle), <z_i, Z0[:, q]> (i < NC major, q < Q0)]
// with <a, b> = sum_n a_n b_n / d_n, in ONE forward sweep that forms the columns in registers: what the multi-harmonic
// periodogram under correlated noise reads (celerite2_amd/harmonics.py).  No counterpart in the reference.
//
// Harmonic h's columns are trial::Sinusoid's at the frequency fl(h w_f) -- the same source, the same phase rule -- and the
// rows come from trial::sweep_rows, the staging of the four searches (c2_trial_sweep.hpp).  The kernel stands BESIDE
// k_trial_sweep, whose instantiations are untouched.
//
// THE MAPPING.  A column's forward substitution needs nothing of another column; only <z_i, z_j> between columns of
// different lanes needs an exchange.  A trial takes G neighbouring lanes:
//   JR <= 16:  one HARMONIC a lane (two columns, the periodogram's own two-column row body); G = GH = 2 (H = 2) or 4 (H = 3, 4)
//   JR  = 32:  one COLUMN a lane (the periodogram's split form: even lane cos, odd lane sin);  G = 2 GH = 4 or 8
// The lanes of a group beyond H (H = 3: the fourth) and the lanes beyond F carry the inert trial (w = 0), read no frequency
// and store nothing.  The statements a lane makes for its own columns are those of k_trial_sweep's row body, in its order,
// so what T holds about one harmonic alone is what c2_whitened_sinusoids writes at fl(h w_f), bit for bit.
// THE EXCHANGE is by XOR distance D = 1 .. G - 1 inside the group: quad permutes for D < 4; D = 7 is row_half_mirror and
// D = 4, 5, 6 a quad permute of the mirrored value -- all DPP, nothing through LDS or memory.  The cross sums are shared
// out: in the one-column form the pair (i, i ^ D) is kept by the lane with the lower column; in the two-column form the
// four products of lanes g < g' are split two and two --
//   both:        own cos with the partner's sin     -> <c_g, s_g'> (lower lane),  <s_g, c_g'> (upper lane)
//   lower lane:  own cos with the partner's cos     -> <c_g, c_g'>
//   upper lane:  own sin with the partner's sin     -> <s_g, s_g'>
// so every element of T has exactly one writer: no atomics, two calls give identical bits.
// H IS A RUN-TIME, WAVE-UNIFORM COUNT over a kernel built for its group size GH (2 or 4): H = 3 and H = 4 share one kernel
// (the idle lane is there either way), which keeps the instantiations at 2 x 4 (JR) x 4 (QR) = 32, half of what a template
// parameter H = 2, 3, 4 and the sweep's 64 would suggest; H only enters the liveness of a lane and the addresses of its stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/celerite2_amd_harmonics.h"
#include "../../include/celerite2_amd_periodogram.h"
#include "c2_trial_columns.hpp"
#include "c2_trial_sweep.hpp"

using namespace c2;

namespace c2 {
namespace harmonics {

// lanes of a trial
constexpr int group_lanes(int GH, int JR) { return JR >= 32 ? 2 * GH : GH; }

// x of the lane at XOR distance D in the group; hm = the half-mirrored x (D >= 4)
template <int D>
__device__ __forceinline__ double xchg(double x, double hm) {
  static_assert(D >= 1 && D <= 7, "a distance inside 8 lanes");
  if constexpr (D == 1) return dpp_mov<kDppXor1>(x);
  if constexpr (D == 2) return dpp_mov<kDppXor2>(x);
  if constexpr (D == 3) return dpp_mov<kDppXor3>(x);
  if constexpr (D == 4) return dpp_mov<kDppXor3>(hm);
  if constexpr (D == 5) return dpp_mov<kDppXor2>(hm);
  if constexpr (D == 6) return dpp_mov<kDppXor1>(hm);
  return hm;
}

// f(std::integral_constant<int, D>{}) for D = 1 .. G - 1
template <int G, int D = 1, class Fn>
__device__ __forceinline__ void each_distance(Fn &&f) {
  if constexpr (D < G) {
    f(std::integral_constant<int, D>{});
    each_distance<G, D + 1>(f);
  }
}

// element (i, j), i <= j, of the upper triangle of an NC x NC matrix stored row-major
__device__ __forceinline__ int tri(int i, int j, int NC) { return i * NC - (i * (i - 1)) / 2 + (j - i); }

// THE KERNEL (GH: lanes a trial's harmonics are rounded to, 2 or 4; JR: J rounded up to 4, 8, 16 or 32; QR: Q0 rounded up to
// 1, 2, 4 or 8).  Blocks: B * FB in grid.x, FB = ceil(F / trials per wavefront), the blocks of a series next to each other.
template <int GH, int JR, int QR>
__global__ __launch_bounds__(kWave) void k_harmonic_sweep(int64_t N, int J, int Q0, int64_t F, int64_t FB, int H,
                                                          const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                          int64_t c_bs, const double *__restrict__ U, const double *__restrict__ W,
                                                          const double *__restrict__ d, const double *__restrict__ Z0,
                                                          const double *__restrict__ freq, int64_t f_bs, double t_ref,
                                                          double *__restrict__ T) {
  constexpr bool SPLIT = JR >= 32;                 // a lane holds one column, not a harmonic's two
  constexpr int NL = SPLIT ? 1 : 2;                // columns a lane holds
  constexpr int G = group_lanes(GH, JR);           // lanes of a trial
  // rows per staged block: 8 where a lane holds one column, as in k_trial_sweep, and at JR = 16 with eight sums per column,
  // where the state, the sums and sixteen rows' staging registers together pass 256 registers (the staging moves data only)
  constexpr int R = SPLIT || (JR == 16 && QR == 8) ? 8 : 16;
  constexpr int NX = (G - 1) * NL;                 // sums with the columns of other lanes
  const int lane = threadIdx.x, m = lane & (G - 1);
  const int64_t b = blockIdx.x / FB, k = (blockIdx.x % FB) * (kWave / G) + lane / G;
  const int g = SPLIT ? m >> 1 : m;                // this lane's harmonic, from 0
  const bool odd = SPLIT && (m & 1);
  const bool live = k < F && g < H;
  const trial::Sinusoid col(live ? pgram::harmonic(g + 1, freq[b * f_bs + k]) : 0.0, {t_ref});   // w_h = fl(h * w)

  double Fst[NL][JR], T0[NL][QR], Tsq[NL], z[NL], T01 = 0.0, X[NX];
#pragma unroll
  for (int a = 0; a < NL; ++a) {
#pragma unroll
    for (int i = 0; i < JR; ++i) Fst[a][i] = 0.0;
#pragma unroll
    for (int q = 0; q < QR; ++q) T0[a][q] = 0.0;
    Tsq[a] = z[a] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) X[i] = 0.0;

  // one row: k_trial_sweep's body at NC = 2 for this lane's own columns, then the sums with the other lanes' columns
  auto row = [&](const double *sx, const double *sp, const double *sw, const double *su, const double *sz) {
    double rhs[2];
    const double rd = sx[1];
    col.columns(sx[0], rhs);
    if (SPLIT) rhs[0] = odd ? rhs[1] : rhs[0];
    double acc[NL][4];
#pragma unroll
    for (int a = 0; a < NL; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.0;
#pragma unroll
    for (int i = 0; i < JR; ++i) {
      const double p = sp[i], w = sw[i], u = su[i];
#pragma unroll
      for (int a = 0; a < NL; ++a) {
        const double fa = p * fma(w, z[a], Fst[a][i]);   // :140, :143
        Fst[a][i] = fa;
        acc[a][i & 3] = fma(fa, u, acc[a][i & 3]);
      }
    }
    double zd[NL];
#pragma unroll
    for (int a = 0; a < NL; ++a) {
      z[a] = rhs[a] - ((acc[a][0] + acc[a][1]) + (acc[a][2] + acc[a][3]));   // :144
      zd[a] = z[a] * rd;
      Tsq[a] = fma(z[a], zd[a], Tsq[a]);
    }
    if (!SPLIT) T01 = fma(zd[0], z[1], T01);             // <c_g, s_g> inside the lane
    double hm[NL];
#pragma unroll
    for (int a = 0; a < NL; ++a) hm[a] = G >= 8 ? dpp_mov<kDppHalfMirror>(z[a]) : 0.0;
    each_distance<G>([&](auto dist) {
      constexpr int D = decltype(dist)::value;
      if constexpr (SPLIT) {
        X[D - 1] = fma(zd[0], xchg<D>(z[0], hm[0]), X[D - 1]);   // (D = 1: the periodogram's <z_0, z_1>, as it forms it)
      } else {
        const bool lower = m < (m ^ D);                          // (the highest bit of D is clear in m)
        const double pc = xchg<D>(z[0], hm[0]), ps = xchg<D>(z[NL - 1], hm[NL - 1]);
        X[2 * (D - 1)] = fma(zd[0], ps, X[2 * (D - 1)]);
        X[2 * (D - 1) + 1] = fma(lower ? zd[0] : zd[NL - 1], lower ? pc : ps, X[2 * (D - 1) + 1]);
      }
    });
#pragma unroll
    for (int q = 0; q < QR; ++q) {
      const double z0 = sz[q];
#pragma unroll
      for (int a = 0; a < NL; ++a) T0[a][q] = fma(zd[a], z0, T0[a][q]);
    }
  };
  trial::sweep_rows<JR, QR, R>(N, J, Q0, b, t, t_bs, c, c_bs, U, W, d, Z0, row);

  if (live) {
    const int NC = 2 * H, HEAD = H * (NC + 1);
    double *Tb = T + (b * F + k) * (HEAD + NC * Q0);
    const int i0 = SPLIT ? m : 2 * g;                            // this lane's first column
    Tb[tri(i0, i0, NC)] = Tsq[0];
    if (!SPLIT) {
      Tb[tri(i0, i0 + 1, NC)] = T01;
      Tb[tri(i0 + 1, i0 + 1, NC)] = Tsq[NL - 1];
    }
    each_distance<G>([&](auto dist) {
      constexpr int D = decltype(dist)::value;
      const int mp = m ^ D;                                      // the partner: a lane of this trial, live when its columns are
      if constexpr (SPLIT) {
        if (mp > m && mp < NC) Tb[tri(m, mp, NC)] = X[D - 1];
      } else if (mp < H) {
        if (mp > m) {
          Tb[tri(i0, 2 * mp + 1, NC)] = X[2 * (D - 1)];          // <c_g, s_g'>
          Tb[tri(i0, 2 * mp, NC)] = X[2 * (D - 1) + 1];          // <c_g, c_g'>
        } else {
          Tb[tri(2 * mp + 1, i0, NC)] = X[2 * (D - 1)];          // <s_g', c_g>
          Tb[tri(2 * mp + 1, i0 + 1, NC)] = X[2 * (D - 1) + 1];  // <s_g', s_g>
        }
      }
    });
#pragma unroll
    for (int q = 0; q < QR; ++q)
      if (q < Q0) {
#pragma unroll
        for (int a = 0; a < NL; ++a) Tb[HEAD + (i0 + a) * Q0 + q] = T0[a][q];
      }
  }
}

}  // namespace harmonics
}  // namespace c2

using namespace c2::harmonics;

extern "C" int c2_whitened_harmonics(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t F, int64_t H, const double *t,
                                     int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *W,
                                     const double *d, const double *Z0, const double *freq, int64_t f_bs, double t_ref,
                                     double *T, c2_stream_t stream) {
  // the stages of trial::launch_sweep: sizes, limits, pointers and strides
  if (B < 1 || N < 1 || J < 1 || Q0 < 1 || F < 1 || H < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || Q0 > trial::kMaxQ0 || H > C2_HARMONICS_MAX) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !Z0 || !freq || !T || t_bs < 0 || c_bs < 0 || f_bs < 0) return C2_ERR_INVALID;
  if (H == 1) return c2_whitened_sinusoids(B, N, J, Q0, F, t, t_bs, c, c_bs, U, W, d, Z0, freq, f_bs, t_ref, T, stream);
  const int GH = H == 2 ? 2 : 4;
  const int64_t tpw = kWave / group_lanes(GH, padded(J)), FB = (F + tpw - 1) / tpw;
  if (FB > 0x7fffffffLL || B > 0x7fffffffLL / FB) return C2_ERR_UNSUPPORTED;   // 2^31 blocks or more
  dispatch_padded(J, [&](auto jr) {
    dispatch_columns(Q0, [&](auto qr) {
      auto go = [&](auto gh) {
        hipLaunchKernelGGL((k_harmonic_sweep<decltype(gh)::value, decltype(jr)::value, decltype(qr)::value>), dim3((unsigned)(B * FB)),
                           dim3(kWave), 0, (hipStream_t)stream, N, (int)J, (int)Q0, F, FB, (int)H, t, t_bs, c, c_bs, U, W, d, Z0, freq,
                           f_bs, t_ref, T);
      };
      if (GH == 2) go(std::integral_constant<int, 2>{});
      else go(std::integral_constant<int, 4>{});
    });
  });
  return launch_ok();
}
