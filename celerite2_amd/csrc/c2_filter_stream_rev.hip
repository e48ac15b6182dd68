// c2_filter_stream_rev.hip -- REVERSE of c2_filter_forecast and of c2_filter_absorb (include/celerite2_amd_filter_stream_rev.h):
// with c2_filter_append_rev (c2_filter_rev.hip) every forward entry point of the streaming layer has its reverse.  No
// counterpart in the reference.
//
// FORECAST.  The forward (k_filter<kForecast>, c2_filter.hip), per query row m, each from the same unchanged state:
//   Dt = t_m - t_last ;  p = exp(-c Dt)  (p := 0 when n == 0) ;  x = p o u ;  h = S x ;  mu = x . F ;  var = a - x . h
// Its reverse, given bmu and bvar:
//   ba_m = bvar_m          xb = bmu_m F - 2 bvar_m h          bU_m = p o xb          pi = x o xb  (= p o pb)
//   bc -= Dt pi            Dtb = -sum_j c_j pi_j              bt_m = Dtb             bstate[0] -= Dtb
//   bF += bmu_m x          bS -= bvar_m x x^T
// accumulated over the taken rows in row order.  bS is the SYMMETRIC representative: lanes i and j form x_i x_j first and then
// fma(., -bvar, acc), the same two operations on the same numbers, so bS_ij == bS_ji to the bit.
//
// ABSORB.  The forward is the decay plus update line on given d, W, z:  S <- (p p^T) o S + d w w^T,  F <- p o F + w z,
// [2] += log d, [3] += z^2 / d.  Phase 1 replays the states from state_in with that line -- the same expression, so the same
// bits -- and writes the (F, S) every taken row STARTS from to ws.  Phase 2 walks back; with St = (p p^T) o S0, Ft = p o F0:
//   bd = lb / d - qb z^2 / d^2 + w^T Sb w        bz = 2 qb z / d + Fb . w        bW = z Fb + 2 d Sb w
//   pi = 2 (Sb o St) 1 + Fb o Ft                 Sb <- (p p^T) o Sb              Fb <- p o Fb
//   bc -= Dt pi        Dtb = -sum_j c_j pi_j     bt_m += Dtb                     bt_{m-1} -= Dtb
// (the last line not for the first row of an empty series; for m = 0 the -Dtb goes to word [0] of bstate_in).  This is the
// step of k_filter_rev with the reverse of the division taken out.
//
// Mapping: that of k_filter -- a group of G lanes per series, lane j owns column j (= row j) of S and of its cotangent, the
// vectors are shared through LDS, the scalar contractions are DPP butterflies.  A lane reads back from ws only what it wrote
// itself.  No atomics: two calls give identical bits.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_filter_stream_rev.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace c2 {
namespace filter_stream_rev {

constexpr int kHead = 4;   // t_last, n, sum log d, sum z^2 / d in front of F and S (celerite2_amd_filter.h)

// As in c2_filter_rev.hip: the contractions over a column run in chunks of 8 elements with the scheduler held at the chunk's
// end from G = 16 on, so that the LDS reads of a whole contraction are not issued ahead of the arithmetic on top of the two
// register columns a lane keeps.
template <int G>
__device__ __forceinline__ void chunk_end() {
  if constexpr (G > 8) __builtin_amdgcn_sched_barrier(0);
}

// Elements 0 .. J-1 of a row into a register column, zeros behind them (branches on J alone, as in c2_filter_rev.hip).
template <int G>
__device__ __forceinline__ void load_row(double (&col)[G], const double *row, int J) {
#pragma unroll
  for (int i = 0; i < G; ++i) {
    col[i] = 0.0;
    if (i < J) col[i] = row[i];
  }
}

__device__ __forceinline__ int wave_max(int top) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int x = __shfl_xor(top, o, kWave);
    top = x > top ? x : top;
  }
  return top;
}

// ---- forecast ---------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kWave) void k_forecast_rev(int64_t B, int M, int J, const double *__restrict__ sin,
                                                        const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                        int64_t c_bs, const double *__restrict__ U,
                                                        const int32_t *__restrict__ count, const double *__restrict__ bmu,
                                                        const double *__restrict__ bvar, double *__restrict__ bs,
                                                        double *__restrict__ bt, double *__restrict__ bc, double *__restrict__ ba,
                                                        double *__restrict__ bU) {
  // No contraction, as in k_filter: h has to be the forward's, and bS stays symmetric to the bit.
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double su[kWave];
  constexpr int CH = G < 8 ? G : 8;
  const Geo<G> L(B, J);
  const int j = L.j, g0 = (L.lane / G) * G;
  const bool act = L.act;
  const int64_t SW = kHead + J + (int64_t)J * J;
  const double *si = sin + L.b * SW;
  const double *tb = t + L.b * t_bs;
  const int64_t r0 = L.b * M;   // first row of this series in the (B, M) arrays
  const double cj = act ? c[L.b * c_bs + L.jj] : 0.0;   // (an idle lane reads column 0 and drops it, here and below)
  int cnt = count ? count[L.b] : M;
  cnt = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  const int top = wave_max(cnt);   // the longest series of this wavefront

  const double tl = si[0];
  const bool empty = si[1] == 0.0;
  const double f0 = si[kHead + L.jj];
  const double F = act ? f0 : 0.0;
  double Sc[G];
  load_row<G>(Sc, si + kHead + J + L.jj * J, J);   // row j of S = its column j
  double bS[G];
#pragma unroll
  for (int i = 0; i < G; ++i) bS[i] = 0.0;
  double bF = 0.0, bcj = 0.0, btl = 0.0;

  for (int m = 0; m < top; ++m) {
    if (m < cnt) {   // (uniform over the group)
      const double tm = tb[m];
      double p = empty ? 0.0 : exp_decay(cj * (tl - tm));
      p = act ? p : 0.0;
      const double ux = U[(r0 + m) * J + L.jj];
      const double bm = bmu[r0 + m], bv = bvar[r0 + m];
      const double x = act ? p * ux : 0.0;
      su[L.lane] = x;
      lds_order();
      double h = 0.0;
#pragma unroll
      for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
        for (int i = i0; i < i0 + CH; ++i) {
          const double xi = su[g0 + i];
          h = fma(Sc[i], xi, h);
          bS[i] = fma(xi * x, -bv, bS[i]);
        }
        chunk_end<G>();
      }
      const double xb = bm * F - 2.0 * (bv * h);
      const double pi = x * xb;   // = p o pb: only that product is used
      bF = fma(bm, x, bF);
      double s = cj * pi;
      s = gsum<G>(s);
      const double Db = empty ? 0.0 : -s;                  // cotangent of t_m - t_last
      bcj -= empty ? 0.0 : (tm - tl) * pi;                 // (a stale t_last of an empty state is never multiplied)
      btl -= Db;
      if (L.valid) {
        if (j == 0) { bt[r0 + m] = Db; ba[r0 + m] = bv; }
        if (act) bU[(r0 + m) * J + j] = p * xb;
      }
      lds_order();   // (the next row overwrites the vector)
    }
  }

  if (L.valid) {
    for (int m = cnt; m < M; ++m) {   // rows not taken: zeros
      if (j == 0) { bt[r0 + m] = 0.0; ba[r0 + m] = 0.0; }
      if (act) bU[(r0 + m) * J + j] = 0.0;
    }
    double *bo = bs + L.b * SW;
    if (j == 0) { bo[0] = btl; bo[1] = 0.0; bo[2] = 0.0; bo[3] = 0.0; }
    if (act) {
      bo[kHead + j] = bF;
#pragma unroll
      for (int i = 0; i < G; ++i)
        if (i < J) bo[kHead + J + j * J + i] = bS[i];
      bc[L.b * J + j] = bcj;   // (a series that took no row: zeros, as is everything above)
    }
  }
}

// ---- absorb -----------------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kWave) void k_absorb_rev(int64_t B, int M, int J, const double *__restrict__ sin,
                                                      const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                      int64_t c_bs, const double *__restrict__ W, const double *__restrict__ d,
                                                      const double *__restrict__ z, const int32_t *__restrict__ count,
                                                      const double *__restrict__ bso, double *ws, double *__restrict__ bsi,
                                                      double *__restrict__ bt, double *__restrict__ bc, double *__restrict__ bW,
                                                      double *__restrict__ bd, double *__restrict__ bz) {
  // No contraction, as in k_filter: phase 1 has to give the bits of the forward call, and phase 2 keeps Sb symmetric to the bit.
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sp[kWave], sw[kWave];
  constexpr int CH = G < 8 ? G : 8;
  const Geo<G> L(B, J);
  const int j = L.j, g0 = (L.lane / G) * G;
  const bool act = L.act, wr = L.valid && L.act;
  const int64_t SW = kHead + J + (int64_t)J * J, WS = J + (int64_t)J * J;
  const double *si = sin + L.b * SW;
  const double *bo = bso + L.b * SW;
  const double *tb = t + L.b * t_bs;
  const int64_t r0 = L.b * M;   // first row of this series in the (B, M) arrays
  double *wsb = ws + r0 * WS;
  const double cj = act ? c[L.b * c_bs + L.jj] : 0.0;   // (an idle lane reads column 0 and drops it, here and below)
  int cnt = count ? count[L.b] : M;
  cnt = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  const int top = wave_max(cnt);   // the longest series of this wavefront
  const double tl0 = si[0];
  const bool empty0 = si[1] == 0.0;

  // ---- phase 1: the state every taken row starts from -> ws -------------------------------------------------------------
  {
    double tl = tl0;
    bool empty = empty0;
    const double f0 = si[kHead + L.jj];
    double F = act ? f0 : 0.0;
    double Sc[G];
    load_row<G>(Sc, si + kHead + J + L.jj * J, J);   // row j of S = its column j
    for (int m = 0; m < top; ++m) {
      if (m < cnt) {   // (uniform over the group)
        if (wr) {
          double *o = wsb + m * WS;
          o[j] = F;
#pragma unroll
          for (int i = 0; i < G; ++i)
            if (i < J) o[J + j * J + i] = Sc[i];
        }
        if (m + 1 < cnt) {   // (the state behind the last row is not needed)
          const double tm = tb[m];
          double p = empty ? 0.0 : exp_decay(cj * (tl - tm));
          p = act ? p : 0.0;
          const double dm = d[r0 + m], zm = z[r0 + m];
          const double wx = W[(r0 + m) * J + L.jj];
          const double w = act ? wx : 0.0;
          sp[L.lane] = p; sw[L.lane] = w;
          lds_order();
#pragma unroll
          for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
            for (int i = i0; i < i0 + CH; ++i) Sc[i] = fma(sw[g0 + i] * w, dm, (sp[g0 + i] * p) * Sc[i]);
            chunk_end<G>();
          }
          F = fma(w, zm, p * F);
          tl = tm; empty = false;
          lds_order();   // (the next row overwrites the vectors)
        }
      }
    }
  }

  // ---- phase 2: the rows backwards ---------------------------------------------------------------------------------------
  const double lb = bo[2], qb = bo[3];
  double carry = bo[0];   // what bt of the row in hand has received from behind it
  const double fb0 = bo[kHead + L.jj];
  double Fb = act ? fb0 : 0.0;
  double Sb[G];
#pragma unroll
  for (int i = 0; i < G; ++i) {   // the symmetric representative: (row j + column j) / 2
    Sb[i] = 0.0;
    if (i < J) Sb[i] = 0.5 * (bo[kHead + J + L.jj * J + i] + bo[kHead + J + i * J + L.jj]);
  }
  double S0[G];
#pragma unroll
  for (int i = 0; i < G; ++i) S0[i] = 0.0;   // (the elements i >= J stay 0: a row is loaded up to J)
  double bcj = 0.0;

  for (int m = top - 1; m >= 0; --m) {
    if (m < cnt) {   // (uniform over the group)
      const double *o = wsb + m * WS;
      const double f0 = o[L.jj];
      const double F0 = act ? f0 : 0.0;
      const double *orow = o + J + L.jj * J;
#pragma unroll
      for (int i = 0; i < G; ++i)
        if (i < J) S0[i] = orow[i];
      const bool emp = m == 0 && empty0;
      const double tm = tb[m], tp = m == 0 ? tl0 : tb[m > 0 ? m - 1 : 0];
      double p = emp ? 0.0 : exp_decay(cj * (tp - tm));
      p = act ? p : 0.0;
      const double dm = d[r0 + m], zm = z[r0 + m];
      const double wx = W[(r0 + m) * J + L.jj];
      const double w = act ? wx : 0.0;
      sp[L.lane] = p; sw[L.lane] = w;
      lds_order();
      const double Ft = p * F0;
      double Sw = 0.0, pi = 0.0;
#pragma unroll
      for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
        for (int i = i0; i < i0 + CH; ++i) {
          const double pp = sp[g0 + i] * p;
          Sw = fma(Sb[i], sw[g0 + i], Sw);
          pi = fma(Sb[i], pp * S0[i], pi);
          Sb[i] = pp * Sb[i];
        }
        chunk_end<G>();
      }
      double s1 = w * Sw, s2 = Fb * w;
      gsum2<G>(s1, s2);
      const double rd = rcp_nr(dm), zr = zm * rd;
      const double db = lb * rd - qb * (zr * zr) + s1;
      const double zb = 2.0 * (qb * zr) + s2;
      const double wb = zm * Fb + 2.0 * (dm * Sw);
      pi = 2.0 * pi + Fb * Ft;   // p o pb: only that product is used, and St = (p p^T) o S0 already has both factors
      Fb = p * Fb;
      double s4 = cj * pi;
      s4 = gsum<G>(s4);
      const double Db = emp ? 0.0 : -s4;                  // cotangent of t_m - t_{m-1}
      bcj -= emp ? 0.0 : (tm - tp) * pi;                  // (a stale t_last of an empty state is never multiplied)
      if (L.valid) {
        if (j == 0) { bt[r0 + m] = carry + Db; bd[r0 + m] = db; bz[r0 + m] = zb; }
        if (act) bW[(r0 + m) * J + j] = wb;
      }
      carry = 0.0 - Db;
      lds_order();   // (the next row overwrites the vectors)
    }
  }

  if (L.valid) {
    for (int m = cnt; m < M; ++m) {   // rows not taken: zeros
      if (j == 0) { bt[r0 + m] = 0.0; bd[r0 + m] = 0.0; bz[r0 + m] = 0.0; }
      if (act) bW[(r0 + m) * J + j] = 0.0;
    }
    double *bi = bsi + L.b * SW;
    if (cnt > 0) {
      if (j == 0) { bi[0] = carry; bi[1] = bo[1]; bi[2] = lb; bi[3] = qb; }
      if (act) {
        bi[kHead + j] = Fb;
#pragma unroll
        for (int i = 0; i < G; ++i)
          if (i < J) bi[kHead + J + j * J + i] = Sb[i];
        bc[L.b * J + j] = bcj;
      }
    } else {   // nothing taken: the identity on the state
      if (j == 0) { bi[0] = bo[0]; bi[1] = bo[1]; bi[2] = bo[2]; bi[3] = bo[3]; }
      if (act) {
        bi[kHead + j] = bo[kHead + j];
        for (int i = 0; i < J; ++i) bi[kHead + J + j * J + i] = bo[kHead + J + j * J + i];
        bc[L.b * J + j] = 0.0;
      }
    }
  }
}

inline int sizes(int64_t B, int64_t M, int64_t J) {
  if (B < 1 || M < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || M > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  return C2_OK;
}

}  // namespace filter_stream_rev
}  // namespace c2

using namespace c2;
using namespace c2::filter_stream_rev;

extern "C" int c2_filter_forecast_rev(int64_t B, int64_t M, int64_t J, const double *state, const double *t, int64_t t_bs,
                                      const double *c, int64_t c_bs, const double *U, const int32_t *count, const double *bmu,
                                      const double *bvar, double *bstate, double *bt, double *bc, double *ba, double *bU,
                                      c2_stream_t stream) {
  if (const int rc = sizes(B, M, J)) return rc;
  if (!state || !t || !c || !U || !bmu || !bvar || !bstate || !bt || !bc || !ba || !bU) return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((k_forecast_rev<G>), dim3((unsigned)((B * G + kWave - 1) / kWave)), dim3(kWave), 0, s, B, (int)M, (int)J,
                       state, t, t_bs, c, c_bs, U, count, bmu, bvar, bstate, bt, bc, ba, bU);
  });
  return launch_ok();
}

extern "C" int c2_filter_absorb_rev(int64_t B, int64_t M, int64_t J, const double *state_in, const double *t, int64_t t_bs,
                                    const double *c, int64_t c_bs, const double *W, const double *d, const double *z,
                                    const int32_t *count, const double *bstate_out, double *ws, double *bstate_in, double *bt,
                                    double *bc, double *bW, double *bd, double *bz, c2_stream_t stream) {
  if (const int rc = sizes(B, M, J)) return rc;
  if (!state_in || !t || !c || !W || !d || !z || !bstate_out || !ws || !bstate_in || !bt || !bc || !bW || !bd || !bz)
    return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((k_absorb_rev<G>), dim3((unsigned)((B * G + kWave - 1) / kWave)), dim3(kWave), 0, s, B, (int)M, (int)J,
                       state_in, t, t_bs, c, c_bs, W, d, z, count, bstate_out, ws, bstate_in, bt, bc, bW, bd, bz);
  });
  return launch_ok();
}
