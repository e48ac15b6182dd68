// c2_filter_rev.hip -- REVERSE of c2_filter_append (include/celerite2_amd_filter_rev.h): the cotangents of the rows of one
// call and of the state it started from, out of the cotangents of what it returned and of the state it left.  No counterpart
// in the reference, whose reverse of factor and solve_lower (reverse.hpp:10-85, 129-170) always runs over whole series.
//
// Phase 1 replays the states from state_in with the absorb line of k_filter (c2_filter.hip) on the W, d, z the forward call
// returned -- no division, the same expression, so the same bits -- and writes the (F, S) every taken row STARTS from,
// unpropagated, to ws.  Phase 2 walks the rows backwards.  With S0, F0 a row's entry state, p its decay (0 for the first row
// of an empty series), St = (p p^T) o S0, Ft = p o F0, g = St u, and lb, qb the cotangents of words [2], [3] of the state:
//   db = bd + lb / d - qb z^2 / d^2 + w^T Sb w        zb = bz + 2 qb z / d + Fb . w
//   wb = bW + z Fb + 2 d Sb w
//   by = zb        ub = -zb Ft        Ftb = Fb - zb u
//   bV = wb / d    gb = -wb / d       db -= (wb . w) / d
//   ba = db        ub -= db g         gb -= db u
//   Stb = Sb + (gb u^T + u gb^T) / 2                  bU = ub + St gb
//   pb = 2 (Stb o S0) p + Ftb o F0                    (formed as p o pb = 2 (Stb o St) 1 + Ftb o Ft: no S0 beside St)
//   Sb <- (p p^T) o Stb      Fb <- p o Ftb
//   bc -= Dt (p o pb)        Dtb = -sum_j c_j p_j pb_j        bt_m += Dtb     bt_{m-1} -= Dtb       (Dt = t_m - t_{m-1})
// (the last line not for the first row of an empty series; for m = 0 the -Dtb goes to word [0] of bstate_in).  Sb is the
// SYMMETRIC representative of the cotangent of S -- exact, since S is symmetric for all parameter values -- and every line
// above keeps it symmetric: the two products of (gb_i u_j + u_i gb_j) are the same two numbers in lanes i and j.
//
// Mapping: that of k_filter -- a group of G lanes per series, lane j owns column j (= row j) of S0 and of Sb, the vectors
// p, u, w, gb are shared through LDS, the four scalar contractions are DPP butterflies.  A lane reads back from ws only what
// it wrote itself (its F_j and its row of S), so nothing is exchanged between lanes through memory.  No atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_filter_rev.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace c2 {
namespace filter_rev {

constexpr int kHead = 4;   // t_last, n, sum log d, sum z^2 / d in front of F and S (celerite2_amd_filter.h)

// The contractions over a column run in chunks of 8 elements with the scheduler held at the chunk's end from G = 16 on: left
// to itself it issues the LDS reads of a whole contraction ahead of the arithmetic, 6 G registers on top of the 4 G of the two
// columns and the row's pointers, and G = 32 spills six registers (profiles/filter_rev.md has the table with the barrier).
template <int G>
__device__ __forceinline__ void chunk_end() {
  if constexpr (G > 8) __builtin_amdgcn_sched_barrier(0);
}

// Elements 0 .. J-1 of a row into a register column, zeros behind them.  The branches are on J alone (scalar): a select on
// a clamped index instead costs one 64-bit address per element, which the compiler keeps across the row loop.  An idle lane
// (j >= J) loads row 0 like lane 0: what it computes from it is finite and never leaves the lane -- its p, u, w, gb are 0.
template <int G>
__device__ __forceinline__ void load_row(double (&col)[G], const double *row, int J) {
#pragma unroll
  for (int i = 0; i < G; ++i) {
    col[i] = 0.0;
    if (i < J) col[i] = row[i];
  }
}

template <int G>
__global__ __launch_bounds__(kWave) void k_filter_rev(int64_t B, int M, int J, const double *__restrict__ sin,
                                                      const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                      int64_t c_bs, const double *__restrict__ U, const double *__restrict__ W,
                                                      const double *__restrict__ d, const double *__restrict__ z,
                                                      const int32_t *__restrict__ count, const int32_t *__restrict__ flag,
                                                      const double *__restrict__ bso, const double *__restrict__ bd,
                                                      const double *__restrict__ bW, const double *__restrict__ bz, double *ws,
                                                      double *__restrict__ bsi, double *__restrict__ bt, double *__restrict__ bc,
                                                      double *__restrict__ ba, double *__restrict__ bU, double *__restrict__ bV,
                                                      double *__restrict__ by) {
  // No contraction, as in k_filter: phase 1 has to give the bits of the forward call, and phase 2 keeps Sb symmetric to the bit.
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sp[kWave], su[kWave], sw[kWave], sg[kWave];
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
  if (flag[L.b] != 0) cnt = 0;   // a failed call passed its series through: so does this one
  int top = cnt;                 // the longest series of this wavefront
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int x = __shfl_xor(top, o, kWave);
    top = x > top ? x : top;
  }
  const double tl0 = si[0];
  const bool empty0 = si[1] == 0.0;

  // ---- phase 1: the state every taken row starts from -> ws -------------------------------------------------------------
  {
    double tl = tl0;
    bool empty = empty0;
    const double f0 = si[kHead + L.jj];
    double F = act ? f0 : 0.0;
    const double *srow = si + kHead + J + L.jj * J;   // row j of S = its column j
    double Sc[G];
    load_row<G>(Sc, srow, J);
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
      const double ux = U[(r0 + m) * J + L.jj], wx = W[(r0 + m) * J + L.jj];
      const double u = act ? ux : 0.0, w = act ? wx : 0.0;
      const double bdm = bd ? bd[r0 + m] : 0.0, bzm = bz ? bz[r0 + m] : 0.0;
      const double bwx = bW ? bW[(r0 + m) * J + L.jj] : 0.0;
      const double bWm = act ? bwx : 0.0;
      sp[L.lane] = p; su[L.lane] = u; sw[L.lane] = w;
      lds_order();
      const double Ft = p * F0;
      double g = 0.0, Sw = 0.0;
#pragma unroll
      for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
        for (int i = i0; i < i0 + CH; ++i) {
          S0[i] = (sp[g0 + i] * p) * S0[i];   // St from here on
          g = fma(S0[i], su[g0 + i], g);
          Sw = fma(Sb[i], sw[g0 + i], Sw);
        }
        chunk_end<G>();
      }
      double s1 = w * Sw, s2 = Fb * w;
      gsum2<G>(s1, s2);
      const double rd = rcp_nr(dm), zr = zm * rd;
      double db = bdm + lb * rd - qb * (zr * zr) + s1;
      const double zb = bzm + 2.0 * (qb * zr) + s2;
      const double wb = bWm + zm * Fb + 2.0 * (dm * Sw);
      double ub = -(zb * Ft);
      const double Ftb = Fb - zb * u;
      const double bv = wb * rd;
      double s3 = wb * w;
      s3 = gsum<G>(s3);
      db -= s3 * rd;
      ub -= db * g;
      const double gb = -bv - db * u;
      sg[L.lane] = act ? gb : 0.0;
      lds_order();
      double acc = 0.0, pb = 0.0;
#pragma unroll
      for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
        for (int i = i0; i < i0 + CH; ++i) {
          acc = fma(S0[i], sg[g0 + i], acc);
          const double Stb = Sb[i] + 0.5 * (sg[g0 + i] * u + su[g0 + i] * gb);
          pb = fma(Stb, S0[i], pb);
          Sb[i] = (sp[g0 + i] * p) * Stb;
        }
        chunk_end<G>();
      }
      pb = 2.0 * pb + Ftb * Ft;   // p o pb: only that product is used, and St = (p p^T) o S0 already has both factors
      Fb = p * Ftb;
      double s4 = cj * pb;
      s4 = gsum<G>(s4);
      const double Db = emp ? 0.0 : -s4;                  // cotangent of t_m - t_{m-1}
      bcj -= emp ? 0.0 : (tm - tp) * pb;                  // (a stale t_last of an empty state is never multiplied)
      if (L.valid) {
        if (j == 0) { bt[r0 + m] = carry + Db; ba[r0 + m] = db; by[r0 + m] = zb; }
        if (act) { bU[(r0 + m) * J + j] = ub + acc; bV[(r0 + m) * J + j] = bv; }
      }
      carry = 0.0 - Db;
      lds_order();   // (the next row overwrites the vectors)
    }
  }

  if (L.valid) {
    for (int m = cnt; m < M; ++m) {   // rows not taken: zeros
      if (j == 0) { bt[r0 + m] = 0.0; ba[r0 + m] = 0.0; by[r0 + m] = 0.0; }
      if (act) { bU[(r0 + m) * J + j] = 0.0; bV[(r0 + m) * J + j] = 0.0; }
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
    } else {   // nothing taken, or the forward call failed: the identity on the state
      if (j == 0) { bi[0] = bo[0]; bi[1] = bo[1]; bi[2] = bo[2]; bi[3] = bo[3]; }
      if (act) {
        bi[kHead + j] = bo[kHead + j];
        for (int i = 0; i < J; ++i) bi[kHead + J + j * J + i] = bo[kHead + J + j * J + i];
        bc[L.b * J + j] = 0.0;
      }
    }
  }
}

}  // namespace filter_rev
}  // namespace c2

using namespace c2;
using namespace c2::filter_rev;

extern "C" int64_t c2_filter_rev_workspace_words(int64_t J) { return J < 1 || J > C2_FAST_WIDTH ? 0 : J + J * J; }

extern "C" int c2_filter_append_rev(int64_t B, int64_t M, int64_t J, const double *state_in, const double *t, int64_t t_bs,
                                    const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                    const double *z, const int32_t *count, const int32_t *flag, const double *bstate_out,
                                    const double *bd, const double *bW, const double *bz, double *ws, double *bstate_in, double *bt,
                                    double *bc, double *ba, double *bU, double *bV, double *by, c2_stream_t stream) {
  if (B < 1 || M < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || M > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  if (!state_in || !t || !c || !U || !W || !d || !z || !flag || !bstate_out || !ws || !bstate_in || !bt || !bc || !ba || !bU ||
      !bV || !by)
    return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((k_filter_rev<G>), dim3((unsigned)((B * G + kWave - 1) / kWave)), dim3(kWave), 0, s, B, (int)M, (int)J,
                       state_in, t, t_bs, c, c_bs, U, W, d, z, count, flag, bstate_out, bd, bW, bz, ws, bstate_in, bt, bc, ba, bU,
                       bV, by);
  });
  return launch_ok();
}
