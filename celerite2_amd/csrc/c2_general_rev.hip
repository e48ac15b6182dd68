// c2_general_rev.hip -- the REVERSE of general_matmul_lower / general_matmul_upper (c2_general_matmul_lower_rev / _upper_rev,
// include/celerite2_amd.h): the cotangent bZ (N, nrhs) of the product carried back to t1, t2, c, U, V and Y, so that a
// conditional mean at new times is differentiable end to end.  No counterpart in the reference (backprop.cpp exports
// general_matmul_*_fwd with the workspace F and no _rev); parity is pinned by dense algebra.
//
// Walk coordinates (c2_general_tile.hip): position s = 0 .. M-1 along t2, q = 0 .. N-1 along t1; walk time tau = t and
// array row = position for the lower variant, tau = -t and array row = M-1-s / N-1-q for the upper one.  Row s FEEDS
// output q iff tau2[s] <= tau1[q] (lower) / tau2[s] < tau1[q] (upper) -- the comparisons of the forward merge
// (forward.hpp:318-322, 378-382); s(q) is the last position that feeds q.  Forward:
//     F_0 = V_0^T Y_0 ;  F_s = p_s o F_{s-1} + V_s^T Y_s ,  p_s = exp(-c (tau2[s] - tau2[s-1]))
//     Z_q += (U_q o e_q) F_{s(q)} ,  e_q = exp(-c (tau1[q] - tau2[s(q)]))          (nothing if no row feeds q)
// Reverse, G = 0 (J x nrhs), the events walked backwards from S-1, the last position that feeds the last output:
//     output q (every q with s(q) = s, before s is un-absorbed):
//         h_j = sum_k F_s[j,k] bZ_q[k] ;  bU_q[j] = e_q[j] h_j ;  bc_j -= (tau1[q] - tau2[s]) U_q[j] bU_q[j]
//         G[j,:] += U_q[j] e_q[j] bZ_q[:]
//     row s:
//         bV_s[j] = sum_k G[j,k] Y_s[k] ;  bY_s[k] = sum_j V_s[j] G[j,k]
//         s >= 1:  bc_j -= (tau2[s] - tau2[s-1]) sum_k G[j,k] (F_s[j,k] - V_s[j] Y_s[k]) ;  G <- p_s o G
//     bt1_q = -+ sum_j c_j U_q[j] bU_q[j] ;  bt2_s = +- sum_j c_j V_s[j] bV_s[j]           (upper sign: lower variant)
// bc is accumulated event by event from these non-negative lags: the closed form over t1 U bU and t2 V bV is the same
// number and cancels (times offset by 2.45e6: 2.7e3 of the suite's criterion against 1e-3).  F is READ, never re-derived:
// (F_s - V_s^T Y_s) / p_s is the inverse of a contraction.  Only rows the forward absorbed are read (positions 1 .. S-1);
// position 0 is formed from V_0, Y_0, which is what the lower variant stored there and what the upper variant, which never
// writes its start row, did not.  Outputs no row feeds and t2 rows behind the last output get exact zeros.
//
// Mapping: k_general_rev<G, LOWER>, a group of G lanes per series (J <= G <= 32, B in grid.x), lane j owning row j of G and
// of the current F row, ONE right-hand side per launch: h, bU, bV and the bc terms are lane-local, bY_s is one DPP
// butterfly, bt1 / bt2 a second one interleaved with it.  The merge is walked one event per iteration with both kinds
// predicated, rows of both streams (time, y_s | bZ_q, V_s | U_q, and F_s beside V_s) arriving through the request-ahead
// ring of c2_merge_ring.hpp.  Several right-hand sides are launches on the same stream, column after column, each adding
// to the bU, bV, bt1, bt2, bc the one before it wrote and writing its own column of bY -- a fixed order and no atomics,
// so two calls give identical bits.  No allocation, no host read: capturable.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"
#include "c2_merge_ring.hpp"

namespace c2 {
namespace general_rev {

// Streams are indexed along the BACKWARD walk: data index m <-> position S-1-m of t2, output index n <-> position N-1-n
// of t1.  k: the right-hand side of this launch; acc != 0: add to what the launches for the columns in front of k wrote.
template <int G, bool LOWER>
__global__ __launch_bounds__(kWave) void k_general_rev(int64_t B, int N, int M, int J, int64_t nrhs, int64_t k, int acc,
                                                       const double *__restrict__ t1, int64_t t1_bs,
                                                       const double *__restrict__ t2, int64_t t2_bs,
                                                       const double *__restrict__ c, int64_t c_bs,
                                                       const double *__restrict__ U, const double *__restrict__ V,
                                                       const double *__restrict__ Y, const double *__restrict__ F,
                                                       const double *__restrict__ bZ, double *bt1, double *bt2, double *bc,
                                                       double *bU, double *bV, double *bY) {
  constexpr int SPW = kWave / G, RD = kRing, PD = kPend, NS = kSlots;
  using Lay = RingLayout<G, 2, 0, 0>;   // scalars: walk time and y_s | bZ_q; row A: V_s | U_q; row B: F_s (data slots)
  constexpr int RS = Lay::kStride;
  __shared__ __attribute__((aligned(16))) double ring[SPW * RS];
  const Geo<G> L(B, J);
  const int j = L.j, grp = L.lane / G;
  const bool act = L.act;
  const double *t1b = t1 + L.b * t1_bs, *t2b = t2 + L.b * t2_bs;
  const double *Ub = U + L.b * N * J + L.jj, *Vb = V + L.b * M * J + L.jj;
  const double *Yb = Y + L.b * M * nrhs + k, *bZb = bZ + L.b * N * nrhs + k;
  const double *Fb = F + (L.b * M * J + L.jj) * nrhs + k;
  double *bt1b = bt1 + L.b * N, *bt2b = bt2 + L.b * M;
  double *bUb = bU + L.b * N * J + L.jj, *bVb = bV + L.b * M * J + L.jj, *bYb = bY + L.b * M * nrhs + k;
  const double cj = act ? c[L.b * c_bs + j] : 0.0;
  const int64_t JK = (int64_t)J * nrhs;

  // S: how many positions of t2 feed the last output -- the rows the forward absorbed (the predicate is monotone)
  int S;
  {
    const double tq = t1b[LOWER ? N - 1 : 0];
    int lo = 0, hi = M;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double tm = t2b[LOWER ? mid : M - 1 - mid];
      if (LOWER ? tm <= tq : tm > tq) lo = mid + 1; else hi = mid;
    }
    S = lo;
  }
  auto arrM = [&](int m) { return LOWER ? S - 1 - m : M - S + m; };   // array row of data index m
  auto arrN = [&](int n) { return LOWER ? N - 1 - n : n; };           // array row of output index n

  // the rows the forward never absorbed: zeros (bV and bt2 once, by the launch of the first column)
  if (L.valid) {
    for (int p = S + j; p < M; p += G) {
      const int row = LOWER ? p : M - 1 - p;
      bYb[(int64_t)row * nrhs] = 0.0;
      if (!acc) {
        bt2b[row] = 0.0;
        for (int i = 0; i < J; ++i) bV[(L.b * M + row) * J + i] = 0.0;
      }
    }
  }

  double *rgT = ring + grp * RS, *rgX = rgT + Lay::kScal, *rgA = rgX + Lay::kScal, *rgB = rgA + NS * G;
  // the first RD indices of both streams (clamped at the end of a grid); the spare slot holds zeros
  rgT[2 * RD] = 0.0; rgX[2 * RD] = 0.0; rgA[2 * RD * G + j] = 0.0; rgB[2 * RD * G + j] = 0.0;
  for (int q = 0; q < RD; ++q) {
    double tm = 0.0, xm = 0.0, am = 0.0, fm = 0.0;
    if (S > 0) {
      const int mm = q < S ? q : S - 1, row = arrM(mm);
      tm = LOWER ? t2b[row] : -t2b[row];
      xm = Yb[(int64_t)row * nrhs];
      const double v = Vb[(int64_t)row * J], f = Fb[(int64_t)row * JK];
      am = act ? v : 0.0;
      fm = mm == S - 1 ? am * xm : (act ? f : 0.0);   // (position 0: V_0^T Y_0)
    }
    const int rn = arrN(q < N ? q : N - 1);
    const double u = Ub[(int64_t)rn * J];
    rgT[q] = tm; rgX[q] = xm; rgA[q * G + j] = am; rgB[q * G + j] = fm;
    rgT[RD + q] = LOWER ? t1b[rn] : -t1b[rn]; rgX[RD + q] = bZb[(int64_t)rn * nrhs];
    rgA[(RD + q) * G + j] = act ? u : 0.0; rgB[(RD + q) * G + j] = 0.0;
  }
  lds_order();

  struct Pend { double t, x, a, f; int slot; };
  Pend pend[PD];
#pragma unroll
  for (int i = 0; i < PD; ++i) pend[i] = Pend{0.0, 0.0, 0.0, 0.0, 2 * RD};

  int n = 0, m = 0;       // indices of the next output and of the row that is un-absorbed next (the current state's row)
  double Gs = 0.0;        // G[j, k]
  double bcj = 0.0;
  const int total = N + M;   // (the launcher refuses N + M >= 2^31)

  for (int it = 0; it < total; it += PD) {
    if (!__any(n < N || m < S)) break;
#pragma unroll
    for (int i = 0; i < PD; ++i) {
      // the row requested PD events ago arrives (never a slot this event reads: it was left PD events ago)
      {
        const Pend &pk = pend[i];
        rgT[pk.slot] = pk.t; rgX[pk.slot] = pk.x; rgA[pk.slot * G + j] = pk.a; rgB[pk.slot * G + j] = pk.f;
      }
      const int sd = m & (RD - 1), sq = RD + (n & (RD - 1));
      const double tm = rgT[sd], tq = rgT[sq], tm1 = rgT[(m + 1) & (RD - 1)];
      const bool hasm = m < S, hasn = n < N;
      // an output goes first while the current row feeds it (the forward's comparisons); with no row left it gets zeros
      const bool isout = hasn && (!hasm || (LOWER ? tm <= tq : tm < tq));
      const bool isrow = !isout && hasm;
      const int so = isout ? sq : (isrow ? sd : 2 * RD);
      {   // the request of this event: the row RD indices down the moving stream (clamped at the end of its grid)
        const int pos = isrow ? m : n, len1 = (isrow ? S : N) - 1;
        const int sreq = pos + RD < len1 ? pos + RD : len1;
        const int rreq = isrow ? arrM(sreq) : arrN(sreq);
        const double *pt = (isrow ? t2b : t1b) + rreq;
        const double *px = (isrow ? Yb : bZb) + (int64_t)rreq * nrhs;
        const double *pa = (isrow ? Vb : Ub) + (int64_t)rreq * J;
        const double rt = *pt, rx = *px, rav = *pa;   // (an idle lane reads column 0 and drops it)
        double rf = 0.0;
        if (isrow) rf = Fb[(int64_t)rreq * JK];
        const double ra = act ? rav : 0.0;
        pend[i].t = LOWER ? rt : -rt;
        pend[i].x = rx;
        pend[i].a = ra;
        pend[i].f = (isrow && sreq == len1) ? ra * rx : (act ? rf : 0.0);   // (position 0: V_0^T Y_0)
        pend[i].slot = so;
      }
      const double a = rgA[so * G + j], x = rgX[so];
      const double f = hasm ? rgB[sd * G + j] : 0.0;   // F_s[j, k] of the current row
      const bool fed = isout && hasm, step = isrow && m + 1 < S;
      const double lag = fed ? tq - tm : (step ? tm - tm1 : 0.0);   // non-negative
      const double e = exp_decay(-(cj * lag));
      // output: bU = e F_s bZ, G += U e bZ.  row: bV = G y, bY = V . G, the decay's part of bc, G <- p G
      const double w = isout ? e * (f * x) : Gs * x;      // bU_q[j] | bV_s[j], this column's part
      const double r = isout ? a * w : Gs * (f - a * x);
      bcj = fma(-lag, r, bcj);
      double red1 = cj * (a * w), red2 = a * Gs;
      Gs = isout ? fma(a * e, x, Gs) : (isrow ? e * Gs : Gs);
      gsum2<G>(red1, red2);
      if ((isout || isrow) && L.valid) {
        const int row = isout ? arrN(n) : arrM(m);
        double *pj = (isout ? bUb : bVb) + (int64_t)row * J;
        double *ps = (isout ? bt1b : bt2b) + row;
        const double bt = (isout == LOWER) ? 0.0 - red1 : red1;
        if (acc) {
          if (act) *pj += w;
          if (j == 0) *ps += bt;
        } else {
          if (act) *pj = w;
          if (j == 0) *ps = bt;
        }
        if (isrow && j == 0) bYb[(int64_t)row * nrhs] = red2;
      }
      lds_order();   // (the next event's arrival may overwrite a slot this one read)
      n += isout ? 1 : 0;
      m += isrow ? 1 : 0;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (L.valid && act) {
    double *p = bc + L.b * J + j;
    *p = acc ? *p + bcj : bcj;
  }
}

template <int G, bool LOWER>
inline void launch(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1, int64_t t1_bs, const double *t2,
                   int64_t t2_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Y,
                   const double *F, const double *bZ, double *bt1, double *bt2, double *bc, double *bU, double *bV, double *bY,
                   hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  for (int64_t k = 0; k < nrhs; ++k)
    hipLaunchKernelGGL((k_general_rev<G, LOWER>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, nrhs, k, k > 0 ? 1 : 0, t1,
                       t1_bs, t2, t2_bs, c, c_bs, U, V, Y, F, bZ, bt1, bt2, bc, bU, bV, bY);
}

template <bool LOWER>
inline int entry(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1, int64_t t1_bs, const double *t2,
                 int64_t t2_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Y, const double *F,
                 const double *bZ, double *bt1, double *bt2, double *bc, double *bU, double *bV, double *bY, c2_stream_t stream) {
  if (B < 1 || N < 1 || M < 1 || J < 1 || nrhs < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t1 || !t2 || !c || !U || !V || !Y || !F || !bZ || !bt1 || !bt2 || !bc || !bU || !bV || !bY) return C2_ERR_INVALID;
  if (N + M > 0x7ffffff0LL || (B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    launch<decltype(g)::value, LOWER>(B, N, M, J, nrhs, t1, t1_bs, t2, t2_bs, c, c_bs, U, V, Y, F, bZ, bt1, bt2, bc, bU, bV, bY, s);
  });
  return launch_ok();
}

}  // namespace general_rev
}  // namespace c2

using namespace c2;

extern "C" int c2_general_matmul_lower_rev(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                                           int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs,
                                           const double *U, const double *V, const double *Y, const double *F,
                                           const double *bZ, double *bt1, double *bt2, double *bc, double *bU, double *bV,
                                           double *bY, c2_stream_t stream) {
  return general_rev::entry<true>(B, N, M, J, nrhs, t1, t1_bs, t2, t2_bs, c, c_bs, U, V, Y, F, bZ, bt1, bt2, bc, bU, bV, bY, stream);
}
extern "C" int c2_general_matmul_upper_rev(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                                           int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs,
                                           const double *U, const double *V, const double *Y, const double *F,
                                           const double *bZ, double *bt1, double *bt2, double *bc, double *bU, double *bV,
                                           double *bY, c2_stream_t stream) {
  return general_rev::entry<false>(B, N, M, J, nrhs, t1, t1_bs, t2, t2_bs, c, c_bs, U, V, Y, F, bZ, bt1, bt2, bc, bU, bV, bY, stream);
}
