// c2_predvar_rev.hip -- the REVERSE of the explained variance at new times (c2_explained_variance_rev,
// include/celerite2_amd.h): the cotangent br (M) of r carried back to t, ts, c, U, W, d, Us, Vs, so that the predictive
// variance at held-out times -- and with it the held-out log predictive density -- is differentiable end to end.  No
// counterpart in the reference; parity is pinned by complex-step derivatives and by dense algebra.
//
// The forward (c2_predvar.hip, its WS form) keeps X (work) and, for every data row n, the states AFTER its update:
// Sws[n] = S'_n and Rws[n] = R_n.  With n(m) the last data row with t_n <= s_m:
//   pass A (BACK = true) undoes the backward sweep, walking UPWARDS with the adjoint Rb = 0; a data row goes first on a tie:
//     query m, n(m) = n-1:  lag = t_n - s ;  eps = exp(-c lag) ;  x = eps o X_m
//                           Rb += br_m x x^T ;  bx = 2 br_m R_n x ;  bVs_m = eps o bx
//                           k = x o bx ;  bc -= lag k ;  bt_n -= c.k ;  bts_m += c.k
//     data n:  p = exp(-c (t_{n+1} - t_n)) ;  G = (p p^T) o R_{n+1}       (n = N-1: G = 0, p = 1)
//              g = G w ;  q = 1/d_n + w.g ;  Mu = Rb u ;  qb = u.Mu ;  gb = -2 Mu + qb w
//              bU_n = -2 Rb g + 2 q Mu ;  bd_n = -qb / d_n^2 ;  bW_n = qb g + G gb ;  Gb = Rb + (gb w^T + w gb^T) / 2
//              n < N-1:  pb = 2 (Gb o R_{n+1}) p ;  k = pb o p ;  bc -= (t_{n+1} - t_n) k ;  bt_{n+1} -= c.k ;  bt_n += c.k
//              Rb <- (p p^T) o Gb
//   pass B (BACK = false) undoes the forward sweep, walking DOWNWARDS with the adjoint Sb = 0; a query goes first on a tie:
//     query m, n(m) = n >= 0:  lag = s - t_n ;  e = exp(-c lag) ;  uL = u* o e ;  h = S'_n uL ;  bX = bVs_m
//                              bh = br_m uL - e o bX ;  be = -h o bX ;  buL = br_m h + S'_n bh
//                              Sb += (bh uL^T + uL bh^T) / 2 ;  bUs_m = e o buL ;  be += u* o buL
//                              k = e o be ;  bc -= lag k ;  bts_m -= c.k ;  bt_n += c.k
//     data n:  bd_n += w^T Sb w ;  bW_n += 2 d_n Sb w
//              n > 0:  p = exp(-c (t_n - t_{n-1})) ;  pb = 2 (Sb o S'_{n-1}) p ;  k = pb o p
//                      bc -= (t_n - t_{n-1}) k ;  bt_n -= c.k ;  bt_{n-1} += c.k ;  Sb <- (p p^T) o Sb
// bVs is the hand-over between the passes (the cotangent of X_m IS that of v*_m); queries with no data row above them get
// bVs = 0 and queries in front of the data bUs = 0, exactly.  bc is summed event by event from these non-negative lags, never
// from the closed form in the times, which cancels.  The states are READ from the workspace, never re-derived: undoing a
// decay is the inverse of a contraction.
//
// Mapping: ONE template, k_predvar_rev<G, BACK>, launched twice on the caller's stream; pass B adds to the bt, bts, bc, bW,
// bd pass A wrote -- a fixed order and no atomics, so two calls give identical bits.  A group of G lanes per series
// (J <= G <= 32, B in grid.x); lane j owns column j of the adjoint state and of the workspace records (J consecutive
// doubles).  Every state-times-vector product is, by symmetry, a lane-local dot product against a vector the group shares
// through LDS; the scalars of an event are DPP butterflies.  The merge of the two grids is walked one event per iteration,
// rows of both streams arriving through the request-ahead ring of c2_merge_ring.hpp; the two kinds of event are two
// predicated bodies, each skipped when no series of the wavefront takes it.  In both passes an event's lag runs to the NEXT
// data row of the walk -- position n for a query, n + 1 for a data row -- and so do the records: a query reads the record
// of position n (`cur`), a data row that of position n + 1 (`nxt`, zero weight behind the last row).  One column load per
// data row: at G <= 16 it is issued one data event ahead into a second column; at G = 32, where the adjoint column and one
// record column are 128 registers, the data event loads the column it needs and keeps it for the queries that follow.
// bt is carried: what the events in front of a data row owe it sits in a register until that row's event stores it, bts_m
// is complete (pass A) or updated once (pass B) at its query: every element has one writer per pass.  No allocation, no
// host read: capturable.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"
#include "c2_merge_ring.hpp"

namespace c2 {
namespace predvar_rev {

// DA, DB: the two rows of a data point (pass A: W, U; pass B: W, W).  QA, QB: those of a query (pass A: X, X; pass B: Us,
// bVs as pass A left it).  ws: Rws (pass A) / Sws (pass B).  bRow: bU (pass A; unused in pass B).  bQ: bVs (pass A) / bUs
// (pass B).  A query's d slot of the ring carries br_m.
template <int G, bool BACK>
__global__ __launch_bounds__(kWave) void k_predvar_rev(int64_t B, int N, int M, int J, const double *__restrict__ t, int64_t t_bs,
                                                       const double *__restrict__ ts, int64_t ts_bs,
                                                       const double *__restrict__ c, int64_t c_bs,
                                                       const double *__restrict__ d, const double *__restrict__ br,
                                                       const double *__restrict__ DA, const double *__restrict__ DB,
                                                       const double *QA, const double *QB, const double *__restrict__ ws,
                                                       double *bt, double *bts, double *bc, double *bRow, double *bW,
                                                       double *bd, double *bQ) {
  constexpr int SPW = kWave / G, RD = kRing, PD = kPend, NS = kSlots;
  constexpr bool UP = BACK;          // pass A walks upwards
  constexpr bool AHEAD = G <= 16;    // a second record column, loaded one data event ahead
  using Lay = RingLayout<G, 2, 0, 7>;   // scalars: time and d | br; the seven vectors below
  constexpr int RS = Lay::kStride;
  __shared__ __attribute__((aligned(16))) double ring[SPW * RS];
  __shared__ __attribute__((aligned(16))) double su[kWave], sw[kWave], sp[kWave], spw[kWave], sg[kWave], sgb[kWave], spg[kWave];
  const Geo<G> L(B, J);
  const int j = L.j, grp = L.lane / G, g0 = grp * G;
  const bool act = L.act;
  const double *tb = t + L.b * t_bs, *tsb = ts + L.b * ts_bs, *db = d + L.b * N, *brb = br + L.b * M;
  const double *DAb = DA + L.b * N * J + L.jj, *DBb = DB + L.b * N * J + L.jj;
  const double *QAb = QA + L.b * M * J + L.jj, *QBb = QB + L.b * M * J + L.jj;
  const double *wsb = ws + (L.b * N * J + L.jj) * J;   // column jj of row 0; a row is J * J further
  double *btb = bt + L.b * N, *btsb = bts + L.b * M, *bdb = bd + L.b * N;
  double *bRb = BACK ? bRow + L.b * N * J + L.jj : nullptr, *bWb = bW + L.b * N * J + L.jj, *bQb = bQ + L.b * M * J + L.jj;
  const double cj = act ? c[L.b * c_bs + j] : 0.0;

  double *rgT = ring + grp * RS, *rgD = rgT + Lay::kScal, *rgA = rgD + Lay::kScal, *rgB = rgA + NS * G;
  // positions run 0, 1, 2, ... along the walk; row(pos) is the array index
  auto rowN = [&](int s) { return UP ? s : N - 1 - s; };
  auto rowM = [&](int s) { return UP ? s : M - 1 - s; };

  double St[G];   // column j of the adjoint state: Rb (pass A) / Sb (pass B)
#pragma unroll
  for (int i = 0; i < G; ++i) St[i] = 0.0;
  // Column j of the record at a position (clamped to the last one, whose weight is then zero), loaded UNCONDITIONALLY.
  // Entries i >= J repeat entry J - 1 and an idle lane holds column 0: neither is ever seen, because every vector they
  // meet is zero there and the matching entries of the adjoint stay zero.
  double cur[G], nxt[G];
  auto load_col = [&](double(&dst)[G], int pos) {
    pos = pos < N - 1 ? pos : N - 1;
    const double *mp = wsb + (int64_t)rowN(pos) * J * J;
#pragma unroll
    for (int i = 0; i < G; ++i) dst[i] = mp[i < J ? i : J - 1];
  };
  load_col(cur, 0);
  if constexpr (AHEAD) load_col(nxt, 1);
  double(&dcol)[G] = AHEAD ? nxt : cur;   // the record a data event reads

  // the first RD positions of both streams (clamped at the end of a grid); the spare slot holds zeros (d: one)
  rgT[2 * RD] = 0.0; rgD[2 * RD] = 1.0; rgA[2 * RD * G + j] = 0.0; rgB[2 * RD * G + j] = 0.0;
  for (int q = 0; q < RD; ++q) {
    const int rn = rowN(q < N ? q : N - 1), rm = rowM(q < M ? q : M - 1);
    const double a0 = DAb[(int64_t)rn * J], b0 = DBb[(int64_t)rn * J], a1 = QAb[(int64_t)rm * J], b1 = QBb[(int64_t)rm * J];
    rgT[q] = tb[rn]; rgD[q] = db[rn];
    rgA[q * G + j] = act ? a0 : 0.0; rgB[q * G + j] = act ? b0 : 0.0;
    rgT[RD + q] = tsb[rm]; rgD[RD + q] = brb[rm];
    rgA[(RD + q) * G + j] = act ? a1 : 0.0; rgB[(RD + q) * G + j] = act ? b1 : 0.0;
  }
  lds_order();

  struct Pend { double t, d, a, b; int slot; };
  Pend pend[PD];
#pragma unroll
  for (int k = 0; k < PD; ++k) pend[k] = Pend{0.0, 1.0, 0.0, 0.0, 2 * RD};

  int n = 0, m = 0;        // positions of the next data row and the next query
  double bcj = 0.0;
  double carry = 0.0;      // what the events so far owe the bt of the next data row
  const int total = N + M; // (the launcher refuses N + M >= 2^31)

  for (int it = 0; it < total; it += PD) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      // the row requested PD events ago arrives (never the slot this event reads: it was left PD events ago)
      {
        const Pend &pk = pend[k];
        rgT[pk.slot] = pk.t; rgD[pk.slot] = pk.d; rgA[pk.slot * G + j] = pk.a; rgB[pk.slot * G + j] = pk.b;
      }
      const double tn = rgT[n & (RD - 1)], tq = rgT[RD + (m & (RD - 1))], tn1 = rgT[(n + 1) & (RD - 1)];
      const bool hasn = n < N, hasm = m < M;
      const bool isd = hasn && (!hasm || (UP ? tn <= tq : tn > tq));   // (the tie rule: c2_merge_ring.hpp)
      const bool isq = !isd && hasm;
      const int pos = isd ? n : m, len1 = (isd ? N : M) - 1;
      const int so = (isd || isq) ? (pos & (RD - 1)) + (isd ? 0 : RD) : 2 * RD;
      {   // the request of this event: the row RD positions down the moving stream (clamped at the end of its grid)
        const int sreq = pos + RD < len1 ? pos + RD : len1;
        const int rreq = UP ? sreq : len1 - sreq;
        const double *pt = (isd ? tb : tsb) + rreq;
        const double *pd = (isd ? db : brb) + rreq;
        const double *pa = (isd ? DAb : QAb) + (int64_t)rreq * J;
        const double *pb = (isd ? DBb : QBb) + (int64_t)rreq * J;
        const double ra = *pa, rbv = *pb;   // (an idle lane reads column 0 and drops it)
        pend[k].t = *pt;
        pend[k].d = *pd;
        pend[k].a = act ? ra : 0.0;
        pend[k].b = act ? rbv : 0.0;
        pend[k].slot = so;
      }
      const double ea = rgA[so * G + j], eb = rgB[so * G + j], ds = rgD[so];
      // the lag to the next data row of the walk: position n + 1 for a data row (none behind the last), n for a query
      const bool step = isd && n + 1 < N, live = isq && hasn;
      const double lag = step ? (UP ? tn1 - tn : tn - tn1) : (live ? (UP ? tn - tq : tq - tn) : 0.0);
      const double e = exp_decay(-(cj * lag));

      if (__any(isd)) {
        const int row = rowN(hasn ? n : N - 1);
        if constexpr (!AHEAD) load_col(cur, isd ? n + 1 : n);
        const double w = isd ? ea : 0.0;
        const double p = step ? e : 1.0;
        if constexpr (BACK) {
          const double u = isd ? eb : 0.0;
          const double pw = step ? p * w : 0.0;
          su[L.lane] = u; sw[L.lane] = w; sp[L.lane] = p; spw[L.lane] = pw;
          lds_order();
          double hM = 0.0, Mu = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            hM = fma(dcol[i], spw[g0 + i], hM);
            Mu = fma(St[i], su[g0 + i], Mu);
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (eight columns at a time: look-ahead costs registers)
          }
          const double gj = act ? p * hM : 0.0;   // g = G w
          double wg = w * gj, uMu = u * Mu;
          gsum2<G>(wg, uMu);
          const double rd = rcp_nr(isd ? ds : 1.0);
          const double qn = rd + wg, q_ = uMu;
          const double gb = act ? fma(q_, w, -2.0 * Mu) : 0.0;
          sg[L.lane] = gj; sgb[L.lane] = gb; spg[L.lane] = step ? p * gb : 0.0;
          lds_order();
          double Mg = 0.0, hG = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            Mg = fma(St[i], sg[g0 + i], Mg);
            hG = fma(dcol[i], spg[g0 + i], hG);
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
          const double bu = fma(2.0 * qn, Mu, -2.0 * Mg), bw = fma(q_, gj, p * hG);
          double ps = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            const double Gb = fma(0.5, fma(sgb[g0 + i], w, sw[g0 + i] * gb), St[i]);
            const double pi = sp[g0 + i];
            ps = fma(Gb * dcol[i], pi, ps);
            St[i] = (pi * p) * Gb;
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = 0; i < G; ++i) pin(St[i]);   // (the update stays in its event)
          const double kk = step ? (2.0 * ps) * p : 0.0;
          bcj = fma(-lag, kk, bcj);
          const double x = gsum<G>(cj * kk);
          if (isd && L.valid) {
            if (act) { bRb[(int64_t)row * J] = bu; bWb[(int64_t)row * J] = bw; }
            if (j == 0) { bdb[row] = -q_ * (rd * rd); btb[row] = carry + x; }
          }
          carry = isd ? -x : carry;
        } else {
          // (what pass A wrote for this row: loaded at the top, added to at the bottom)
          const double oW = bWb[(int64_t)row * J], od = bdb[row], ot = btb[row];
          sw[L.lane] = w; sp[L.lane] = p;
          lds_order();
          double Sw = 0.0, ps = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            const double pi = sp[g0 + i];
            Sw = fma(St[i], sw[g0 + i], Sw);
            ps = fma(St[i] * dcol[i], pi, ps);
            St[i] = (pi * p) * St[i];
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = 0; i < G; ++i) pin(St[i]);
          const double kk = step ? (2.0 * ps) * p : 0.0;
          bcj = fma(-lag, kk, bcj);
          double wSw = w * Sw, x = cj * kk;
          gsum2<G>(wSw, x);
          if (isd && L.valid) {
            if (act) bWb[(int64_t)row * J] = fma(2.0 * ds, Sw, oW);
            if (j == 0) { bdb[row] = od + wSw; btb[row] = ot + (carry - x); }
          }
          carry = isd ? x : carry;
        }
        if constexpr (AHEAD) {   // the record of position n + 1 serves the queries behind this row; the next one is requested
#pragma unroll
          for (int i = 0; i < G; ++i) cur[i] = isd ? nxt[i] : cur[i];
          load_col(nxt, isd ? n + 2 : n + 1);
        }
        lds_order();   // (the next body overwrites the vectors)
      }

      if (__any(isq)) {
        const int row = rowM(hasm ? m : M - 1);
        const double brq = live ? ds : 0.0;
        if constexpr (BACK) {
          const double xq = isq ? e * ea : 0.0;   // x = eps o X
          su[L.lane] = xq;
          lds_order();
          double h = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            const double xi = su[g0 + i];
            h = fma(cur[i], xi, h);
            St[i] = fma(brq * xq, xi, St[i]);
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = 0; i < G; ++i) pin(St[i]);
          const double bx = (2.0 * brq) * h;
          const double kk = xq * bx;
          bcj = fma(-lag, kk, bcj);
          const double ck = gsum<G>(cj * kk);
          if (isq && L.valid) {
            if (act) bQb[(int64_t)row * J] = live ? e * bx : 0.0;
            if (j == 0) btsb[row] = live ? ck : 0.0;
          }
          carry = live ? carry - ck : carry;
        } else {
          const double ot = btsb[row];
          const double us = isq ? ea : 0.0, bX = live ? eb : 0.0;
          const double uL = us * e;
          su[L.lane] = uL;
          lds_order();
          double h = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            h = fma(cur[i], su[g0 + i], h);
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
          const double bh = fma(brq, uL, -(e * bX));
          sw[L.lane] = bh;
          lds_order();
          double Sbh = 0.0;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            const double bhi = sw[g0 + i];
            Sbh = fma(cur[i], bhi, Sbh);
            St[i] = fma(0.5, fma(bhi, uL, su[g0 + i] * bh), St[i]);
            if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int i = 0; i < G; ++i) pin(St[i]);
          const double buL = fma(brq, h, Sbh);
          const double be = fma(us, buL, -(h * bX));
          const double kk = live ? e * be : 0.0;
          bcj = fma(-lag, kk, bcj);
          const double ck = gsum<G>(cj * kk);
          if (isq && L.valid) {
            if (act) bQb[(int64_t)row * J] = live ? e * buL : 0.0;
            if (j == 0 && live) btsb[row] = ot - ck;
          }
          carry = live ? carry + ck : carry;
        }
        lds_order();
      }
      n += isd ? 1 : 0;
      m += isq ? 1 : 0;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (L.valid && act) {
    double *p = bc + L.b * J + j;
    *p = BACK ? bcj : *p + bcj;
  }
}

template <int G>
inline void launch(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *ts, int64_t ts_bs,
                   const double *c, int64_t c_bs, const double *U, const double *W, const double *d, const double *Us,
                   const double *work, const double *Sws, const double *Rws, const double *br, double *bt, double *bts, double *bc,
                   double *bU, double *bW, double *bd, double *bUs, double *bVs, hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  hipLaunchKernelGGL((k_predvar_rev<G, true>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, t, t_bs, ts, ts_bs, c, c_bs, d, br,
                     W, U, work, work, Rws, bt, bts, bc, bU, bW, bd, bVs);
  hipLaunchKernelGGL((k_predvar_rev<G, false>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, t, t_bs, ts, ts_bs, c, c_bs, d,
                     br, W, W, Us, (const double *)bVs, Sws, bt, bts, bc, (double *)nullptr, bW, bd, bUs);
}

}  // namespace predvar_rev
}  // namespace c2

using namespace c2;

extern "C" int c2_explained_variance_rev(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs,
                                         const double *ts, int64_t ts_bs, const double *c, int64_t c_bs, const double *U,
                                         const double *W, const double *d, const double *Us, const double *Vs,
                                         const double *work, const double *Sws, const double *Rws, const double *br, double *bt,
                                         double *bts, double *bc, double *bU, double *bW, double *bd, double *bUs, double *bVs,
                                         c2_stream_t stream) {
  if (B < 1 || N < 1 || M < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t || !ts || !c || !U || !W || !d || !Us || !Vs || !work || !Sws || !Rws || !br || !bt || !bts || !bc || !bU || !bW || !bd ||
      !bUs || !bVs)
    return C2_ERR_INVALID;
  if (N + M > 0x7ffffff0LL || (B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    predvar_rev::launch<decltype(g)::value>(B, N, M, J, t, t_bs, ts, ts_bs, c, c_bs, U, W, d, Us, work, Sws, Rws, br, bt, bts, bc,
                                            bU, bW, bd, bUs, bVs, s);
  });
  return launch_ok();
}
