// c2_predvar.hip -- the EXPLAINED VARIANCE at new times, r_m = k*_m^T (K + D)^-1 k*_m for M sorted query times against the
// factored matrix of N data times (c2_explained_variance, include/celerite2_amd.h): the predictive variance at the
// queries is k(0) - r_m.  Two sweeps over a merge of the two grids, O((N + M) J^2) work and O((N + M) J) memory per
// series; no counterpart in the reference, which forms the N x M cross-covariance and solves against M right-hand sides.
//
// With K + D = L diag(d) L^T, L = I + tril(U W^T o decay), query rows u*, v* at time s, and n the last data row with
// t_n <= s (n = -1 in front of the data):
//   forward state   S'_n = (p p^T) o S'_{n-1} + d_n w_n w_n^T,  p = exp(-c (t_n - t_{n-1}))   (the S of factor after row n)
//   backward state  R_{n+1} = the M of c2_invdiag.hip after row n + 1,  R_N = 0
//   e  = exp(-c (s - t_n)),  uL = u* o e,  h = S'_n uL,  r = uL^T h                                 (0 if n = -1)
//   X  = v* - e o h,  x = exp(-c (t_{n+1} - s)) o X,  r += x^T R_{n+1} x                            (0 if n = N - 1)
// (X is, up to its pivot, the row of W the query would get if it were appended behind row n: the first term is what the
// rows in front of the query explain, the second what the rows behind it add.)
//
// Two stream-ordered launches of ONE kernel template, k_predvar<G, BACK>:
//   BACK = false  walks both grids upwards.  A data event applies the S' update; a query event writes r_m = uL^T h and
//                 X_m into the workspace.  Reads t, d, W, ts, Us, Vs.
//   BACK = true   walks both grids downwards.  A data event is the M update of k_invdiag_group (no q stored, no upper
//                 solve); a query event adds x^T R x to r_m.  Reads t, d, U, W, ts, X.
// Mapping of k_invdiag_group: a group of G lanes per series (J <= G <= 32), lane j owns column j of the symmetric state,
// the state-times-vector product is a lane-local dot product against a vector the group shares through LDS, the scalar
// of an event is one DPP butterfly.  The merge of the two grids, one event per iteration with both kinds predicated, the
// tie rule and the request-ahead LDS ring the rows come through are described in c2_merge_ring.hpp.  A data event and a query
// event are the same arithmetic with different operands -- h = (state) v, s = v^T h with v = p o w or e o X (backward),
// the rank-one update with a zero coefficient and a unit decay for a query (forward) -- so predication costs selects, not
// a second body.
//
// No atomics: every r_m and X_m is written by exactly one lane, two calls give identical bits.  No lane reads another
// series.  No allocation, no host read: the pair can be captured in a graph.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"
#include "c2_merge_ring.hpp"

namespace c2 {
namespace predvar {

// DA, DB: the two rows of a data point (forward: W, W; backward: W, U).  QA, QB: those of a query (forward: Us, Vs;
// backward: X, X).  Forward writes r and X; backward reads a query's r_m eight positions ahead with its row (the d slot of
// the ring, which a query does not otherwise use) and stores r_m plus its own term: every r_m is read before it is written.
// WS (c2_explained_variance_fwd): a data event also stores the state AFTER its update -- column j of S'_n (forward) / of R_n
// (backward) into ws[b, n, j, :], lane j its own J consecutive doubles: what c2_explained_variance_rev reads.
template <int G, bool BACK, bool WS = false>
__global__ __launch_bounds__(kWave) void k_predvar(int64_t B, int N, int M, int J, const double *__restrict__ t, int64_t t_bs,
                                                   const double *__restrict__ ts, int64_t ts_bs,
                                                   const double *__restrict__ c, int64_t c_bs,
                                                   const double *__restrict__ d, const double *__restrict__ DA,
                                                   const double *__restrict__ DB, const double *QA, const double *QB,
                                                   double *r, double *X, double *__restrict__ ws = nullptr) {
  constexpr int SPW = kWave / G, RD = kRing, PD = kPend, NS = kSlots;
  using Lay = RingLayout<G, 2, 0, 4>;   // scalars: time and d; the four vectors below
  constexpr int RS = Lay::kStride;
  __shared__ __attribute__((aligned(16))) double ring[SPW * RS];
  __shared__ __attribute__((aligned(16))) double sv[kWave], sp[kWave], su[kWave], sh[kWave];
  const Geo<G> L(B, J);
  const int j = L.j, grp = L.lane / G, g0 = grp * G;
  const bool act = L.act;
  const double *tb = t + L.b * t_bs, *tsb = ts + L.b * ts_bs, *db = d + L.b * N;
  const double *DAb = DA + L.b * N * J + L.jj, *DBb = DB + L.b * N * J + L.jj;
  const double *QAb = QA + L.b * M * J + L.jj, *QBb = QB + L.b * M * J + L.jj;
  double *rb = r + L.b * M, *Xb = BACK ? nullptr : X + L.b * M * J + L.jj;
  const double cj = act ? c[L.b * c_bs + j] : 0.0;

  double *rgT = ring + grp * RS, *rgD = rgT + Lay::kScal, *rgA = rgD + Lay::kScal, *rgB = rgA + NS * G;
  // positions run 0, 1, 2, ... along the walk; row(pos) is the array index
  auto rowN = [&](int s) { return BACK ? N - 1 - s : s; };
  auto rowM = [&](int s) { return BACK ? M - 1 - s : s; };

  double St[G];   // column j of S' (forward) / of R (backward)
#pragma unroll
  for (int i = 0; i < G; ++i) St[i] = 0.0;

  // the first RD positions of both streams (clamped at the end of a grid); the spare slot holds zeros (d: one)
  rgT[2 * RD] = 0.0; rgD[2 * RD] = 1.0; rgA[2 * RD * G + j] = 0.0; rgB[2 * RD * G + j] = 0.0;
  for (int q = 0; q < RD; ++q) {
    const int rn = rowN(q < N ? q : N - 1), rm = rowM(q < M ? q : M - 1);
    const double a0 = DAb[(int64_t)rn * J], b0 = DBb[(int64_t)rn * J], a1 = QAb[(int64_t)rm * J], b1 = QBb[(int64_t)rm * J];
    rgT[q] = tb[rn]; rgD[q] = db[rn];
    rgA[q * G + j] = act ? a0 : 0.0; rgB[q * G + j] = act ? b0 : 0.0;
    rgT[RD + q] = tsb[rm]; rgD[RD + q] = BACK ? rb[rm] : 1.0;
    rgA[(RD + q) * G + j] = act ? a1 : 0.0; rgB[(RD + q) * G + j] = act ? b1 : 0.0;
  }
  lds_order();

  struct Pend { double t, d, a, b; int slot; };
  Pend pend[PD];
#pragma unroll
  for (int k = 0; k < PD; ++k) pend[k] = Pend{0.0, 1.0, 0.0, 0.0, 2 * RD};

  int n = 0, m = 0;        // positions of the next data row and the next query
  double tref = 0.0;       // time of the data row taken last (n > 0)
  const int total = N + M; // (the launcher refuses N + M >= 2^31)

  for (int it = 0; it < total; it += PD) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      // the row requested PD events ago arrives (never the slot this event reads: it was left PD events ago)
      {
        const Pend &pk = pend[k];
        rgT[pk.slot] = pk.t; rgD[pk.slot] = pk.d; rgA[pk.slot * G + j] = pk.a; rgB[pk.slot * G + j] = pk.b;
      }
      const double tn = rgT[n & (RD - 1)], tq = rgT[RD + (m & (RD - 1))];
      const bool hasn = n < N, hasm = m < M;
      const bool isd = hasn && (!hasm || (BACK ? tn > tq : tn <= tq));   // (the tie rule: c2_merge_ring.hpp)
      const bool isq = !isd && hasm;
      const int pos = isd ? n : m, len1 = (isd ? N : M) - 1;
      const int so = (isd || isq) ? (pos & (RD - 1)) + (isd ? 0 : RD) : 2 * RD;
      {   // the request of this event: the row RD positions down the moving stream (clamped at the end of its grid)
        const int sreq = pos + RD < len1 ? pos + RD : len1;
        const int rreq = BACK ? len1 - sreq : sreq;
        const double *pt = (isd ? tb : tsb) + rreq;
        const double *pd = isd ? db + rreq : (BACK ? rb + rreq : db);   // backward: a query's d slot carries its forward r_m
        const double *pa = (isd ? DAb : QAb) + (int64_t)rreq * J;
        const double *pb = (isd ? DBb : QBb) + (int64_t)rreq * J;
        const double ra = *pa, rbv = *pb, rd = *pd;   // (an idle lane reads column 0 and drops it)
        pend[k].t = *pt;
        pend[k].d = (isd || BACK) ? rd : 1.0;
        pend[k].a = act ? ra : 0.0;
        pend[k].b = act ? rbv : 0.0;
        pend[k].slot = so;
      }
      const double tev = isd ? tn : tq;
      const double ea = rgA[so * G + j], eb = rgB[so * G + j];
      const double dslot = rgD[so];
      const double dn = (isd || !BACK) ? dslot : 1.0;   // (forward: 1 in a query's slot)
      // decay from the data row taken last to this event (no row taken yet: the state is zero, any finite factor does)
      const double dt = n > 0 ? (BACK ? tev - tref : tref - tev) : 0.0;
      const double e = exp_decay(cj * dt);
      double s;
      if constexpr (!BACK) {
        // data: S'_ij <- p_i p_j S'_ij + d w_i w_j.  query: h = S' (u* o e), r = (u* o e)^T h, X = v* - e o h; S' kept
        const double v = isd ? ea : ea * e;
        const double pj = isd ? e : 1.0;
        const double dw = isd ? dn * ea : 0.0;
        sv[L.lane] = v; sp[L.lane] = pj;
        lds_order();
        double h = 0.0;   // (the product and the update in one pass over the columns)
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const double vi = sv[g0 + i];
          h = fma(St[i], vi, h);
          St[i] = fma(dw, vi, (sp[g0 + i] * pj) * St[i]);
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (eight columns at a time: look-ahead costs registers)
        }
#pragma unroll
        for (int i = 0; i < G; ++i) pin(St[i]);
        s = gsum<G>(v * h);
        if (isq && L.valid) {
          const int row = rowM(m);
          if (act) Xb[(int64_t)row * J] = fma(-e, h, eb);
          if (j == 0) rb[row] = s;
        }
      } else {
        // data: the update of k_invdiag_group.  query: x = e o X, r += x^T R x; R kept (u = 0, p = 1)
        const double v = e * ea;             // p o w  /  e o X
        const double pj = isd ? e : 1.0;
        const double un = isd ? eb : 0.0;
        sv[L.lane] = v; sp[L.lane] = pj; su[L.lane] = un;
        lds_order();
        double h = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          h = fma(St[i], sv[g0 + i], h);
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
        s = gsum<G>(v * h);
        const double qn = rcp_nr(dn) + s;
        sh[L.lane] = h;
        lds_order();
        const double ee = isd ? fma(qn, un, -(pj * h)) : 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const double x = fma(-sh[g0 + i], un, pj * St[i]);
          St[i] = fma(su[g0 + i], ee, sp[g0 + i] * x);
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < G; ++i) pin(St[i]);
        if (isq && L.valid && j == 0) rb[rowM(m)] = dslot + s;   // (its forward part came through the ring: no load to wait for)
      }
      if constexpr (WS) {
        if (isd && L.valid && act) {
          double *sw = ws + ((L.b * N + rowN(n)) * J + j) * J;
#pragma unroll
          for (int i = 0; i < G; ++i)
            if (i < J) sw[i] = St[i];
        }
      }
      lds_order();   // (the next event overwrites the vectors)
      tref = isd ? tn : tref;
      n += isd ? 1 : 0;
      m += isq ? 1 : 0;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int G>
inline void launch_ws(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *ts, int64_t ts_bs,
                      const double *c, int64_t c_bs, const double *U, const double *W, const double *d, const double *Us,
                      const double *Vs, double *r, double *work, double *Sws, double *Rws, hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  hipLaunchKernelGGL((k_predvar<G, false, true>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, t, t_bs, ts, ts_bs, c, c_bs,
                     d, W, W, Us, Vs, r, work, Sws);
  hipLaunchKernelGGL((k_predvar<G, true, true>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, t, t_bs, ts, ts_bs, c, c_bs,
                     d, W, U, (const double *)work, (const double *)work, r, (double *)nullptr, Rws);
}

template <int G>
inline void launch(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *ts, int64_t ts_bs,
                   const double *c, int64_t c_bs, const double *U, const double *W, const double *d, const double *Us,
                   const double *Vs, double *r, double *work, hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  hipLaunchKernelGGL((k_predvar<G, false>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, t, t_bs, ts, ts_bs, c, c_bs, d,
                     W, W, Us, Vs, r, work, (double *)nullptr);
  hipLaunchKernelGGL((k_predvar<G, true>), grid, dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, t, t_bs, ts, ts_bs, c, c_bs, d,
                     W, U, (const double *)work, (const double *)work, r, (double *)nullptr, (double *)nullptr);
}

}  // namespace predvar
}  // namespace c2

using namespace c2;
using namespace c2::predvar;

extern "C" int c2_explained_variance(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs,
                                     const double *ts, int64_t ts_bs, const double *c, int64_t c_bs, const double *U,
                                     const double *W, const double *d, const double *Us, const double *Vs, double *r,
                                     double *work, c2_stream_t stream) {
  if (B < 1 || N < 1 || M < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t || !ts || !c || !U || !W || !d || !Us || !Vs || !r || !work) return C2_ERR_INVALID;
  if (N + M > 0x7ffffff0LL || (B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) { launch<decltype(g)::value>(B, N, M, J, t, t_bs, ts, ts_bs, c, c_bs, U, W, d, Us, Vs, r, work, s); });
  return launch_ok();
}

extern "C" int c2_explained_variance_fwd(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs,
                                         const double *ts, int64_t ts_bs, const double *c, int64_t c_bs, const double *U,
                                         const double *W, const double *d, const double *Us, const double *Vs, double *r,
                                         double *work, double *Sws, double *Rws, c2_stream_t stream) {
  if (B < 1 || N < 1 || M < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t || !ts || !c || !U || !W || !d || !Us || !Vs || !r || !work || !Sws || !Rws) return C2_ERR_INVALID;
  if (N + M > 0x7ffffff0LL || (B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    launch_ws<decltype(g)::value>(B, N, M, J, t, t_bs, ts, ts_bs, c, c_bs, U, W, d, Us, Vs, r, work, Sws, Rws, s);
  });
  return launch_ok();
}
