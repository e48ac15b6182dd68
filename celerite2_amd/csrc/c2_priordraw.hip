// c2_priordraw.hip -- a JOINT DRAW OF THE NOISE-FREE PRIOR PROCESS on the merge of two sorted grids, the N data times t
// and the M query times ts (c2_prior_draw, include/celerite2_amd.h): the one piece of a posterior draw at new times by
// Matheron's rule, f_s + K(s, t) (K + D)^-1 (y - mean - f_t - eps), that the library did not have in linear time.  One
// forward sweep, O((N + M) (J^2 + J K)) work per series for K draws, nothing stored per row; no counterpart in the
// reference, which draws from the dense M x M conditional covariance.
//
// The sweep applies the Cholesky factor of the zero-noise kernel matrix on the merged grid to standard normals, one
// row (event) at a time.  An event at time s has rows u, v and K normals z; with the J x J state S of factor and the
// J x K state F of dot_tril (both zero in front of the first event):
//   p = exp(-c (s - s_prev));  S <- (p p^T) o S;  F <- p o F                       (not at the first event)
//   h = S u;  w^ = v - h;  d = u^T w^;  a = u^T v;  f = u^T F                       (a = k(0))
//   if d > tau a:  f += sqrt(d) z;  S += w^ w^^T / d;  F += w^ z^T / sqrt(d)        (else the point is DETERMINED: f as it is)
//   store f (K values) to ft[n] or fs[m]
// w^ = d w is the unnormalised row of W, so a zero pivot never divides: a point that coincides with an earlier one (a
// query at a data time, a repeated query, repeated data times) has d = rounding noise of order J eps k(0), is skipped
// by the threshold tau = 2^-44 (kTau), and gets the value the earlier point fixed.  A skipped point loses at most
// tau k(0) = 5.7e-14 k(0) of variance.
//
// Mapping of k_predvar<G, false> (c2_predvar.hip): a group of G lanes per series (J <= G <= 32), lane j owns column j of
// the symmetric S and row j of F; h is a lane-local dot product against u shared through LDS; d, a and the K values f
// are DPP butterflies.  The merge (one event per iteration with both kinds predicated, data first on a tie: they are the
// same arithmetic with different operand pointers) and the request-ahead LDS ring the rows come through are those of
// c2_merge_ring.hpp, walking upwards; the normals of a row travel with its row (lane j carries normals j, j + G, ...).
//
// The K draws are covered in blocks of KB held in registers (F: KB doubles per lane): KB = 8 (2 at G = 1), and KB = 1
// for a single draw; block number in grid.y, so a larger K is more wavefronts of ONE launch, each of which recomputes S
// (J^2 of the J^2 + J KB work of an event).  B is in grid.x.
//
// No atomics: every f is written by exactly one lane, two calls give identical bits.  No lane reads another series.
// No allocation, no host read: capturable.  A row's normals are read (eight positions ahead of its event, or at the top
// of its event for the last rows of a stream) before its draw is stored, and each block reads and writes its own
// columns only: ft may be nt and fs may be ns.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"
#include "c2_merge_ring.hpp"

namespace c2 {
namespace priordraw {

// draws per register block (K > 1).  One lane per series (G = 1) takes 2: 64 series' rings with eight normals a row
// would need 98 KB of LDS, and at J = 1 the S a further block recomputes is one number.
template <int G>
constexpr int kBlock = G == 1 ? 2 : 8;
constexpr double kTau = 0x1p-44;   // a point with d <= kTau a is determined by the points in front of it

// nt, ns, ft, fs carry no __restrict__: ft may be nt and fs may be ns.
template <int G, int KB>
__global__ __launch_bounds__(kWave) void k_priordraw(int64_t B, int N, int M, int J, int K, const double *__restrict__ t,
                                                     int64_t t_bs, const double *__restrict__ ts, int64_t ts_bs,
                                                     const double *__restrict__ c, int64_t c_bs,
                                                     const double *__restrict__ U, const double *__restrict__ V,
                                                     const double *__restrict__ Us, const double *__restrict__ Vs,
                                                     const double *nt, const double *ns, double *ft, double *fs) {
  constexpr int SPW = kWave / G, RD = kRing, PD = kPend, NS = kSlots;
  constexpr int ZL = (KB + G - 1) / G;   // normals a lane carries per row: j, j + G, ...
  constexpr bool ZALL = (ZL * G == KB);  // every lane's every index is inside the block
  using Lay = RingLayout<G, 1, KB, 3>;   // scalar: the time; a slot's KB normals behind the rows; the three vectors below
  constexpr int RS = Lay::kStride;
  __shared__ __attribute__((aligned(16))) double ring[SPW * RS];
  __shared__ __attribute__((aligned(16))) double su[kWave], sp[kWave], sw[kWave];
  const Geo<G> L(B, J);
  const int j = L.j, grp = L.lane / G, g0 = grp * G;
  const bool act = L.act;
  const int kb0 = (int)blockIdx.y * KB;             // first draw of this block
  const int kc = K - kb0 < KB ? K - kb0 : KB;       // draws in it
  const double *tb = t + L.b * t_bs, *tsb = ts + L.b * ts_bs;
  const double *Ub = U + L.b * N * J + L.jj, *Vb = V + L.b * N * J + L.jj;
  const double *Usb = Us + L.b * M * J + L.jj, *Vsb = Vs + L.b * M * J + L.jj;
  const double *ntb = nt + L.b * N * K + kb0, *nsb = ns + L.b * M * K + kb0;
  double *ftb = ft + L.b * N * K + kb0, *fsb = fs + L.b * M * K + kb0;
  const double cj = act ? c[L.b * c_bs + j] : 0.0;
  int zi[ZL];     // this lane's draw indices inside the block (an index beyond the block reads draw 0 and drops it)
  bool zok[ZL];
#pragma unroll
  for (int q = 0; q < ZL; ++q) {
    zok[q] = j + q * G < kc;
    zi[q] = zok[q] ? j + q * G : 0;
  }

  double *rgT = ring + grp * RS, *rgA = rgT + Lay::kScal, *rgB = rgA + NS * G, *rgZ = rgB + NS * G;
  auto put_z = [&](int slot, int q, double z) {
    if (ZALL || j + q * G < KB) rgZ[slot * KB + j + q * G] = z;
  };

  double St[G];   // column j of S
  double F[KB];   // row j of F
#pragma unroll
  for (int i = 0; i < G; ++i) St[i] = 0.0;
#pragma unroll
  for (int k = 0; k < KB; ++k) F[k] = 0.0;

  // the first RD positions of both streams (clamped at the end of a grid); the spare slot holds zeros
  rgT[2 * RD] = 0.0; rgA[2 * RD * G + j] = 0.0; rgB[2 * RD * G + j] = 0.0;
#pragma unroll
  for (int q = 0; q < ZL; ++q) put_z(2 * RD, q, 0.0);
  for (int s = 0; s < RD; ++s) {
    const int rn = s < N ? s : N - 1, rm = s < M ? s : M - 1;
    const double a0 = Ub[(int64_t)rn * J], b0 = Vb[(int64_t)rn * J], a1 = Usb[(int64_t)rm * J], b1 = Vsb[(int64_t)rm * J];
    rgT[s] = tb[rn];
    rgA[s * G + j] = act ? a0 : 0.0; rgB[s * G + j] = act ? b0 : 0.0;
    rgT[RD + s] = tsb[rm];
    rgA[(RD + s) * G + j] = act ? a1 : 0.0; rgB[(RD + s) * G + j] = act ? b1 : 0.0;
#pragma unroll
    for (int q = 0; q < ZL; ++q) {
      const double z0 = ntb[(int64_t)rn * K + zi[q]], z1 = nsb[(int64_t)rm * K + zi[q]];
      put_z(s, q, zok[q] ? z0 : 0.0);
      put_z(RD + s, q, zok[q] ? z1 : 0.0);
    }
  }
  lds_order();

  struct Pend { double t, a, b, z[ZL]; int slot; };
  Pend pend[PD];
#pragma unroll
  for (int k = 0; k < PD; ++k) {
    pend[k].t = 0.0; pend[k].a = 0.0; pend[k].b = 0.0; pend[k].slot = 2 * RD;
#pragma unroll
    for (int q = 0; q < ZL; ++q) pend[k].z[q] = 0.0;
  }

  int n = 0, m = 0;        // positions of the next data row and the next query
  double tprev = 0.0;      // time of the event before this one (n + m > 0)
  const int total = N + M; // (the launcher refuses N + M >= 2^31)

  for (int it = 0; it < total; it += PD) {
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      // the row requested PD events ago arrives (never the slot this event reads: it was left PD events ago)
      {
        const Pend &pk = pend[k];
        rgT[pk.slot] = pk.t; rgA[pk.slot * G + j] = pk.a; rgB[pk.slot * G + j] = pk.b;
#pragma unroll
        for (int q = 0; q < ZL; ++q) put_z(pk.slot, q, pk.z[q]);
      }
      const double tn = rgT[n & (RD - 1)], tq = rgT[RD + (m & (RD - 1))];
      const bool hasn = n < N, hasm = m < M;
      const bool isd = hasn && (!hasm || tn <= tq);   // (the tie rule: c2_merge_ring.hpp)
      const bool isq = !isd && hasm;
      const bool ev = isd || isq;
      const int pos = isd ? n : m, len1 = (isd ? N : M) - 1;
      const int so = ev ? (pos & (RD - 1)) + (isd ? 0 : RD) : 2 * RD;
      {   // the request of this event: the row RD positions down the moving stream (clamped at the end of its grid)
        const int rreq = pos + RD < len1 ? pos + RD : len1;
        const double *pt = (isd ? tb : tsb) + rreq;
        const double *pa = (isd ? Ub : Usb) + (int64_t)rreq * J;
        const double *pb = (isd ? Vb : Vsb) + (int64_t)rreq * J;
        const double *pz = (isd ? ntb : nsb) + (int64_t)rreq * K;
        const double ra = *pa, rbv = *pb;   // (an idle lane reads column 0 and drops it)
        pend[k].t = *pt;
        pend[k].a = act ? ra : 0.0;
        pend[k].b = act ? rbv : 0.0;
#pragma unroll
        for (int q = 0; q < ZL; ++q) {
          const double rz = pz[zi[q]];
          pend[k].z[q] = zok[q] ? rz : 0.0;
        }
        pend[k].slot = so;
      }
      const double tev = isd ? tn : tq;
      const double uj = rgA[so * G + j], vj = rgB[so * G + j];
      double z[KB];
#pragma unroll
      for (int q = 0; q < KB; ++q) z[q] = rgZ[so * KB + q];
      // decay from the event before (first event: the states are zero, any finite factor does)
      const double dt = (ev && n + m > 0) ? tprev - tev : 0.0;
      const double e = exp_decay(cj * dt);
      su[L.lane] = uj; sp[L.lane] = e;
      lds_order();
      double h = 0.0;   // (the decay and the product in one pass over the columns)
#pragma unroll
      for (int i = 0; i < G; ++i) {
        St[i] = (sp[g0 + i] * e) * St[i];
        h = fma(St[i], su[g0 + i], h);
        if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (eight columns at a time: look-ahead costs registers)
      }
      const double wh = vj - h;
      double d = uj * wh, a = uj * vj;
      gsum2<G>(d, a);
      const bool take = d > kTau * a;
      const double ds = take ? d : 1.0;
      const double inv = rcp_nr(ds);
      const double sq = take ? sqrt(ds) : 0.0;   // sqrt(d), or 0 for a determined point
      const double wd = take ? wh * inv : 0.0;   // w^_j / d
      const double wr = wh * (sq * inv);         // w^_j / sqrt(d)
      sw[L.lane] = wh;
      lds_order();
#pragma unroll
      for (int i = 0; i < G; ++i) {
        St[i] = fma(sw[g0 + i], wd, St[i]);
        if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < G; ++i) pin(St[i]);
      double f[KB];
#pragma unroll
      for (int q = 0; q < KB; ++q) {
        const double Fq = e * F[q];
        f[q] = fma(sq, z[q], gsum<G>(uj * Fq));
        F[q] = fma(wr, z[q], Fq);
      }
#pragma unroll
      for (int q = 0; q < KB; ++q) pin(F[q]);
      if (ev && L.valid) {   // lane j stores draws j, j + G, ... of the block
        double *ob = (isd ? ftb : fsb) + (int64_t)pos * K;
#pragma unroll
        for (int q = 0; q < ZL; ++q) {
          double val = f[q * G < KB ? q * G : 0];
#pragma unroll
          for (int i = 1; i < G && q * G + i < KB; ++i) val = (j == i) ? f[q * G + i] : val;
          if (zok[q]) ob[zi[q]] = val;
        }
      }
      lds_order();   // (the next event overwrites the vectors)
      tprev = ev ? tev : tprev;
      n += isd ? 1 : 0;
      m += isq ? 1 : 0;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int G>
inline int launch(int64_t B, int64_t N, int64_t M, int64_t J, int64_t K, const double *t, int64_t t_bs, const double *ts,
                   int64_t ts_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Us,
                   const double *Vs, const double *nt, const double *ns, double *ft, double *fs, hipStream_t s) {
  constexpr int KB = kBlock<G>;
  const unsigned gx = (unsigned)((B * G + kWave - 1) / kWave);
  if ((K + KB - 1) / KB > 65535) return C2_ERR_UNSUPPORTED;   // (blocks of draws are in grid.y)
  if (K == 1)
    hipLaunchKernelGGL((k_priordraw<G, 1>), dim3(gx, 1), dim3(kWave), 0, s, B, (int)N, (int)M, (int)J, 1, t, t_bs, ts, ts_bs,
                       c, c_bs, U, V, Us, Vs, nt, ns, ft, fs);
  else
    hipLaunchKernelGGL((k_priordraw<G, KB>), dim3(gx, (unsigned)((K + KB - 1) / KB)), dim3(kWave), 0, s, B, (int)N, (int)M,
                       (int)J, (int)K, t, t_bs, ts, ts_bs, c, c_bs, U, V, Us, Vs, nt, ns, ft, fs);
  return launch_ok();
}

}  // namespace priordraw
}  // namespace c2

using namespace c2;
using namespace c2::priordraw;

extern "C" int c2_prior_draw(int64_t B, int64_t N, int64_t M, int64_t J, int64_t K, const double *t, int64_t t_bs,
                             const double *ts, int64_t ts_bs, const double *c, int64_t c_bs, const double *U, const double *V,
                             const double *Us, const double *Vs, const double *nt, const double *ns, double *ft, double *fs,
                             c2_stream_t stream) {
  if (B < 1 || N < 1 || M < 1 || J < 1 || K < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t || !ts || !c || !U || !V || !Us || !Vs || !nt || !ns || !ft || !fs) return C2_ERR_INVALID;
  if (N + M > 0x7ffffff0LL || (B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  return dispatch_group(J, [&](auto g) {
    return launch<decltype(g)::value>(B, N, M, J, K, t, t_bs, ts, ts_bs, c, c_bs, U, V, Us, Vs, nt, ns, ft, fs, s);
  });
}
