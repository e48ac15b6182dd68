// c2_invdiag_rev.hip -- the REVERSE of the inverse-diagonal sweep (c2_inverse_diag_rev, include/celerite2_amd.h): cotangents
// of q = diag((K + D)^-1) and of alpha = (K + D)^-1 r back to (t, c, U, W, d, z).  What makes the leave-one-out predictive
// density a training objective (autograd.loo_log_predictive[_kernel]); no counterpart in the reference.
//
// The forward sweep (c2_invdiag.hip) runs n = N-1 .. 0 with the symmetric state M and the solve's F; its workspace form
// stores the M and F ENTERING every row (Mws, Fws).  The reverse runs upwards, n = 0 .. N-1, with the adjoint state
// Mb (symmetric J x J) and Fb (J), both 0 in front of row 0.  At row n, with p = exp(-c (t_{n+1} - t_n)) (1 at n = N-1),
// G = (p p^T) o M, g = G w, Fp = p o F:
//   a_  = balpha_n + u.Fb        bu  = alpha_n Fb          Fbp = Fb - a_ w
//   bz_n = a_ / d_n              bd_n = -a_ z_n / d_n^2    bw  = -a_ Fp
//   Mu  = Mb u                   q_  = bq_n + u.Mu         gb  = -2 Mu + q_ w
//   bu += -2 Mb g + 2 q_n Mu     bd_n += -q_ / d_n^2       bw += q_ g + G gb
//   Gb  = Mb + (gb w^T + w gb^T) / 2
//   pb  = 2 (Gb o M) p + F o Fbp
//   Mb <- (p p^T) o Gb           Fb <- p o Fbp
//   n < N-1:  bc += -(t_{n+1} - t_n) pb o p ;  x_n = -sum_j c_j pb_j p_j ;  bt_n = x_{n-1} - x_n   (x_{-1} = x_{N-1} = 0)
//
// The mapping is the forward kernel's: a GROUP of G lanes per series, lane j owns column j of Mb and reads column j of Mws
// (J consecutive doubles).  Mb u, G w, Mb g, G gb and the pb sum are lane-local dot products (by symmetry) against vectors
// the group shares through LDS -- two rounds per row: (u, w, p, p o w), then (g, gb, p o gb), gb needing only the first
// round's reductions.  u.Fb and u.Mu are one interleaved DPP butterfly, x a second one off the critical path.  bc is a
// register per lane stored once; every output element has one writer: no atomics, two calls give identical bits.  The scalar
// streams (t, d, q, bq, z, alpha, balpha in; bt, bd, bz out) move transposed in blocks of 16 rows.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"
#include "c2_merge_ring.hpp"

namespace c2 {
namespace invdiag_rev {

constexpr int kRows = 16;   // rows per block of the scalar streams, as in the forward kernel

template <int G, bool HASZ>
__global__ __launch_bounds__(kWave) void k_invdiag_rev(
    int64_t B, int64_t N, int J, const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c, int64_t c_bs,
    const double *__restrict__ U, const double *__restrict__ W, const double *__restrict__ d, const double *__restrict__ z,
    const double *__restrict__ q, const double *__restrict__ alpha, const double *__restrict__ Mws,
    const double *__restrict__ Fws, const double *__restrict__ bq, const double *__restrict__ balpha, double *__restrict__ bt,
    double *__restrict__ bc, double *__restrict__ bU, double *__restrict__ bW, double *__restrict__ bd,
    double *__restrict__ bz) {
  constexpr int SPW = kWave / G, R = kRows, NV = (R + G - 1) / G;
  constexpr int UN = 4;                 // rows per trip of the row loop: ring slots are compile-time
  constexpr int RD = 4;                 // ring of U, W, F rows: three rows of look-ahead
  // ring of M columns: three rows of look-ahead, one at G = 16; none at G = 32, where Mb and one column of M are 128 registers
  // and a second column spills
  constexpr int MD = G <= 8 ? 4 : (G == 16 ? 2 : 1);
  constexpr int NS = HASZ ? 7 : 4;      // streams: t_n - t_{n+1}, d, q, bq [, z, alpha, balpha]
  static_assert(R % UN == 0 && UN % RD == 0 && UN % MD == 0, "ring slots by row index");
  __shared__ __attribute__((aligned(16))) double spw[kWave], su[kWave], sw[kWave], sp[kWave], sg[kWave], spg[kWave], sgb[kWave];
  // one block of the input streams; a row's outputs replace inputs it has consumed (bt: slot 0, bd: 1, bz: 4)
  __shared__ __attribute__((aligned(16))) double sc[NS][SPW][R];
  const Geo<G> L(B, J);
  const int j = L.j, grp = L.lane / G, g0 = grp * G;
  const bool act = L.act;
  const double *tb = t + L.b * t_bs;
  const double *sin_[7] = {nullptr, d + L.b * N, q + L.b * N, bq + L.b * N, HASZ ? z + L.b * N : nullptr,
                           HASZ ? alpha + L.b * N : nullptr, HASZ ? balpha + L.b * N : nullptr};
  const double *Ub = U + L.b * N * J + L.jj, *Wb = W + L.b * N * J + L.jj;
  const double *Fwb = HASZ ? Fws + L.b * N * J + L.jj : nullptr;
  const double *Mwb = Mws + (L.b * N * J + L.jj) * J;   // column jj of row 0; a row is J * J further
  double *bUb = bU + L.b * N * J + L.jj, *bWb = bW + L.b * N * J + L.jj;
  const double cj = act ? c[L.b * c_bs + j] : 0.0;

  double Mb[G];   // column j of the adjoint state
#pragma unroll
  for (int i = 0; i < G; ++i) Mb[i] = 0.0;
  double Fb = 0.0, bcj = 0.0, xprev = 0.0;

  // transposed scalar streams: lane j of a group takes rows n0 + j, n0 + G + j, ... of a block
  double vs[NS][NV];
  auto vload = [&](int64_t n0) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      int64_t n = n0 + m * G + j;
      n = n < N - 1 ? n : N - 1;
      const int64_t n1 = n < N - 1 ? n + 1 : N - 1;
      vs[0][m] = tb[n] - tb[n1];   // (0 at n = N - 1: p = 1)
#pragma unroll
      for (int k = 1; k < NS; ++k) vs[k][m] = sin_[k][n];
    }
  };
  auto vstage = [&]() {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int idx = m * G + j;
      if (G * NV == R || idx < R) {
#pragma unroll
        for (int k = 0; k < NS; ++k) sc[k][grp][idx] = vs[k][m];
      }
    }
  };
  double ru[RD], rw[RD], rf[RD];
  auto load_row = [&](auto slot, int64_t n) {
    constexpr int r = decltype(slot)::value;
    n = n < N - 1 ? n : N - 1;
    const double x = Ub[n * J], y = Wb[n * J];   // (an idle lane reads column 0 and drops it)
    ru[r] = act ? x : 0.0;
    rw[r] = act ? y : 0.0;
    if constexpr (HASZ) {
      const double f = Fwb[n * J];
      rf[r] = act ? f : 0.0;
    } else {
      rf[r] = 0.0;
    }
  };
  // Column j of the forward state of the rows in flight, loaded UNCONDITIONALLY (a select on the loaded value turns into a
  // branch around the load and a wait behind it: no look-ahead).  Entries i >= J repeat entry J - 1 and an idle lane holds
  // column 0: neither is ever seen, because every vector they meet is zero there (u, w, and g, gb masked below) and the
  // matching entries of Mb stay zero.
  double Mq[MD][G];
  auto load_M = [&](auto slot, int64_t n) {
    constexpr int k = decltype(slot)::value;
    n = n < N - 1 ? n : N - 1;
    const double *mp = Mwb + n * J * J;
#pragma unroll
    for (int i = 0; i < G; ++i) Mq[k][i] = mp[i < J ? i : J - 1];
  };

  const int64_t nblk = (N + R - 1) / R;
  int64_t n0 = 0;
  vload(0); vstage();
  load_row(std::integral_constant<int, 0>{}, 0);
  load_row(std::integral_constant<int, 1>{}, 1);
  load_row(std::integral_constant<int, 2>{}, 2);
  load_M(std::integral_constant<int, 0>{}, 0);
  if constexpr (MD == 4) {
    load_M(std::integral_constant<int, 1>{}, 1);
    load_M(std::integral_constant<int, 2>{}, 2);
  }
  lds_order();

  auto row = [&](auto rr_tag, int rbase) {
    constexpr int rr = decltype(rr_tag)::value;   // row index mod UN
    const int r = rbase + rr;
    const int64_t n = n0 + r;
    const double ndt = sc[0][grp][r], dn = sc[1][grp][r], qn = sc[2][grp][r], bqn = sc[3][grp][r];
    const double zn = HASZ ? sc[HASZ ? 4 : 0][grp][r] : 0.0, an = HASZ ? sc[HASZ ? 5 : 0][grp][r] : 0.0;
    const double ban = HASZ ? sc[HASZ ? 6 : 0][grp][r] : 0.0;
    const double un = ru[rr % RD], wn = rw[rr % RD], Fn = rf[rr % RD];
    load_row(std::integral_constant<int, (rr + RD - 1) % RD>{}, n + RD - 1);
    load_M(std::integral_constant<int, (rr + MD - 1) % MD>{}, n + MD - 1);
    const double(&Mw)[G] = Mq[rr % MD];
    const double p = exp_decay(cj * ndt);
    const double pw = p * wn;
    spw[L.lane] = pw; su[L.lane] = un; sw[L.lane] = wn; sp[L.lane] = p;
    lds_order();
    double hM = 0.0, Mu = 0.0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
      hM = fma(Mw[i], spw[g0 + i], hM);
      Mu = fma(Mb[i], su[g0 + i], Mu);
      if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (eight columns at a time: look-ahead costs registers)
    }
    const double gj = act ? p * hM : 0.0;   // g = G w
    double uF = un * Fb, uMu = un * Mu;
    if constexpr (HASZ) gsum2<G>(uF, uMu);
    else uMu = gsum<G>(uMu);
    const double a_ = HASZ ? ban + uF : 0.0, q_ = bqn + uMu;
    const double rd = rcp_nr(dn), rd2 = rd * rd;
    const double bzn = a_ * rd, bdn = -fma(a_, zn, q_) * rd2;
    const double Fbp = HASZ ? fma(-a_, wn, Fb) : 0.0;
    const double gb = act ? fma(q_, wn, -2.0 * Mu) : 0.0;
    sg[L.lane] = gj; sgb[L.lane] = gb; spg[L.lane] = p * gb;
    lds_order();
    double Mg = 0.0, hG = 0.0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
      Mg = fma(Mb[i], sg[g0 + i], Mg);
      hG = fma(Mw[i], spg[g0 + i], hG);
      if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
    }
    double bu = fma(2.0 * qn, Mu, -2.0 * Mg), bw = fma(q_, gj, p * hG);
    if constexpr (HASZ) {
      bu = fma(an, Fb, bu);
      bw = fma(-a_, p * Fn, bw);
    }
    if (L.valid && act) { bUb[n * J] = bu; bWb[n * J] = bw; }
    double ps = 0.0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const double Gb = fma(0.5, fma(sgb[g0 + i], wn, sw[g0 + i] * gb), Mb[i]);
      const double pi = sp[g0 + i];
      ps = fma(Gb * Mw[i], pi, ps);
      Mb[i] = (pi * p) * Gb;
      if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < G; ++i) pin(Mb[i]);   // (the update stays in its row)
    double pb = 2.0 * ps;
    if constexpr (HASZ) {
      pb = fma(Fn, Fbp, pb);
      Fb = p * Fbp;
    }
    const double pbp = pb * p;        // (n = N - 1: ndt = 0, and M = F = 0 give pb = 0)
    bcj = fma(ndt, pbp, bcj);         // -(t_{n+1} - t_n) pb p
    const double x = -gsum<G>(cj * pbp);
    if (j == 0) {
      sc[0][grp][r] = xprev - x;
      sc[1][grp][r] = bdn;
      if constexpr (HASZ) sc[4][grp][r] = bzn;
    }
    xprev = x;
    lds_order();   // (the next row overwrites the vectors)
    __builtin_amdgcn_sched_barrier(0);
  };

  for (int64_t blk = 0; blk < nblk; ++blk, n0 += R) {
    if (blk + 1 < nblk) vload(n0 + R);
    const int64_t left = N - n0;
    const int rows = left < R ? (int)left : R;
    int rbase = 0;
    for (; rbase + UN <= rows; rbase += UN) {
      row(std::integral_constant<int, 0>{}, rbase);
      row(std::integral_constant<int, 1>{}, rbase);
      row(std::integral_constant<int, 2>{}, rbase);
      row(std::integral_constant<int, 3>{}, rbase);
    }
    if (rbase < rows) row(std::integral_constant<int, 0>{}, rbase);       // (the last block only)
    if (rbase + 1 < rows) row(std::integral_constant<int, 1>{}, rbase);
    if (rbase + 2 < rows) row(std::integral_constant<int, 2>{}, rbase);
    if (L.valid) {
#pragma unroll
      for (int m = 0; m < NV; ++m) {
        const int idx = m * G + j;
        if ((G * NV == R || idx < R) && idx < rows) {
          bt[L.b * N + n0 + idx] = sc[0][grp][idx];
          bd[L.b * N + n0 + idx] = sc[1][grp][idx];
          if constexpr (HASZ) bz[L.b * N + n0 + idx] = sc[4][grp][idx];
        }
      }
    }
    if (blk + 1 < nblk) { lds_order(); vstage(); lds_order(); }
  }
  if (L.valid && act) bc[L.b * J + j] = bcj;
}

template <int G>
inline void launch(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs, const double *U,
                   const double *W, const double *d, const double *z, const double *q, const double *alpha, const double *Mws,
                   const double *Fws, const double *bq, const double *balpha, double *bt, double *bc, double *bU, double *bW,
                   double *bd, double *bz, hipStream_t s) {
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  if (z)
    hipLaunchKernelGGL((k_invdiag_rev<G, true>), grid, dim3(kWave), 0, s, B, N, (int)J, t, t_bs, c, c_bs, U, W, d, z, q, alpha, Mws,
                       Fws, bq, balpha, bt, bc, bU, bW, bd, bz);
  else
    hipLaunchKernelGGL((k_invdiag_rev<G, false>), grid, dim3(kWave), 0, s, B, N, (int)J, t, t_bs, c, c_bs, U, W, d, z, q, alpha, Mws,
                       Fws, bq, balpha, bt, bc, bU, bW, bd, bz);
}

}  // namespace invdiag_rev
}  // namespace c2

using namespace c2;

extern "C" int c2_inverse_diag_rev(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                   int64_t c_bs, const double *U, const double *W, const double *d, const double *z,
                                   const double *q, const double *alpha, const double *Mws, const double *Fws, const double *bq,
                                   const double *balpha, double *bt, double *bc, double *bU, double *bW, double *bd, double *bz,
                                   c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !q || !Mws || !bq || !bt || !bc || !bU || !bW || !bd) return C2_ERR_INVALID;
  const bool hz = z != nullptr;
  if (hz != (alpha != nullptr) || hz != (Fws != nullptr) || hz != (balpha != nullptr) || hz != (bz != nullptr)) return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    invdiag_rev::launch<decltype(g)::value>(B, N, J, t, t_bs, c, c_bs, U, W, d, z, q, alpha, Mws, Fws, bq, balpha, bt, bc, bU, bW,
                                            bd, bz, s);
  });
  return launch_ok();
}
