// c2_trial_sweep.hpp -- THE FORWARD SWEEP THAT CARRIES ONE TRIAL PER LANE, once for every kind of trial: the row staging
// (sweep_rows), the kernel (k_trial_sweep<Column, JR, QR>) and its launcher (launch_sweep<Column>), behind
// c2_whitened_sinusoids (c2_periodogram.hip), c2_whitened_transits (c2_transit.hip), c2_whitened_keplerians (c2_kepler.hip)
// and c2_whitened_shapes (c2_shapes.hip), which differ in the column source alone (c2_trial_columns.hpp).  The kernel runs
// internal::forward (internal.hpp:107-146) on right-hand sides that
// its lanes form in registers; everything else about a row -- t_n, 1 / d_n, the Z0 row, u_n, w_{n-1}, p_n -- is the same for
// all 64 lanes: the wavefront stages R rows at a time in LDS, lane (r, j) loading u, w and forming ONE decay factor, and
// every lane reads the block back by broadcast.  The next block's global loads are issued before a block's rows are swept
// and staged after them (one wavefront per block, LDS in order: one buffer does).  Row 0 is staged with p = 1 and
// w_{-1} = 0, which leave a state that starts at zero at zero: the row body has no first-row case.
#pragma once
#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "c2_launch.hpp"
#include "c2_trial_columns.hpp"

namespace c2 {
namespace trial {

constexpr int kMaxQ0 = 8;   // columns of Z0 a trial kernel takes (QR: Q0 rounded up to 1, 2, 4 or 8)

// row(x, p, w, u, z0) for n = 0 .. N - 1 of series b, in order: x is the LDS pair (t_n, 1 / d_n), p, w, u are the LDS rows
// p_n, w_{n-1}, u_n (JR doubles, zero beyond J) and z0 the row Z0[n] (QR doubles, zero beyond Q0).  (x is handed over as a
// pointer, not as two values: a body that branches on t_n before it needs 1 / d_n -- the transit's ramp -- then waits for 8
// bytes at the head of the row, not 16, and reads 1 / d_n with the rest of the row behind the branch.)  The state of the
// recurrence and the sums are the calling kernel's, captured by `row`.  JR: J rounded up to 4, 8, 16 or 32; R: rows per
// staged block (kWave / JR divides it).  One wavefront per block.
template <int JR, int QR, int R, class Row>
__device__ __forceinline__ void sweep_rows(int64_t N, int J, int Q0, int64_t b, const double *__restrict__ t, int64_t t_bs,
                                           const double *__restrict__ c, int64_t c_bs, const double *__restrict__ U,
                                           const double *__restrict__ W, const double *__restrict__ d,
                                           const double *__restrict__ Z0, Row &&row) {
  constexpr int RPL = kWave / JR, NV = R / RPL;             // rows one pass of the wavefront covers; passes per block
  constexpr int NZ = (R * QR + kWave - 1) / kWave;          // passes over the block's Z0 rows
  __shared__ __attribute__((aligned(16))) double sp[R][JR], sw[R][JR], su[R][JR];
  __shared__ __attribute__((aligned(16))) double sx[R][2], sz[R][QR];   // sx: (t_n, 1 / d_n)
  const int lane = threadIdx.x;
  const int j = lane & (JR - 1), r0 = lane / JR;
  const bool act = j < J;                                    // this lane stages column j of U, W and forms p_j
  const double *tb = t + b * t_bs, *db = d + b * N, *Zb = Z0 + b * N * Q0;
  const double *Ub = U + b * N * J + (act ? j : 0), *Wb = W + b * N * J + (act ? j : 0);
  const double cj = act ? c[b * c_bs + j] : 0.0;

  // the staged block: what this lane loads for rows n0 + r0, n0 + r0 + RPL, ...
  double vu[NV], vw[NV], vdt[NV], vt = 0.0, vd = 1.0, vz[NZ];
  auto vload = [&](int64_t n0) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      int64_t n = n0 + r0 + m * RPL;
      n = n < N - 1 ? n : N - 1;
      const int64_t nm = n > 0 ? n - 1 : 0;                  // (row 0: p = 1 and w_{-1} = 0 leave the state at zero)
      const double u = Ub[n * J], w = Wb[nm * J];            // (an idle lane reads column 0 and drops it)
      vu[m] = act ? u : 0.0;
      vw[m] = act && n > 0 ? w : 0.0;
      vdt[m] = tb[nm] - tb[n];
    }
    if (lane < R) {
      int64_t n = n0 + lane;
      n = n < N - 1 ? n : N - 1;
      vt = tb[n]; vd = db[n];
    }
#pragma unroll
    for (int m = 0; m < NZ; ++m) {
      const int e = lane + m * kWave, k = e % QR;
      int64_t n = n0 + e / QR;
      n = n < N - 1 ? n : N - 1;                             // (e >= R * QR: a valid row, not staged)
      const double z0 = Zb[n * Q0 + (k < Q0 ? k : 0)];
      vz[m] = k < Q0 ? z0 : 0.0;
    }
  };
  auto vstage = [&]() {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int r = r0 + m * RPL;
      sp[r][j] = exp_decay(cj * vdt[m]);                     // internal.hpp:139
      sw[r][j] = vw[m]; su[r][j] = vu[m];
    }
    if (lane < R) { sx[lane][0] = vt; sx[lane][1] = rcp_nr(vd); }
#pragma unroll
    for (int m = 0; m < NZ; ++m) {
      const int e = lane + m * kWave;
      if (R * QR >= (m + 1) * kWave || e < R * QR) sz[e / QR][e % QR] = vz[m];
    }
  };

  vload(0);
  for (int64_t n0 = 0; n0 < N; n0 += R) {
    lds_order();   // (the rows of the last block are read)
    vstage();
    lds_order();
    if (n0 + R < N) vload(n0 + R);
    const int rows = N - n0 < R ? (int)(N - n0) : R;
#pragma unroll 1
    for (int r = 0; r < rows; ++r) row(sx[r], sp[r], sw[r], su[r], sz[r]);
  }
}

// THE KERNEL (JR: J rounded up to 4, 8, 16 or 32; QR: Q0 rounded up to 1, 2, 4 or 8).  ONE LANE PER TRIAL: a wavefront takes
// 64 consecutive trials of one series and needs no exchange between lanes; a lane holds its column source, the NC columns
// of the state F (NC JR registers) and its sums.  With two columns at JR = 32 the state alone is 128 registers and, with the
// constants of the source, does not fit 256 beside the sums: there a trial takes TWO neighbouring lanes, one column each (32
// trials per wavefront, R = 8 rows a block), both forming both column values, the even lane keeps <z_0, .>, the odd lane
// <z_1, .>, and the one value a row exchanges is the partner's z for <z_0, z_1> (a DPP move inside the quad).  Both forms
// make the same statements per value, so T does not depend on which one ran.
//   F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x NC, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = a_n - F^T u_n                     (:144),   a_n = the column values at t_n
//   T[b, k, :] = [<z, z>, <z, Z0[:, q]> (q < Q0)]                                                        (NC = 1)
//              = [<z_0, z_0>, <z_0, z_1>, <z_1, z_1>, <z_0, Z0[:, q]> (q < Q0), <z_1, Z0[:, q]> (q < Q0)]   (NC = 2)
// with <a, b> = sum_n a_n b_n / d_n.  Lanes with k >= K carry the inert trial and store nothing.  Every element of T is
// written by exactly one lane: no atomics, two calls give identical bits.  Blocks: B * KB in grid.x, KB = ceil(K / trials
// per wavefront), the trial blocks of a series next to each other.
template <class Column>
constexpr int trials_per_wave(int JR) { return Column::NC == 2 && JR >= 32 ? kWave / 2 : kWave; }

template <class Column, int JR, int QR>
__global__ __launch_bounds__(kWave) void k_trial_sweep(int64_t N, int J, int Q0, int64_t K, int64_t KB,
                                                       const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                       int64_t c_bs, const double *__restrict__ U, const double *__restrict__ W,
                                                       const double *__restrict__ d, const double *__restrict__ Z0,
                                                       const double *__restrict__ trials, int64_t tr_bs, double *__restrict__ T,
                                                       const typename Column::Params prm) {
  constexpr int NC = Column::NC;
  constexpr bool SPLIT = trials_per_wave<Column>(JR) < kWave;   // a lane holds one column (column 0: even lane, 1: odd), not both
  constexpr int NL = SPLIT ? 1 : NC;                            // columns a lane holds
  constexpr int R = SPLIT ? 8 : 16;                             // rows per staged block
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / KB, k = (blockIdx.x % KB) * trials_per_wave<Column>(JR) + (SPLIT ? lane >> 1 : lane);
  const bool odd = SPLIT && (lane & 1);
  const Column col(trials + b * tr_bs + (k < K ? k : 0) * Column::WORDS, k < K, b, prm);

  // column 0 (SPLIT: this lane's own) and column 1
  double Fst[NL][JR], T0[NL][QR], Tsq[NL], z[NL], T01 = 0.0;
#pragma unroll
  for (int a = 0; a < NL; ++a) {
#pragma unroll
    for (int i = 0; i < JR; ++i) Fst[a][i] = 0.0;
#pragma unroll
    for (int q = 0; q < QR; ++q) T0[a][q] = 0.0;
    Tsq[a] = z[a] = 0.0;
  }

  // one row: sx = (t_n, 1 / d_n) and the staged LDS rows p_n, w_{n-1}, u_n, Z0[n]
  auto row = [&](const double *sx, const double *sp, const double *sw, const double *su, const double *sz) {
    // (1 / d_n: a two-column source takes it with t_n, one 16-byte read; a one-column source branches on t_n first -- the
    // ramp, the gather -- and reads it behind the branch with the rest of the row: sweep_rows says why)
    double rhs[NC], rd;
    if (NC == 2) rd = sx[1];
    col.columns(sx[0], rhs);
    if (NC == 1) rd = sx[1];
    if (SPLIT) rhs[0] = odd ? rhs[NC - 1] : rhs[0];
    double acc[NL][4];
#pragma unroll
    for (int a = 0; a < NL; ++a) acc[a][0] = acc[a][1] = acc[a][2] = acc[a][3] = 0.0;
#pragma unroll
    for (int i = 0; i < JR; ++i) {
      // (u_n[i] is read beside p and w for a two-column source and at its use for a one-column source: the statement orders of
      // the kernels this one replaces, which the compiler's schedule of the 32-wide row follows -- 8 % of the transit's time)
      const double p = sp[i], w = sw[i];
      double u;
      if (NC == 2) u = su[i];
#pragma unroll
      for (int a = 0; a < NL; ++a) {
        const double fa = p * fma(w, z[a], Fst[a][i]);   // :140, :143
        Fst[a][i] = fa;
        if (NC == 1) u = su[i];
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
    // <z_0, z_1> as (z_0 / d) z_1: column 1's z is the partner lane's when a lane holds one column (kept by the even lane)
    if (NC == 2) T01 = fma(zd[0], SPLIT ? dpp_mov<kDppXor1>(z[0]) : z[NL - 1], T01);
#pragma unroll
    for (int q = 0; q < QR; ++q) {
      const double z0 = sz[q];
#pragma unroll
      for (int a = 0; a < NL; ++a) T0[a][q] = fma(zd[a], z0, T0[a][q]);
    }
  };
  sweep_rows<JR, QR, R>(N, J, Q0, b, t, t_bs, c, c_bs, U, W, d, Z0, row);

  if (k < K) {
    constexpr int HEAD = NC * (NC + 1) / 2;                     // the products among the columns: 1 or 3
    double *Tb = T + (b * K + k) * (HEAD + NC * Q0);
    if (!odd) Tb[0] = Tsq[0];
    if (NC == 2) {
      if (!odd) Tb[1] = T01;
      if (!SPLIT || odd) Tb[2] = Tsq[NL - 1];
    }
#pragma unroll
    for (int q = 0; q < QR; ++q)
      if (q < Q0) {
        if (!odd) Tb[HEAD + q] = T0[0][q];
        if (NC == 2 && (!SPLIT || odd)) Tb[HEAD + Q0 + q] = T0[NL - 1][q];
      }
  }
}

// THE LAUNCHER of c2_whitened_*: the checks of the arguments every kind takes, with the kind's own merged in by stage, the
// blocks of a series, the launch.
template <class Column>
int launch_sweep(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs, const double *c,
                 int64_t c_bs, const double *U, const double *W, const double *d, const double *Z0, const double *trials,
                 int64_t tr_bs, double *T, const typename Column::Params &prm, c2_stream_t stream, const KindChecks &kind = {}) {
  if (B < 1 || N < 1 || J < 1 || Q0 < 1 || K < 1 || kind.bad_size) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || Q0 > kMaxQ0 || kind.too_large) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !Z0 || !trials || !T || t_bs < 0 || c_bs < 0 || tr_bs < 0 || kind.bad_arg) return C2_ERR_INVALID;
  const int64_t tpw = trials_per_wave<Column>(padded(J)), KB = (K + tpw - 1) / tpw;
  if (KB > 0x7fffffffLL || B > 0x7fffffffLL / KB) return C2_ERR_UNSUPPORTED;   // 2^31 blocks or more
  dispatch_padded(J, [&](auto jr) {
    dispatch_columns(Q0, [&](auto qr) {
      hipLaunchKernelGGL((k_trial_sweep<Column, decltype(jr)::value, decltype(qr)::value>), dim3((unsigned)(B * KB)), dim3(kWave), 0,
                         (hipStream_t)stream, N, (int)J, (int)Q0, K, KB, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T, prm);
    });
  });
  return launch_ok();
}

}  // namespace trial
}  // namespace c2
