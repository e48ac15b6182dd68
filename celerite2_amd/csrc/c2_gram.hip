// c2_gram.hip -- the WHITENED GRAM MATRIX of a design matrix under the factored covariance (c2_whitened_gram,
// include/celerite2_amd_linear.h): for every series, with d, W of c2_factor, A (N, P) shared or (B, N, P) and optionally
// y (B, N),
//   S = [A | y]^T (K + D)^-1 [A | y] = sum_n z_n z_n^T / d_n,      z = L^-1 [A | y]      (Q = P + 1 columns, or P without y)
// in ONE forward sweep that keeps S in registers and never writes Z.  What generalized least squares and the likelihood
// with the linear coefficients marginalised out need (autograd.gls); no counterpart in the reference, whose callers
// compose it from solve_lower (forward.hpp:158-170) and a dense product.
//
// The recurrence is internal::forward (internal.hpp:107-146) with Q right-hand sides, is_solve:
//   F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x Q, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = y_n - F^T u_n                     (:144)
//   S  += z_n z_n^T / d_n
//
// One mapping, k_gram<JR, QR>: a GROUP of G = max(JR, QR) lanes per series (JR, QR: J, Q rounded up to 4, 8, 16 or 32).
// Lane k owns column k of F (JR registers) and column k of S (QR registers).  The row's u_n, w_{n-1}, p_n are loaded or
// formed by lanes j < J and shared through LDS, so z_k is a lane-local dot product; the only exchange a row adds is the
// Q values z for the rank-one update (one LDS write, QR broadcast reads).  (z_i z_k) is rounded before it is scaled by
// 1 / d_n, so S_ik and S_ki are the same bits.  t, d, y move transposed in time, 16 rows per block, as in k_invdiag_group;
// rows of U, W, A are requested RD rows ahead.  Idle lanes (j >= J, k >= Q) carry zeros and store nothing.
// There is no time-parallel form: at one series the sweep is latency-bound like the other row-by-row kernels.
// No atomics anywhere: two calls give identical bits.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_linear.h"
#include "c2_launch.hpp"

namespace c2 {
namespace gram {

constexpr int kRows = 16;   // rows per block of the scalar streams: 128 bytes per series
constexpr int kMaxCols = 32;

template <int JR, int QR>
__global__ __launch_bounds__(kWave) void k_gram(int64_t B, int64_t N, int J, int P, int Q, const double *__restrict__ t,
                                                int64_t t_bs, const double *__restrict__ c, int64_t c_bs,
                                                const double *__restrict__ U, const double *__restrict__ W,
                                                const double *__restrict__ d, const double *__restrict__ A, int64_t a_bs,
                                                const double *__restrict__ y, double *__restrict__ S) {
  constexpr int G = JR > QR ? JR : QR, SPW = kWave / G, R = kRows, NV = (R + G - 1) / G, RD = G >= 32 ? 4 : 8;
  __shared__ __attribute__((aligned(16))) double sp[kWave], sw[kWave], su[kWave], sz[kWave];
  __shared__ __attribute__((aligned(16))) double sc[2][3][SPW][R];
  const Geo<G> L(B, J);
  const int k = L.j, grp = L.lane / G, g0 = grp * G;
  const bool act = L.act;                                    // k < J: this lane loads column k of U, W and forms p_k
  const bool acol = k < P, ycol = y != nullptr && k == P;    // where this lane's column of [A | y] comes from
  const double *tb = t + L.b * t_bs, *db = d + L.b * N, *yb = y ? y + L.b * N : nullptr;
  const double *Ub = U + L.b * N * J + L.jj, *Wb = W + L.b * N * J + L.jj;
  const double *Ab = A + L.b * a_bs + (acol ? k : 0);
  const double cj = act ? c[L.b * c_bs + k] : 0.0;

  double Fc[JR], Sc[QR];
#pragma unroll
  for (int i = 0; i < JR; ++i) Fc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < QR; ++i) Sc[i] = 0.0;
  double tprev = tb[0], wprev = 0.0, zprev = 0.0;   // (row 0: p = 1 and w_{-1} z_{-1} = 0 leave F at zero)

  // transposed scalar streams: lane k of a group takes rows n0 + k, n0 + G + k, ... of a block
  double vt[NV], vd[NV], vy[NV];
  auto vload = [&](int64_t n0) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      int64_t n = n0 + m * G + k;
      n = n < N - 1 ? n : N - 1;
      vt[m] = tb[n]; vd[m] = db[n];
      vy[m] = yb ? yb[n] : 0.0;
    }
  };
  auto vstage = [&](int buf) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int idx = m * G + k;
      if (G * NV == R || idx < R) { sc[buf][0][grp][idx] = vt[m]; sc[buf][1][grp][idx] = vd[m]; sc[buf][2][grp][idx] = vy[m]; }
    }
  };
  double ru[RD], rw[RD], ra[RD];
  auto load_row = [&](int r, int64_t n) {
    n = n < N - 1 ? n : N - 1;
    const double x = Ub[n * J], w = Wb[n * J], a = Ab[n * P];   // (an idle lane reads column 0 and drops it)
    ru[r] = act ? x : 0.0;
    rw[r] = act ? w : 0.0;
    ra[r] = acol ? a : 0.0;
  };

  const int64_t nblk = (N + R - 1) / R;
  int64_t n0 = 0;
  vload(0); vstage(0);
#pragma unroll
  for (int r = 0; r < RD; ++r) load_row(r, r);
  lds_order();
  int buf = 0;

  auto block = [&](auto checked_tag) {
    constexpr bool CHECKED = decltype(checked_tag)::value;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t n = n0 + r;
      if (!CHECKED || n < N) {
        const double tn = sc[buf][0][grp][r], dn = sc[buf][1][grp][r], yn = sc[buf][2][grp][r];
        const double un = ru[r % RD], wn = rw[r % RD], an = ra[r % RD];
        load_row(r % RD, n + RD);
        const double p = exp_decay(cj * (tprev - tn));   // internal.hpp:139
        tprev = tn;
        sp[L.lane] = p; sw[L.lane] = wprev; su[L.lane] = un;
        wprev = wn;
        lds_order();
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < JR; ++i) {
          const double f = sp[g0 + i] * fma(sw[g0 + i], zprev, Fc[i]);   // :140, :143
          Fc[i] = f;
          acc[i & 3] = fma(f, su[g0 + i], acc[i & 3]);
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (eight rows of F at a time: look-ahead costs registers)
        }
        const double zk = (ycol ? yn : an) - ((acc[0] + acc[1]) + (acc[2] + acc[3]));   // :144
        zprev = zk;
        sz[L.lane] = zk;
        lds_order();
        const double rd = rcp_nr(dn);
#pragma unroll
        for (int i = 0; i < QR; ++i) {
          Sc[i] = fma(sz[g0 + i] * zk, rd, Sc[i]);   // (the product first: S_ik and S_ki round alike)
          if (i % 8 == 7) __builtin_amdgcn_sched_barrier(0);
        }
        lds_order();   // (the next row overwrites the vectors)
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  for (int64_t blk = 0; blk < nblk; ++blk, n0 += R) {
    if (blk + 1 < nblk) vload(n0 + R);
    if (blk == nblk - 1) block(std::true_type{});
    else block(std::false_type{});
    if (blk + 1 < nblk) { vstage(buf ^ 1); lds_order(); buf ^= 1; }
  }

  if (L.valid && k < Q) {   // S is symmetric to the bit: lane k stores its column as row k, Q consecutive doubles
    double *Sb = S + (L.b * Q + k) * Q;
#pragma unroll
    for (int i = 0; i < QR; ++i)
      if (i < Q) Sb[i] = Sc[i];
  }
}

}  // namespace gram
}  // namespace c2

using namespace c2;
using namespace c2::gram;

extern "C" int c2_whitened_gram(int64_t B, int64_t N, int64_t J, int64_t P, const double *t, int64_t t_bs, const double *c,
                                int64_t c_bs, const double *U, const double *W, const double *d, const double *A,
                                int64_t a_bs, const double *y, double *S, c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1 || P < 1) return C2_ERR_INVALID;
  const int64_t Q = P + (y ? 1 : 0);
  if (J > C2_FAST_WIDTH || Q > kMaxCols) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !A || !S) return C2_ERR_INVALID;
  const int64_t G = padded(J) > padded(Q) ? padded(J) : padded(Q);
  if ((B * G + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
  dispatch_padded(J, [&](auto jr) {
    dispatch_padded(Q, [&](auto qr) {
      hipLaunchKernelGGL((k_gram<decltype(jr)::value, decltype(qr)::value>), grid, dim3(kWave), 0, s, B, N, (int)J, (int)P,
                         (int)Q, t, t_bs, c, c_bs, U, W, d, A, a_bs, y, S);
    });
  });
  return launch_ok();
}
