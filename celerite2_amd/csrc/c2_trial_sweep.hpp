// c2_trial_sweep.hpp -- the ROW STAGING of the forward sweeps that carry one trial per lane (k_sinusoids, c2_periodogram.hip;
// k_transits, c2_transit.hip; k_keplerians, c2_kepler.hip), once.  Such a kernel runs internal::forward (internal.hpp:107-146) on right-hand sides that
// its lanes form in registers; everything else about a row -- t_n, 1 / d_n, the Z0 row, u_n, w_{n-1}, p_n -- is the same for
// all 64 lanes: the wavefront stages R rows at a time in LDS, lane (r, j) loading u, w and forming ONE decay factor, and
// every lane reads the block back by broadcast.  The next block's global loads are issued before a block's rows are swept
// and staged after them (one wavefront per block, LDS in order: one buffer does).  Row 0 is staged with p = 1 and
// w_{-1} = 0, which leave a state that starts at zero at zero: the row body has no first-row case.
#pragma once
#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"

namespace c2 {
namespace trial {

constexpr int kMaxQ0 = 8;   // columns of Z0 a trial kernel takes (QR: Q0 rounded up to 1, 2, 4 or 8)

// row(x, p, w, u, z0) for n = 0 .. N - 1 of series b, in order: x is the LDS pair (t_n, 1 / d_n), p, w, u are the LDS rows
// p_n, w_{n-1}, u_n (JR doubles, zero beyond J) and z0 the row Z0[n] (QR doubles, zero beyond Q0).  (x is handed over as a
// pointer, not as two values: a body that branches on t_n before it needs 1 / d_n -- k_transits' ramp -- then waits for 8
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

}  // namespace trial
}  // namespace c2
