// c2_transit.hip -- the WHITENED TRANSIT TEMPLATES of a trial grid under the factored covariance (c2_whitened_transits,
// include/celerite2_amd_transit.h): for every series b and trial k = (period P, epoch t0, duration w, ingress tau), with d, W
// of c2_factor and Z0 = L^-1 [A0 | y - mean] (B, N, Q0) of c2_solve_lower,
//   z = L^-1 b_k(t),   <a, b> = sum_n a_n b_n / d_n,   T[b, k, :] = [<z, z>, <z, Z0[:, j]> (j < Q0)]
// in ONE forward sweep that forms the box or trapezoid b_k in registers and writes neither it nor z: what box least squares
// under correlated noise reads (celerite2_amd/transit.py).  No counterpart in the reference.
//
// The recurrence is internal::forward (internal.hpp:107-146) as restated in c2_gram.hip, with one right-hand side:
//   f <- p_n o (f + w_{n-1} z_{n-1})        (f: J, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = b_n - f^T u_n                     (:144)
// THE TEMPLATE is the header's rule, every line rounded once and none contracted into an fma (template_value below), so a
// numpy restatement takes the same discrete decisions -- which side of a fold, inside or outside an edge -- bit for bit.
//
// k_transits<JR, QR> (JR: J rounded up to 4, 8, 16 or 32; QR: Q0 rounded up to 1, 2, 4 or 8).  ONE LANE PER TRIAL at every
// width: a wavefront takes 64 consecutive trials of one series and needs no exchange between lanes; a lane holds f (JR
// registers), its five trial constants (P, 1 / P, t0, w / 2, tau) and the 1 + QR sums.  It is c2_periodogram.hip's sibling:
// the staging below is k_sinusoids' (a copy: that file's code is left as it is), the row loop is its own.  Everything else
// about a row -- t_n, 1 / d_n, the Z0 row, u_n, w_{n-1}, p_n -- is the same for all 64 lanes: the wavefront stages R = 16
// rows at a time in LDS, lane (r, j) loading u, w and forming ONE decay factor, and every lane reads the block back by
// broadcast.  The next block's global loads are issued before a block's rows are swept and staged after them (one
// wavefront per block, LDS in order: one buffer does).  Lanes with k >= K carry the null trial (0, 0, 0, 0) and store
// nothing.  Every element of T is written by exactly one lane: no atomics, two calls give identical bits.  Blocks:
// B * ceil(K / 64) in grid.x, the trial blocks of a series next to each other.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_transit.h"
#include "c2_launch.hpp"

namespace c2 {
namespace transit {

constexpr int kMaxQ0 = 8;

// b_n of the header's rule from the lane's constants: invP = fl(1 / P), or 0 for a single event (then q = 0 and phi = x);
// hw = 0.5 w (exact).  The ramp's division is met only by a wavefront with a lane on an ingress or egress at that row.
__device__ __forceinline__ double template_value(double t, double P, double invP, double t0, double hw, double tau) {
#pragma clang fp contract(off)
  const double x = t - t0;
  const double q = __builtin_rint(x * invP);
  const double qp = q * P;
  const double phi = x - qp;
  const double u = hw - __builtin_fabs(phi);
  double b = u >= tau ? 1.0 : 0.0;
  const bool ramp = u >= 0.0 && u < tau;
  if (__builtin_amdgcn_ballot_w64(ramp) != 0) b = ramp ? u / tau : b;   // (wave-uniform: the division is skipped, not masked)
  return b;
}

template <int JR, int QR>
__global__ __launch_bounds__(kWave) void k_transits(int64_t N, int J, int Q0, int64_t K, int64_t KB,
                                                    const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                    int64_t c_bs, const double *__restrict__ U, const double *__restrict__ W,
                                                    const double *__restrict__ d, const double *__restrict__ Z0,
                                                    const double *__restrict__ trials, int64_t tr_bs, double *__restrict__ T) {
  constexpr int R = 16;                                     // rows per staged block
  constexpr int RPL = kWave / JR, NV = R / RPL;             // rows one pass of the wavefront covers; passes per block
  constexpr int NZ = (R * QR + kWave - 1) / kWave;          // passes over the block's Z0 rows
  __shared__ __attribute__((aligned(16))) double sp[R][JR], sw[R][JR], su[R][JR];
  __shared__ __attribute__((aligned(16))) double sx[R][2], sz[R][QR];   // sx: (t_n, 1 / d_n)
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / KB, k = (blockIdx.x % KB) * kWave + lane;
  const int j = lane & (JR - 1), r0 = lane / JR;
  const bool act = j < J;                                    // this lane stages column j of U, W and forms p_j
  const double *tb = t + b * t_bs, *db = d + b * N, *Zb = Z0 + b * N * Q0;
  const double *Ub = U + b * N * J + (act ? j : 0), *Wb = W + b * N * J + (act ? j : 0);
  const double cj = act ? c[b * c_bs + j] : 0.0;
  const double *tr = trials + b * tr_bs + (k < K ? k : 0) * 4;
  const double P = k < K ? tr[0] : 0.0, t0 = k < K ? tr[1] : 0.0, hw = k < K ? 0.5 * tr[2] : 0.0, tau = k < K ? tr[3] : 0.0;
  const double invP = P != 0.0 ? 1.0 / P : 0.0;              // (a correctly rounded division, once per lane)

  double f[JR], T0[QR], Tsq = 0.0, z = 0.0;
#pragma unroll
  for (int i = 0; i < JR; ++i) f[i] = 0.0;
#pragma unroll
  for (int q = 0; q < QR; ++q) T0[q] = 0.0;

  // the staged block: what this lane loads for rows n0 + r0, n0 + r0 + RPL, ...
  double vu[NV], vw[NV], vdt[NV], vt = 0.0, vd = 1.0, vz[NZ];
  auto vload = [&](int64_t n0) {
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      int64_t n = n0 + r0 + m * RPL;
      n = n < N - 1 ? n : N - 1;
      const int64_t nm = n > 0 ? n - 1 : 0;                  // (row 0: p = 1 and w_{-1} = 0 leave f at zero)
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
      const int e = lane + m * kWave, q = e % QR;
      int64_t n = n0 + e / QR;
      n = n < N - 1 ? n : N - 1;                             // (e >= R * QR: a valid row, not staged)
      const double z0 = Zb[n * Q0 + (q < Q0 ? q : 0)];
      vz[m] = q < Q0 ? z0 : 0.0;
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
    for (int r = 0; r < rows; ++r) {
      const double rhs = template_value(sx[r][0], P, invP, t0, hw, tau), rd = sx[r][1];
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < JR; ++i) {
        const double fa = sp[r][i] * fma(sw[r][i], z, f[i]);   // :140, :143
        f[i] = fa;
        acc[i & 3] = fma(fa, su[r][i], acc[i & 3]);
      }
      z = rhs - ((acc[0] + acc[1]) + (acc[2] + acc[3]));       // :144
      const double zd = z * rd;
      Tsq = fma(z, zd, Tsq);
#pragma unroll
      for (int q = 0; q < QR; ++q) T0[q] = fma(zd, sz[r][q], T0[q]);
    }
  }

  if (k < K) {
    double *Tb = T + (b * K + k) * (1 + Q0);
    Tb[0] = Tsq;
#pragma unroll
    for (int q = 0; q < QR; ++q)
      if (q < Q0) Tb[1 + q] = T0[q];
  }
}

inline int padded(int64_t n) { return n <= 4 ? 4 : group_size(n); }   // 4, 8, 16 or 32 (as c2_periodogram.hip's)

// f(std::integral_constant<int, R>{}) for R = padded(n); f(... group_size(n)) for the columns of Z0 (1, 2, 4 or 8)
template <class Fn>
inline void dispatch_padded(int64_t n, Fn &&f) {
  switch (padded(n)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}
template <class Fn>
inline void dispatch_columns(int64_t n, Fn &&f) {
  switch (group_size(n)) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

}  // namespace transit
}  // namespace c2

using namespace c2;
using namespace c2::transit;

extern "C" int c2_whitened_transits(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                                    const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                    const double *Z0, const double *trials, int64_t tr_bs, double *T, c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1 || Q0 < 1 || K < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || Q0 > kMaxQ0) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !Z0 || !trials || !T) return C2_ERR_INVALID;
  if (t_bs < 0 || c_bs < 0 || tr_bs < 0) return C2_ERR_INVALID;
  const int64_t KB = (K + kWave - 1) / kWave;
  if (KB > 0x7fffffffLL || B > 0x7fffffffLL / KB) return C2_ERR_UNSUPPORTED;   // 2^31 blocks or more
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * KB));
  dispatch_padded(J, [&](auto jr) {
    dispatch_columns(Q0, [&](auto qr) {
      hipLaunchKernelGGL((k_transits<decltype(jr)::value, decltype(qr)::value>), grid, dim3(kWave), 0, s, N, (int)J, (int)Q0, K,
                         KB, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T);
    });
  });
  return launch_ok();
}
