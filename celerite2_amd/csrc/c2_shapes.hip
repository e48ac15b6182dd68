// c2_shapes.hip -- the WHITENED TABULATED SHAPES of a trial grid under the factored covariance (c2_whitened_shapes,
// include/celerite2_amd_shapes.h): for every series b and trial k = (period P, epoch t0, width w, shape index s), with d, W
// of c2_factor, Z0 = L^-1 [A0 | y - mean] (B, N, Q0) of c2_solve_lower and a bank of NS event profiles tabulated on S nodes,
//   z = L^-1 b_k(t),   <a, b> = sum_n a_n b_n / d_n,   T[b, k, :] = [<z, z>, <z, Z0[:, j]> (j < Q0)]
// in ONE forward sweep that forms b_k in registers -- the profile interpolated linearly between its two nodes around the
// sample -- and writes neither it nor z: what least squares with a limb-darkened transit, a flare or a measured template
// under correlated noise reads (celerite2_amd/shapes.py).  No counterpart in the reference.
//
// The recurrence is internal::forward (internal.hpp:107-146) as restated in c2_gram.hip, with one right-hand side:
//   f <- p_n o (f + w_{n-1} z_{n-1})        (f: J, zero at row 0; p_n = exp(-c (t_n - t_{n-1})); :139-143)
//   z_n = b_n - f^T u_n                     (:144)
// THE COLUMN is the header's rule, every line rounded once and none contracted into an fma (shape::value,
// c2_shape_column.hpp), so a numpy restatement takes the same discrete decisions bit for bit.
//
// k_shapes<JR, QR> (JR: J rounded up to 4, 8, 16 or 32; QR: Q0 rounded up to 1, 2, 4 or 8) is k_transits' sibling
// (c2_transit.hip): ONE LANE PER TRIAL at every width, rows staged through LDS, R = 16 rows a block, by trial::sweep_rows
// (c2_trial_sweep.hpp), the row body's recurrence statements those of k_transits in the same order.  A lane holds f (JR
// registers), its trial (shape::Trial) and the 1 + QR sums.  The bank is not staged: a lane in an event gathers its two
// nodes, adjacent doubles, through the vector cache (c2_shape_column.hpp says why).  Lanes with k >= K carry the null trial
// (0, 0, 0, 0) and store nothing.  Every element of T is written by exactly one lane: no atomics, two calls give identical
// bits.  Blocks: B * ceil(K / 64) in grid.x, the trial blocks of a series next to each other.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_shapes.h"
#include "c2_launch.hpp"
#include "c2_shape_column.hpp"
#include "c2_trial_sweep.hpp"

namespace c2 {
namespace shape {

template <int JR, int QR>
__global__ __launch_bounds__(kWave) void k_shapes(int64_t N, int J, int Q0, int64_t K, int64_t KB,
                                                  const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                  int64_t c_bs, const double *__restrict__ U, const double *__restrict__ W,
                                                  const double *__restrict__ d, const double *__restrict__ Z0,
                                                  const double *__restrict__ trials, int64_t tr_bs, double *__restrict__ T,
                                                  const double *__restrict__ shapes, int64_t sh_bs, int NS, int S) {
  constexpr int R = 16;                                     // rows per staged block
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / KB, k = (blockIdx.x % KB) * kWave + lane;
  const Trial tr = make_trial(trials + b * tr_bs + (k < K ? k : 0) * 4, k < K, shapes + b * sh_bs, NS, S);

  double f[JR], T0[QR], Tsq = 0.0, z = 0.0;
#pragma unroll
  for (int i = 0; i < JR; ++i) f[i] = 0.0;
#pragma unroll
  for (int q = 0; q < QR; ++q) T0[q] = 0.0;

  // one row: sx = (t_n, 1 / d_n) and the staged LDS rows p_n, w_{n-1}, u_n, Z0[n]
  auto row = [&](const double *sx, const double *sp, const double *sw, const double *su, const double *sz) {
    const double rhs = value(tr, sx[0]), rd = sx[1];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < JR; ++i) {
      const double fa = sp[i] * fma(sw[i], z, f[i]);   // :140, :143
      f[i] = fa;
      acc[i & 3] = fma(fa, su[i], acc[i & 3]);
    }
    z = rhs - ((acc[0] + acc[1]) + (acc[2] + acc[3]));       // :144
    const double zd = z * rd;
    Tsq = fma(z, zd, Tsq);
#pragma unroll
    for (int q = 0; q < QR; ++q) T0[q] = fma(zd, sz[q], T0[q]);
  };
  trial::sweep_rows<JR, QR, R>(N, J, Q0, b, t, t_bs, c, c_bs, U, W, d, Z0, row);

  if (k < K) {
    double *Tb = T + (b * K + k) * (1 + Q0);
    Tb[0] = Tsq;
#pragma unroll
    for (int q = 0; q < QR; ++q)
      if (q < Q0) Tb[1 + q] = T0[q];
  }
}

}  // namespace shape
}  // namespace c2

using namespace c2;
using namespace c2::shape;

extern "C" int c2_whitened_shapes(int64_t B, int64_t N, int64_t J, int64_t Q0, int64_t K, const double *t, int64_t t_bs,
                                  const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                                  const double *Z0, const double *trials, int64_t tr_bs, double *T, const double *shapes,
                                  int64_t sh_bs, int64_t NS, int64_t S, c2_stream_t stream) {
  if (B < 1 || N < 1 || J < 1 || Q0 < 1 || K < 1 || NS < 1 || S < 2) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || Q0 > trial::kMaxQ0) return C2_ERR_UNSUPPORTED;
  if (NS > kMaxNodes || S > kMaxNodes || NS * S > kMaxNodes) return C2_ERR_UNSUPPORTED;
  if (!t || !c || !U || !W || !d || !Z0 || !trials || !T || !shapes) return C2_ERR_INVALID;
  if (t_bs < 0 || c_bs < 0 || tr_bs < 0 || (sh_bs != 0 && sh_bs != NS * S)) return C2_ERR_INVALID;
  const int64_t KB = (K + kWave - 1) / kWave;
  if (KB > 0x7fffffffLL || B > 0x7fffffffLL / KB) return C2_ERR_UNSUPPORTED;   // 2^31 blocks or more
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(B * KB));
  dispatch_padded(J, [&](auto jr) {
    dispatch_columns(Q0, [&](auto qr) {
      hipLaunchKernelGGL((k_shapes<decltype(jr)::value, decltype(qr)::value>), grid, dim3(kWave), 0, s, N, (int)J, (int)Q0, K,
                         KB, t, t_bs, c, c_bs, U, W, d, Z0, trials, tr_bs, T, shapes, sh_bs, (int)NS, (int)S);
    });
  });
  return launch_ok();
}
