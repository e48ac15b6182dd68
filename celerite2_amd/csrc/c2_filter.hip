// c2_filter.hip -- STREAMING UPDATES of a factored GP (include/celerite2_amd_filter.h): append rows to a series, absorb rows of
// an existing factorisation, or forecast from the state, in O(M J^2) per series and without the old rows.  No counterpart
// in the reference, whose factor and solve_lower (forward.hpp:69-135, 156-170) always start at row 0.
//
// Everything rows 0 .. n-1 contribute to row n passes through the symmetric J x J state S of factor and the J-vector F of
// solve_lower.  Kept UNPROPAGATED behind the last row (its own contribution included),
//   S = sum_k d_k (e_k o w_k)(e_k o w_k)^T,   F = sum_k (e_k o w_k) z_k,   e_k = exp(-c (t_last - t_k)),
// one row (t, a, u, v, y) with p = exp(-c (t - t_last)) (p := 0 for the first row of a series: S = F = 0 there, and a
// t_last far above t would give 0 * inf) costs
//   S <- (p p^T) o S ;  F <- p o F
//   g = S u ;  d = a - u^T g ;  w = (v - g) / d ;  z = y - u^T F          (forward.hpp:126-133, :168)
//   S <- S + d w w^T ;  F <- F + w z                                       (:119-123, :166)
// Three modes of that body: kAppend runs all of it, kAbsorb reads d, w, z and applies the decay and the update line only,
// kForecast changes nothing and gives mu = u^T (p o F), var = a - u^T ((p p^T) o S) u per query row.
//
// Mapping: as k_invdiag_group (c2_invdiag.hip) -- a GROUP of G lanes per series, lane j owns column j of S (= row j: S is
// symmetric, so g_j is a lane-local dot product against u, which the group shares through LDS); u^T g and u^T F are one
// interleaved DPP butterfly (gsum2).  The two products that change S are symmetric in (i, j) -- (p_i p_j) S_ij and
// (w_i w_j) d -- so lanes i and j compute S_ij with the same bits.  A series' J^2 + J doubles are one contiguous run that the
// group reads once and writes once; the rows are read as they come (M is small: a night's observations).  The state is
// written only at the end and only by a series that took rows and did not fail, so state_out may be state_in.
// No atomics: two calls give identical bits.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_filter.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace c2 {
namespace filter {

enum Mode { kAppend = 0, kAbsorb = 1, kForecast = 2 };
constexpr int kHead = 4;   // t_last, n, sum log d, sum z^2 / d in front of F and S

// x0, X1, X2, x3 / o0, O1, o2 by mode:  kAppend a, U, V, y / d, W, z;  kAbsorb d, W, -, z / -;  kForecast a, U, -, - / mu, -, var
template <int G, int MODE>
__global__ __launch_bounds__(kWave) void k_filter(int64_t B, int M, int J, const double *sin, double *sout,
                                                  const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                  int64_t c_bs, const double *__restrict__ x0, const double *__restrict__ X1,
                                                  const double *__restrict__ X2, const double *__restrict__ x3,
                                                  const int32_t *__restrict__ count, double *__restrict__ o0,
                                                  double *__restrict__ O1, double *__restrict__ o2, int32_t *__restrict__ flag) {
  // No contraction of a product with a later sum: every fma below is written out.  Contracted, the butterfly's first level
  // becomes fma(u_0, g_0, u_1 g_1) in one lane and fma(u_1, g_1, u_0 g_0) in its partner, the lanes of a group disagree
  // on d in the last bit, and S[i,j] == S[j,i] no longer holds to the bit.
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sp[kWave], su[kWave], sw[kWave];
  const Geo<G> L(B, J);
  const int j = L.j, g0 = (L.lane / G) * G;
  const bool act = L.act;
  const int64_t SW = kHead + J + (int64_t)J * J;
  const double *si = sin + L.b * SW;
  const double *tb = t + L.b * t_bs;
  const int64_t r0 = L.b * M;   // first row of this series in the (B, M) arrays
  const double cj = act ? c[L.b * c_bs + L.jj] : 0.0;   // (an idle lane reads column 0 and drops it, here and below)
  int cnt = count ? count[L.b] : M;
  cnt = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  int top = cnt;   // the longest series of this wavefront
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int x = __shfl_xor(top, o, kWave);
    top = x > top ? x : top;
  }

  double tl = si[0], nn = si[1], ld = si[2], qq = si[3];
  const double f0 = si[kHead + L.jj];
  double F = act ? f0 : 0.0;
  const double *srow = si + kHead + J + L.jj * J;   // row j of S = its column j
  double Sc[G];
#pragma unroll
  for (int i = 0; i < G; ++i) {   // (every load is issued, none behind a branch of its own: padding re-reads element 0)
    const double x = srow[i < J ? i : 0];
    Sc[i] = (act && i < J) ? x : 0.0;
  }
  bool empty = nn == 0.0;
  int fail = 0;

  for (int m = 0; m < top; ++m) {
    if (m < cnt && fail == 0) {   // (uniform over the group)
      const double tm = tb[m];
      double p = empty ? 0.0 : exp_decay(cj * (tl - tm));
      p = act ? p : 0.0;
      if constexpr (MODE == kAppend) {
        const double am = x0[r0 + m], ym = x3[r0 + m];
        const double ux = X1[(r0 + m) * J + L.jj], vx = X2[(r0 + m) * J + L.jj];
        const double um = act ? ux : 0.0, vm = act ? vx : 0.0;
        sp[L.lane] = p; su[L.lane] = um;
        lds_order();
        F = p * F;
        double g = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          Sc[i] = (sp[g0 + i] * p) * Sc[i];
          g = fma(Sc[i], su[g0 + i], g);
        }
        double s = g * um, r = um * F;
        gsum2<G>(s, r);
        const double dm = am - s, zm = ym - r;
        if (L.valid && j == 0) o0[r0 + m] = dm;
        if (dm <= 0.0) {   // (a NaN pivot passes)
          fail = m + 1;
        } else {
          const double rd = rcp_nr(dm);
          const double w = (vm - g) * rd;
          sw[L.lane] = w;
          lds_order();
#pragma unroll
          for (int i = 0; i < G; ++i) Sc[i] = fma(sw[g0 + i] * w, dm, Sc[i]);
          F = fma(w, zm, F);
          ld += log(dm);
          qq = fma(zm * zm, rd, qq);
          tl = tm; nn += 1.0; empty = false;
          if (L.valid) {
            if (act) O1[(r0 + m) * J + j] = w;
            if (j == 0) o2[r0 + m] = zm;
          }
        }
      } else if constexpr (MODE == kAbsorb) {
        const double dm = x0[r0 + m], zm = x3[r0 + m];
        const double wx = X1[(r0 + m) * J + L.jj];
        const double w = act ? wx : 0.0;
        sp[L.lane] = p; sw[L.lane] = w;
        lds_order();
#pragma unroll
        for (int i = 0; i < G; ++i) Sc[i] = fma(sw[g0 + i] * w, dm, (sp[g0 + i] * p) * Sc[i]);
        F = fma(w, zm, p * F);
        ld += log(dm);
        qq = fma(zm * zm, rcp_nr(dm), qq);
        tl = tm; nn += 1.0; empty = false;
      } else {
        const double am = x0[r0 + m];
        const double ux = X1[(r0 + m) * J + L.jj];
        const double x = act ? p * ux : 0.0;
        su[L.lane] = x;
        lds_order();
        double h = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) h = fma(Sc[i], su[g0 + i], h);
        double s = x * h, r = x * F;
        gsum2<G>(s, r);
        if (L.valid && j == 0) { o0[r0 + m] = r; o2[r0 + m] = am - s; }
      }
      lds_order();   // (the next row overwrites the vectors)
    }
  }

  if constexpr (MODE != kForecast) {
    if (L.valid) {
      double *so = sout + L.b * SW;
      if (cnt > 0 && fail == 0) {
        if (j == 0) { so[0] = tl; so[1] = nn; so[2] = ld; so[3] = qq; }
        if (act) {
          so[kHead + j] = F;
#pragma unroll
          for (int i = 0; i < G; ++i)
            if (i < J) so[kHead + J + j * J + i] = Sc[i];
        }
      } else if (so != si) {   // nothing taken, or failed: the state as on entry
        if (j == 0) { so[0] = si[0]; so[1] = si[1]; so[2] = si[2]; so[3] = si[3]; }
        if (act) {
          so[kHead + j] = si[kHead + j];
          for (int i = 0; i < J; ++i) so[kHead + J + j * J + i] = si[kHead + J + j * J + i];
        }
      }
      if constexpr (MODE == kAppend) {
        if (j == 0) flag[L.b] = fail;
      }
    }
  }
}

template <int MODE>
inline int launch(int64_t B, int64_t M, int64_t J, const double *sin, double *sout, const double *t, int64_t t_bs,
                  const double *c, int64_t c_bs, const double *x0, const double *X1, const double *X2, const double *x3,
                  const int32_t *count, double *o0, double *O1, double *o2, int32_t *flag, bool missing,
                  c2_stream_t stream) {   // missing: a null among the pointers only this mode takes
  if (B < 1 || M < 1 || J < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || M > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  if (missing || !sin || !t || !c || !x0 || !X1) return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((k_filter<G, MODE>), dim3((unsigned)((B * G + kWave - 1) / kWave)), dim3(kWave), 0, s, B, (int)M, (int)J,
                       sin, sout, t, t_bs, c, c_bs, x0, X1, X2, x3, count, o0, O1, o2, flag);
  });
  return launch_ok();
}

}  // namespace filter
}  // namespace c2

using namespace c2;
using namespace c2::filter;

extern "C" int64_t c2_filter_state_words(int64_t J) { return J < 1 || J > C2_FAST_WIDTH ? 0 : kHead + J + J * J; }

extern "C" int c2_filter_append(int64_t B, int64_t M, int64_t J, const double *state_in, double *state_out, const double *t,
                                int64_t t_bs, const double *c, int64_t c_bs, const double *a, const double *U, const double *V,
                                const double *y, const int32_t *count, double *d, double *W, double *z, int32_t *flag,
                                c2_stream_t stream) {
  return launch<kAppend>(B, M, J, state_in, state_out, t, t_bs, c, c_bs, a, U, V, y, count, d, W, z, flag,
                         !state_out || !V || !y || !d || !W || !z || !flag, stream);
}

extern "C" int c2_filter_absorb(int64_t B, int64_t M, int64_t J, const double *state_in, double *state_out, const double *t,
                                int64_t t_bs, const double *c, int64_t c_bs, const double *W, const double *d, const double *z,
                                const int32_t *count, c2_stream_t stream) {
  return launch<kAbsorb>(B, M, J, state_in, state_out, t, t_bs, c, c_bs, d, W, nullptr, z, count, nullptr, nullptr, nullptr,
                         nullptr, !state_out || !z, stream);
}

extern "C" int c2_filter_forecast(int64_t B, int64_t M, int64_t J, const double *state, const double *t, int64_t t_bs,
                                  const double *c, int64_t c_bs, const double *a, const double *U, const int32_t *count,
                                  double *mu, double *var, c2_stream_t stream) {
  return launch<kForecast>(B, M, J, state, nullptr, t, t_bs, c, c_bs, a, U, nullptr, nullptr, count, mu, nullptr, var, nullptr,
                           !mu || !var, stream);
}
