// c2_filter_draw.hip -- FORECAST SAMPLE PATHS (include/celerite2_amd_filter_draw.h): K joint draws of M future rows from a
// filter state, in O(M (J^2 + J K)) per series and without the old rows.  No counterpart in the reference, whose draws
// (terms.hpp / the Python GaussianProcess.sample) start from the whole series.
//
// Drawing the rows one after the other is the append of c2_filter.hip run backwards in y.  Per row, after the decay,
//   g = S u ;  d = a - u^T g ;  w = (v - g) / d                                  (shared by the draws: no y in them)
//   z_k = sqrt(d) eps_k ;  y_k = u^T F_k + z_k ;  F_k <- F_k + w z_k             (per draw k)
//   S <- S + d w w^T
// The S path is k_filter<G, kAppend>'s, statement for statement: a GROUP of G lanes per series, lane j owns column j of S,
// p, u and w go through LDS.  d and flag therefore have the append's bits.  (The statements are repeated here, not shared
// through a device function: routed through one, k_filter's own code came out scheduled differently, and that kernel is
// to stay as it is.  tests/test_gpu_filter_draw.py holds the two together bit for bit.)
//
// F per draw: the LANES OF THE GROUP OWN DRAWS.  Lane j keeps the whole F (G doubles, zeros behind J) of the draws
// k = j, j + G, j + 2 G, ... of its pass, 32 / G of them, so a pass carries kChunk = 32 draws in 64 registers from J = 2
// on (16 draws at J = 1: slots() below).  u^T F_k is then lane-local -- G fmas in index order, against the p, u and w the S path left in LDS -- and no
// draw's arithmetic depends on the slot or the lane that holds it, nor on K.  (Keeping F_k[j] in lane j instead costs a
// butterfly of 2 log2 G DPP moves and log2 G additions per draw on all G lanes: profiles/filter_draw.md.)  The G lanes of a
// group read and write G consecutive doubles of eps and paths.  Draws beyond a pass go to grid.y; every y-block repeats the
// S path (J^2 per row against J per draw) and block y = 0 alone writes d and flag.  sqrt is the correctly rounded
// one.  No atomics: two calls give identical bits.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd_filter_draw.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace c2 {
namespace filter_draw {

constexpr int kHead = 4;            // t_last, n, sum log d, sum z^2 / d in front of F and S (celerite2_amd_filter.h)
constexpr int kChunk = 32;          // draws of one pass: G lanes x (kChunk / G) slots
constexpr int kMaxPasses = 65535;   // grid.y
// Draws a lane keeps: kChunk over the G lanes of a group, and at most 16 (one lane per series: 32 slots' addresses and store
// masks no longer fit the scalar registers).  A pass carries G * slots(G) draws: 16 at J = 1, 32 from there on.
constexpr int slots(int G) { return kChunk / G > 16 ? 16 : kChunk / G; }

// As in c2_filter_rev.hip: from G = 16 on the scheduler is held every 8 elements of a loop over the group's LDS vectors, so
// that the reads of a whole loop are not issued ahead of the arithmetic on top of the two register columns a lane keeps.
template <int G>
__device__ __forceinline__ void chunk_end(int i) {
  if constexpr (G > 8) {
    if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
  }
}

template <int G>
__global__ __launch_bounds__(kWave) void k_filter_draw(int64_t B, int M, int J, int K, const double *__restrict__ state,
                                                       const double *__restrict__ t, int64_t t_bs, const double *__restrict__ c,
                                                       int64_t c_bs, const double *__restrict__ a, const double *__restrict__ U,
                                                       const double *__restrict__ V, const double *__restrict__ eps,
                                                       const int32_t *__restrict__ count, double *__restrict__ paths,
                                                       double *__restrict__ d, int32_t *__restrict__ flag) {
#pragma clang fp contract(off)   // (as k_filter: the lanes of a group must agree on d to the bit)
  constexpr int KB = slots(G);   // draws a lane keeps
  __shared__ __attribute__((aligned(16))) double sp[kWave], su[kWave], sw[kWave];
  const Geo<G> L(B, J);
  const int j = L.j, g0 = (L.lane / G) * G;
  const bool act = L.act;
  const int64_t SW = kHead + J + (int64_t)J * J;
  const double *si = state + L.b * SW;
  const double *tb = t + L.b * t_bs;
  const int64_t r0 = L.b * M;   // first row of this series in the (B, M) arrays
  const double cj = act ? c[L.b * c_bs + L.jj] : 0.0;
  const bool first = blockIdx.y == 0;   // the pass that writes d and flag
  const int k0 = (int)blockIdx.y * (KB * G) + j;   // slot s of this lane holds draw k0 + s G
  const int left = L.valid ? K - k0 : 0;         // ... and stores it when s G < left
  int cnt = count ? count[L.b] : M;
  cnt = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  int top = cnt;   // the longest series of this wavefront
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int x = __shfl_xor(top, o, kWave);
    top = x > top ? x : top;
  }

  double tl = si[0];
  bool empty = si[1] == 0.0;
  const double *srow = si + kHead + J + L.jj * J;   // row j of S = its column j
  double Sc[G], Fk[KB][G];
#pragma unroll
  for (int i = 0; i < G; ++i) {   // (every load is issued, none behind a branch of its own: padding re-reads element 0)
    const double x = srow[i < J ? i : 0], f = si[kHead + (i < J ? i : 0)];
    Sc[i] = (act && i < J) ? x : 0.0;
#pragma unroll
    for (int s = 0; s < KB; ++s) Fk[s][i] = i < J ? f : 0.0;   // (an idle lane of the group owns draws too)
  }
  int fail = 0;

  for (int m = 0; m < top; ++m) {
    if (m < cnt && fail == 0) {   // (uniform over the group)
      const double tm = tb[m];
      double p = empty ? 0.0 : exp_decay(cj * (tl - tm));
      p = act ? p : 0.0;
      const double am = a[r0 + m];
      const double ux = U[(r0 + m) * J + L.jj], vx = V[(r0 + m) * J + L.jj];
      const double um = act ? ux : 0.0, vm = act ? vx : 0.0;
      const int64_t e0 = (r0 + m) * K;
      double e[KB];
#pragma unroll
      for (int s = 0; s < KB; ++s) {   // (issued ahead of the S path; a slot beyond K re-reads draw K - 1 and is never stored)
        const int k = k0 + s * G;
        e[s] = eps[e0 + (k < K ? k : K - 1)];
      }
      // -- the S path: k_filter<G, kAppend>'s statements, in its order (u^T g alone is gsum's: gsum2's additions) --
      sp[L.lane] = p; su[L.lane] = um;
      lds_order();
      double g = 0.0;
#pragma unroll
      for (int i = 0; i < G; ++i) {
        Sc[i] = (sp[g0 + i] * p) * Sc[i];
        g = fma(Sc[i], su[g0 + i], g);
      }
      const double dm = am - gsum<G>(g * um);
      if (first && L.valid && j == 0) d[r0 + m] = dm;
      if (dm <= 0.0) {   // (a NaN pivot passes)
        fail = m + 1;
      } else {
        const double rd = rcp_nr(dm);
        const double w = (vm - g) * rd;
        sw[L.lane] = w;
        lds_order();
#pragma unroll
        for (int i = 0; i < G; ++i) Sc[i] = fma(sw[g0 + i] * w, dm, Sc[i]);
        // -- the draws of this lane --
        if constexpr (G > 8) asm volatile("" ::: "memory");   // (re-read p and u: kept from the S path they cost 2 G registers)
        const double sd = __dsqrt_rn(dm);
        double r[KB];
#pragma unroll
        for (int s = 0; s < KB; ++s) r[s] = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const double pi = sp[g0 + i], ui = su[g0 + i];
#pragma unroll
          for (int s = 0; s < KB; ++s) {
            Fk[s][i] = pi * Fk[s][i];
            r[s] = fma(ui, Fk[s][i], r[s]);
          }
          chunk_end<G>(i);
        }
        int lm = left;  // (opaque per row: hoisted out of the row loop, the KB store masks do not fit the scalar registers)
        asm volatile("" : "+v"(lm));
#pragma unroll
        for (int s = 0; s < KB; ++s) {
          e[s] = sd * e[s];   // z_k
          double y = r[s] + e[s];
          if constexpr (G > 8) asm volatile("" : "+v"(y));   // (else u^T F_k sinks into the store's branch and holds u until there)
          if (s * G < lm) paths[e0 + k0 + s * G] = y;
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const double wi = sw[g0 + i];
#pragma unroll
          for (int s = 0; s < KB; ++s) Fk[s][i] = fma(wi, e[s], Fk[s][i]);
          chunk_end<G>(i);
        }
        tl = tm; empty = false;
      }
      lds_order();   // (the next row overwrites the vectors)
    }
  }
  if (first && L.valid && j == 0) flag[L.b] = fail;
}

}  // namespace filter_draw
}  // namespace c2

using namespace c2;
using namespace c2::filter_draw;

static int64_t chunk(int64_t J) { return (int64_t)group_size(J) * slots(group_size(J)); }

extern "C" int64_t c2_filter_draw_chunk(int64_t J) { return J < 1 || J > C2_FAST_WIDTH ? 0 : chunk(J); }

extern "C" int c2_filter_draw(int64_t B, int64_t M, int64_t J, int64_t K, const double *state, const double *t, int64_t t_bs,
                              const double *c, int64_t c_bs, const double *a, const double *U, const double *V,
                              const double *eps, const int32_t *count, double *paths, double *d, int32_t *flag,
                              c2_stream_t stream) {
  if (B < 1 || M < 1 || J < 1 || K < 1) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || M > 0x7fffffffLL || K > kMaxPasses * chunk(J)) return C2_ERR_UNSUPPORTED;
  if (!state || !t || !c || !a || !U || !V || !eps || !paths || !d || !flag) return C2_ERR_INVALID;
  const int64_t gx = (B * group_size(J) + kWave - 1) / kWave, gy = (K + chunk(J) - 1) / chunk(J);
  if (gx > 0x7fffffffLL || gx * gy > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((k_filter_draw<G>), dim3((unsigned)gx, (unsigned)gy), dim3(kWave), 0, s, B, (int)M, (int)J, (int)K, state,
                       t, t_bs, c, c_bs, a, U, V, eps, count, paths, d, flag);
  });
  return launch_ok();
}
