// c2_shape_column.hpp -- THE COLUMN OF A TABULATED-SHAPE TRIAL as a lane forms it in registers: the rule of
// include/celerite2_amd_shapes.h, stated once and shared by the sweep that whitens the column (c2_shapes.hip) and by the
// projection of null draws onto it (c2_shape_project.hip), so that both see the same column values bit for bit.
// tests/shapes_ref.py restates it.  The fold and the in / out decision (x, q, phi, u) are transit::template_value's lines
// (c2_trial_columns.hpp), restated here so that that file's text stays as it is.
//
// THE BANK IS READ THROUGH THE VECTOR CACHE, not staged in LDS: a bank at the cap (1024 doubles, 8 KB; 16 KB as (value,
// difference) pairs) next to the 13.5 KB of staged rows of a one-wave block would take the blocks per compute unit from 11
// to 5 at J = 32 (DESIGN.md 5n has the table); 8 KB shared by every wavefront of a series stays in the cache.  The two nodes
// are adjacent doubles.  The gather is skipped, wave-uniformly, at a row where no lane is in an event; what a lane computes
// does not depend on which lanes share its wavefront.
#pragma once
#include <hip/hip_runtime.h>

#include "c2_common.hpp"

namespace c2 {
namespace shape {

constexpr int kMaxNodes = 1024;   // NS * S of a bank (the header's limit)

// what a lane keeps of its trial and of the bank, formed once before the walk
struct Trial {
  double P, invP, t0, hw, ginv, top;   // invP = fl(1 / P) or 0; hw = 0.5 w (exact); ginv = fl(fl(S - 1) / w); top = fl(S - 1)
  const double *node;                  // shape[is]: the clamped index, never a trusted one
  int last;                            // S - 2: the last interval
};

// (P, t0, w, s) of a live lane, the null trial (0, 0, 0, 0) otherwise.  `bank`: this series' (NS, S) doubles.
__device__ __forceinline__ Trial make_trial(const double *tr, bool live, const double *bank, int NS, int S) {
#pragma clang fp contract(off)
  Trial T;
  const double w = live ? tr[2] : 0.0, s = live ? tr[3] : 0.0;
  T.P = live ? tr[0] : 0.0;
  T.t0 = live ? tr[1] : 0.0;
  T.invP = T.P != 0.0 ? 1.0 / T.P : 0.0;                     // (a correctly rounded division, once per lane)
  T.hw = 0.5 * w;
  T.top = (double)(S - 1);
  T.ginv = T.top / w;                                        // (correctly rounded; w == 0: inf, w NaN: NaN -- g then takes 0)
  const int is = (s >= 0.0 && s < (double)NS) ? (int)s : 0;  // (NaN fails both comparisons)
  T.node = bank + (int64_t)is * S;
  T.last = S - 2;
  return T;
}

// b_n of the header's rule.  Whatever the trial holds, the two reads are node[i], node[i + 1] with 0 <= i <= S - 2.
__device__ __forceinline__ double value(const Trial &T, double t) {
#pragma clang fp contract(off)
  const double x = t - T.t0;
  const double q = __builtin_rint(x * T.invP);
  const double qp = q * T.P;
  const double phi = x - qp;
  const double u = T.hw - __builtin_fabs(phi);
  const double v = phi + T.hw;
  double g = v * T.ginv;
  g = g > 0.0 ? g : 0.0;                                     // (a NaN g takes 0)
  g = g < T.top ? g : T.top;
  const int fl = (int)__builtin_floor(g);
  const int i = fl < T.last ? fl : T.last;
  const double fr = g - (double)i;                           // (exact)
  const bool in = !(u < 0.0);
  double a = 0.0, c = 0.0;
  if (__builtin_amdgcn_ballot_w64(in) != 0) {                // (wave-uniform: the loads are skipped, not masked)
    a = T.node[i];
    c = T.node[i + 1];
  }
  const double dlt = c - a;
  const double fd = fr * dlt;
  const double b = a + fd;
  return in ? b : 0.0;
}

}  // namespace shape
}  // namespace c2
