// c2_trial_columns.hpp -- THE COLUMNS OF A TRIAL as a lane forms them in registers, one COLUMN SOURCE per kind of trial
// (namespace trial, at the end): the periodogram's phase, the transit template, the Keplerian pair and the tabulated shape.
// One statement of each rule, shared by the sweep that whitens the columns (k_trial_sweep, c2_trial_sweep.hpp) and by the
// projection of null draws onto them (k_project, c2_trial_project.hip), so that both see the same column values bit for
// bit.  The public headers (celerite2_amd_periodogram.h, _transit.h, _kepler.h, _shapes.h) state the rules line by line;
// tests/periodogram_ref.py, tests/transit_ref.py, tests/kepler_ref.py and tests/shapes_ref.py restate them.
//
// A source states NC (its columns: 1 or 2; 2 H for H harmonics), WORDS (doubles per trial) and Params (what a launch hands
// every lane beside the trials); it is built from (this lane's trial -- trial 0 when the lane is beyond K --, live, the
// series, Params), a lane that is not live taking the INERT trial (all zeros) without reading; columns(t, a[NC]) gives the
// column values at a time.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"

namespace c2 {
namespace pgram {

// x = fl(w * fl(t - t_ref)): the two roundings of the header, kept apart from whatever uses x
__device__ __forceinline__ double phase(double w, double t, double t_ref) {
#pragma clang fp contract(off)
  const double dt = t - t_ref;
  const double x = w * dt;
  return x;
}

// w_h = fl(h * w): harmonic h's frequency (celerite2_amd_harmonics.h), one rounding
__device__ __forceinline__ double harmonic(int h, double w) {
#pragma clang fp contract(off)
  const double wh = (double)h * w;
  return wh;
}

}  // namespace pgram

// THE FOLD of a repeating event, shared by the transit template and the tabulated shape: what a lane keeps of (P, t0, w) --
// invP = fl(1 / P), or 0 for a single event (then q = 0 and phi = x); hw = 0.5 w (exact) -- and the time from the nearest
// event's centre, every line rounded once and none contracted into an fma.
struct Fold {
  double P, invP, t0, hw;
  __device__ __forceinline__ Fold(const double *tr, bool live) : P(live ? tr[0] : 0.0), t0(live ? tr[1] : 0.0), hw(live ? 0.5 * tr[2] : 0.0) {
    invP = P != 0.0 ? 1.0 / P : 0.0;                           // (a correctly rounded division, once per lane)
  }
  __device__ __forceinline__ double phi(double t) const {
#pragma clang fp contract(off)
    const double x = t - t0;
    const double q = __builtin_rint(x * invP);
    const double qp = q * P;
    const double phi = x - qp;
    return phi;
  }
};

namespace kepler {

constexpr double kTwoPi = 0x1.921fb54442d18p+2;    // fl(2 pi)
constexpr double kInvTwoPi = 0x1.45f306dc9c883p-3;   // fl(1 / fl(2 pi))

// what a lane keeps of its trial, formed once before the sweep
struct Trial {
  double w, e, tp, b, se, ce;   // b = sqrt(1 - e^2); se, ce = sin e, cos e (the starter's sin(a + e))
};

__device__ __forceinline__ Trial make_trial(double w, double e, double tp) {
#pragma clang fp contract(off)
  Trial tr;
  tr.w = w; tr.e = e; tr.tp = tp;
  const double ee = e * e;
  tr.b = sqrt(1.0 - ee);
  sincos_cw(e, tr.se, tr.ce);
  return tr;
}

// r of the header's rule: x = fl(w * fl(t - tp)) reduced by the double 2 pi.  The fma is exact (the header says why).
__device__ __forceinline__ double mean_anomaly(double w, double t, double tp) {
#pragma clang fp contract(off)
  const double dt = t - tp;
  const double x = w * dt;
  const double q = __builtin_rint(x * kInvTwoPi);
  return __builtin_fma(-q, kTwoPi, x);
}

// Danby's quartic step of E - e sin E = a at E with (s, c) = (sin E, cos E)
__device__ __forceinline__ double danby(double E, double a, double e, double s, double c) {
#pragma clang fp contract(off)
  const double f = fma(-e, s, E) - a;
  const double f2 = e * s, f3 = e * c, f1 = 1.0 - f3;
  const double d1 = -f * rcp_nr(f1);
  const double d2 = -f * rcp_nr(fma(0.5 * d1, f2, f1));
  return -f * rcp_nr(fma(d2 * d2, f3 * (1.0 / 6.0), fma(0.5 * d2, f2, f1)));
}

// (cos nu, sin nu) at time t: the header's sequence, statement by statement
__device__ __forceinline__ void columns(const Trial &tr, double t, double &cnu, double &snu) {
#pragma clang fp contract(off)
  const double e = tr.e;
  const double r = mean_anomaly(tr.w, t, tr.tp), a = __builtin_fabs(r);
  double s, c, delta;
  sincos_cw_fast(a, s, c);
  const double sae = fma(s, tr.ce, c * tr.se);                      // sin(a + e)
  const double E0 = a + e, E1 = fma(e * s, rcp_nr((1.0 - sae) + s), a);
  double E = E1 < E0 ? E1 : E0;
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    sincos_cw_fast(E, s, c);
    delta = danby(E, a, e, s, c);
    E += delta;
  }
  {  // the pair at the new E by a rotation: delta is below 2e-3 after three steps, the series are exact to rounding
    const double d2 = delta * delta;
    const double sd = delta * fma(d2, fma(d2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
    const double cd = fma(d2, fma(d2, 1.0 / 24.0, -0.5), 1.0);
    const double s1 = fma(s, cd, c * sd), c1 = fma(c, cd, -(s * sd));
    s = s1; c = c1;
  }
  delta = danby(E, a, e, s, c);
  {  // and by the fourth step (below 1e-11: first order)
    const double s1 = fma(c, delta, s), c1 = fma(-s, delta, c);
    s = s1; c = c1;
  }
  const double g = rcp_nr(fma(-e, c, 1.0));
  cnu = (c - e) * g;
  snu = __builtin_copysign(1.0, r) * ((tr.b * s) * g);
}

}  // namespace kepler

namespace trial {

struct NoParams {};

// What a kind's own arguments add to the three stages of an entry point's checks, made in this order by every launcher:
// sizes (C2_ERR_INVALID), limits (C2_ERR_UNSUPPORTED), pointers and strides (C2_ERR_INVALID).
struct KindChecks {
  bool bad_size = false, too_large = false, bad_arg = false;
};

// (w): cos x, sin x at x = fl(w * fl(t - t_ref))
struct Sinusoid {
  static constexpr int NC = 2, WORDS = 1;
  struct Params { double t_ref; };
  double om, t_ref;
  __device__ __forceinline__ Sinusoid(const double *tr, bool live, int64_t, const Params &p) : om(live ? tr[0] : 0.0), t_ref(p.t_ref) {}
  // (a frequency the lane formed itself: harmonic h's fl(h * w) of c2_harmonics.hip)
  __device__ __forceinline__ Sinusoid(double om_, const Params &p) : om(om_), t_ref(p.t_ref) {}
  __device__ __forceinline__ void columns(double t, double (&a)[2]) const { sincos_cw(pgram::phase(om, t, t_ref), a[1], a[0]); }
};

// (w) and H harmonics: the 2 H columns (c_1, s_1, ..., c_H, s_H) of celerite2_amd_harmonics.h -- H Sinusoids at the
// frequencies fl(h w), so harmonic h's pair is, bit for bit, the Sinusoid's pair of a trial that holds fl(h w)
template <int H>
struct Harmonics {
  static constexpr int NC = 2 * H, WORDS = 1;
  typedef Sinusoid::Params Params;
  Sinusoid s[H];
  template <int... I>
  __device__ __forceinline__ Harmonics(double w, const Params &p, std::integer_sequence<int, I...>)
      : s{Sinusoid(pgram::harmonic(I + 1, w), p)...} {}
  __device__ __forceinline__ Harmonics(const double *tr, bool live, int64_t, const Params &p)
      : Harmonics(live ? tr[0] : 0.0, p, std::make_integer_sequence<int, H>{}) {}
  __device__ __forceinline__ void columns(double t, double (&a)[2 * H]) const {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      double pair[2];
      s[h].columns(t, pair);
      a[2 * h] = pair[0];
      a[2 * h + 1] = pair[1];
    }
  }
};

// (P, t0, w, tau): b_n of celerite2_amd_transit.h.  The ramp's division is met only by a wavefront with a lane on an
// ingress or egress at that row.
struct Transit {
  static constexpr int NC = 1, WORDS = 4;
  typedef NoParams Params;
  Fold fold;
  double tau;
  __device__ __forceinline__ Transit(const double *tr, bool live, int64_t, const Params &) : fold(tr, live), tau(live ? tr[3] : 0.0) {}
  // b_n from the folded time.  (By value: as a member reading hw and tau through `this`, the compiler ran the division on
  // every row instead of branching round it.)
  static __device__ __forceinline__ double edge(double phi, double hw, double tau) {
#pragma clang fp contract(off)
    const double u = hw - __builtin_fabs(phi);
    double b = u >= tau ? 1.0 : 0.0;
    const bool ramp = u >= 0.0 && u < tau;
    if (__builtin_amdgcn_ballot_w64(ramp) != 0) b = ramp ? u / tau : b;   // (wave-uniform: the division is skipped, not masked)
    return b;
  }
  __device__ __forceinline__ void columns(double t, double (&a)[1]) const { a[0] = edge(fold.phi(t), fold.hw, tau); }
};

// (w, e, tp): cos nu, sin nu of the orbit
struct Keplerian {
  static constexpr int NC = 2, WORDS = 3;
  typedef NoParams Params;
  kepler::Trial tr;
  __device__ __forceinline__ Keplerian(const double *p, bool live, int64_t, const Params &)
      : tr(kepler::make_trial(live ? p[0] : 0.0, live ? p[1] : 0.0, live ? p[2] : 0.0)) {}
  __device__ __forceinline__ void columns(double t, double (&a)[2]) const { kepler::columns(tr, t, a[0], a[1]); }
};

// (P, t0, w, s) and a bank of NS profiles on S nodes ((NS, S) doubles a series, `stride` apart, 0 when shared): b_n of
// celerite2_amd_shapes.h, the profile interpolated linearly between its two nodes around the sample.
// THE BANK IS READ THROUGH THE VECTOR CACHE, not staged in LDS: a bank at the cap (1024 doubles, 8 KB; 16 KB as (value,
// difference) pairs) next to the 13.5 KB of staged rows of a one-wave block would take the blocks per compute unit from 11
// to 5 at J = 32 (DESIGN.md 5n has the table); 8 KB shared by every wavefront of a series stays in the cache.  The two nodes
// are adjacent doubles.  The gather is skipped, wave-uniformly, at a row where no lane is in an event; what a lane computes
// does not depend on which lanes share its wavefront.
struct Shape {
  static constexpr int NC = 1, WORDS = 4;
  struct Params { const double *bank; int64_t stride; int NS, S; };
  Fold fold;
  double ginv, top;     // ginv = fl(fl(S - 1) / w); top = fl(S - 1)
  const double *node;   // shape[is]: the clamped index, never a trusted one
  int last;             // S - 2: the last interval
  __device__ __forceinline__ Shape(const double *tr, bool live, int64_t b, const Params &p) : fold(tr, live) {
#pragma clang fp contract(off)
    const double w = live ? tr[2] : 0.0, s = live ? tr[3] : 0.0;
    top = (double)(p.S - 1);
    ginv = top / w;                                                // (correctly rounded; w == 0: inf, w NaN: NaN -- g then takes 0)
    const int is = (s >= 0.0 && s < (double)p.NS) ? (int)s : 0;    // (NaN fails both comparisons)
    node = p.bank + b * p.stride + (int64_t)is * p.S;
    last = p.S - 2;
  }
  // Whatever the trial holds, the two reads are node[i], node[i + 1] with 0 <= i <= S - 2.
  __device__ __forceinline__ void columns(double t, double (&a)[1]) const {
#pragma clang fp contract(off)
    const double phi = fold.phi(t);
    const double u = fold.hw - __builtin_fabs(phi);
    const double v = phi + fold.hw;
    double g = v * ginv;
    g = g > 0.0 ? g : 0.0;                                     // (a NaN g takes 0)
    g = g < top ? g : top;
    const int fl = (int)__builtin_floor(g);
    const int i = fl < last ? fl : last;
    const double fr = g - (double)i;                           // (exact)
    const bool in = !(u < 0.0);
    double lo = 0.0, hi = 0.0;
    if (__builtin_amdgcn_ballot_w64(in) != 0) {                // (wave-uniform: the loads are skipped, not masked)
      lo = node[i];
      hi = node[i + 1];
    }
    const double dlt = hi - lo;
    const double fd = fr * dlt;
    const double b = lo + fd;
    a[0] = in ? b : 0.0;
  }
};

constexpr int kMaxNodes = 1024;   // NS * S of a bank (C2_SHAPE_MAX_NODES)

inline KindChecks bank_checks(const double *shapes, int64_t sh_bs, int64_t NS, int64_t S) {
  return {NS < 1 || S < 2, NS > kMaxNodes || S > kMaxNodes || NS * S > kMaxNodes, !shapes || (sh_bs != 0 && sh_bs != NS * S)};
}

}  // namespace trial
}  // namespace c2
