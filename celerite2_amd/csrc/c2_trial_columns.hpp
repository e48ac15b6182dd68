// c2_trial_columns.hpp -- THE COLUMNS OF A TRIAL as a lane forms them in registers: the periodogram's phase, the transit
// template and the Keplerian pair.  One statement of each rule, shared by the sweeps that whiten the columns
// (c2_periodogram.hip, c2_transit.hip, c2_kepler.hip) and by the projection of null draws onto them (c2_trial_project.hip),
// so that both see the same column values bit for bit.  The public headers (celerite2_amd_periodogram.h, _transit.h,
// _kepler.h) state the rules line by line; tests/periodogram_ref.py, tests/transit_ref.py and tests/kepler_ref.py restate them.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace pgram

namespace transit {

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

}  // namespace transit

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
}  // namespace c2
