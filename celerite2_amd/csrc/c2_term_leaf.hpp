// c2_term_leaf.hpp -- the LEAF formulas of the term kernels: parameters -> celerite coefficients of one RealTerm /
// ComplexTerm / SHOTerm / Matern32Term / RotationTerm record (python/celerite2/terms.py:515-521, 554-569, 644-691,
// 729-745, 791-812) and their hand-written reverse.  Shared by c2_term_params.hip (the flat sum of terms) and
// c2_term_expr.hip (sums, products, derivatives and the exposure-time convolution on top of the same leaves), so that
// there is ONE copy of every formula.  The coefficient arrays are reached through an accessor `A` with operator[](int):
// a plain `double *` for the (B, Jr | Jc) rows of the flat program, a strided view of the work buffer for the algebra.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/celerite2_amd.h"

namespace c2leaf {

constexpr double kTwoPi = 6.283185307179586476925286766559;

// ---- SHO, terms.py:658-691 ------------------------------------------------------------------------------------------
// under-damped (Q >= 1/2): one complex term.  f = sqrt(max(4 Q^2 - 1, eps)).
__device__ __forceinline__ void sho_under(double S0, double w0, double Q, double eps, double &a, double &b, double &c,
                                          double &d) {
  const double f = sqrt(fmax(4.0 * Q * Q - 1.0, eps));
  a = S0 * w0 * Q;
  c = 0.5 * w0 / Q;
  b = a / f;
  d = c * f;
}
// cotangents of (ac, bc, cc, dc) -> ADDED to (bS0, bw0, bQ).  Where max(., eps) clamps, nothing flows through f.
__device__ __forceinline__ void sho_under_rev(double S0, double w0, double Q, double eps, double ga, double gb, double gc,
                                              double gd, double &bS0, double &bw0, double &bQ) {
  const double g = 4.0 * Q * Q - 1.0;
  const double f = sqrt(fmax(g, eps));
  const double a = S0 * w0 * Q, c = 0.5 * w0 / Q;
  const double ba = ga + gb / f;
  const double bcv = gc + gd * f;
  const double bf = gd * c - gb * a / (f * f);
  bS0 += ba * w0 * Q;
  bw0 += ba * S0 * Q + bcv * 0.5 / Q;
  bQ += ba * S0 * w0 - bcv * c / Q;
  if (g > eps) bQ += bf * 4.0 * Q / f;
}
// over-damped (Q < 1/2): two real terms.  f = sqrt(max(1 - 4 Q^2, eps)).
__device__ __forceinline__ void sho_over(double S0, double w0, double Q, double eps, double &a0, double &a1, double &c0,
                                         double &c1) {
  const double f = sqrt(fmax(1.0 - 4.0 * Q * Q, eps));
  const double A = 0.5 * S0 * w0 * Q, C = 0.5 * w0 / Q;
  a0 = A * (1.0 + 1.0 / f);
  a1 = A * (1.0 - 1.0 / f);
  c0 = C * (1.0 - f);
  c1 = C * (1.0 + f);
}
__device__ __forceinline__ void sho_over_rev(double S0, double w0, double Q, double eps, double ga0, double ga1, double gc0,
                                             double gc1, double &bS0, double &bw0, double &bQ) {
  const double g = 1.0 - 4.0 * Q * Q;
  const double f = sqrt(fmax(g, eps));
  const double A = 0.5 * S0 * w0 * Q, C = 0.5 * w0 / Q;
  const double bA = ga0 * (1.0 + 1.0 / f) + ga1 * (1.0 - 1.0 / f);
  const double bC = gc0 * (1.0 - f) + gc1 * (1.0 + f);
  const double bf = A * (ga1 - ga0) / (f * f) + C * (gc1 - gc0);
  bS0 += bA * 0.5 * w0 * Q;
  bw0 += bA * 0.5 * S0 * Q + bC * 0.5 / Q;
  bQ += bA * 0.5 * S0 * w0 - bC * C / Q;
  if (g > eps) bQ -= bf * 4.0 * Q / f;
}

// (S0 | sigma, w0 | rho, Q | tau) -> (S0, w0, Q): the reference's parameter spec, terms.py:644-652.
__device__ __forceinline__ void sho_params(int par, double p0, double p1, double p2, double &S0, double &w0, double &Q) {
  w0 = (par & C2_SHO_RHO) ? kTwoPi / p1 : p1;
  Q = (par & C2_SHO_TAU) ? 0.5 * w0 * p2 : p2;
  S0 = (par & C2_SHO_SIGMA) ? p0 * p0 / (w0 * Q) : p0;
}
// (bS0, bw0, bQ) -> cotangents of the three parameters as given: sigma -> S0 depends on w0 and Q, tau -> Q on w0.
__device__ __forceinline__ void sho_params_rev(int par, double p0, double p1, double p2, double S0, double w0, double Q,
                                               double bS0, double bw0, double bQ, double &g0, double &g1, double &g2) {
  g0 = bS0;
  if (par & C2_SHO_SIGMA) {
    g0 = bS0 * 2.0 * p0 / (w0 * Q);
    bw0 -= bS0 * S0 / w0;
    bQ -= bS0 * S0 / Q;
  }
  g2 = bQ;
  if (par & C2_SHO_TAU) {
    g2 = bQ * 0.5 * w0;
    bw0 += bQ * 0.5 * p2;
  }
  g1 = (par & C2_SHO_RHO) ? -bw0 * w0 / p1 : bw0;
}

// ---- rotation term, terms.py:791-812: two under-damped oscillators at period and period / 2 --------------------------
struct Rot {
  double amp, Q1, g1, w1, S1, Q2, g2, w2, S2;
};
__device__ __forceinline__ Rot rot_params(double sigma, double period, double Q0, double dQ, double f) {
  Rot r;
  r.amp = sigma * sigma / (1.0 + f);
  r.Q1 = 0.5 + Q0 + dQ;
  r.g1 = sqrt(4.0 * r.Q1 * r.Q1 - 1.0);
  r.w1 = 2.0 * kTwoPi * r.Q1 / (period * r.g1);
  r.S1 = r.amp / (r.w1 * r.Q1);
  r.Q2 = 0.5 + Q0;
  r.g2 = sqrt(4.0 * r.Q2 * r.Q2 - 1.0);
  r.w2 = 4.0 * kTwoPi * r.Q2 / (period * r.g2);
  r.S2 = f * r.amp / (r.w2 * r.Q2);
  return r;
}

// One record forward: p = the series' row of P; R0, R1 = (ar, cr), C0 .. C3 = (ac, bc, cc, dc), indexed by coefficient
// slot.  `bad` becomes t + 1 when the series is on the wrong side of the record's SHO regime.
template <class A>
__device__ __forceinline__ void leaf_forward(const c2_term_rec &T, int t, const double *p, A R0, A R1, A C0, A C1, A C2,
                                             A C3, int32_t &bad) {
  const int jr = T.jr, jc = T.jc;
  switch (T.kind) {
    case C2_TERM_REAL:
      R0[jr] = p[T.col[0]];
      R1[jr] = p[T.col[1]];
      break;
    case C2_TERM_COMPLEX:
      C0[jc] = p[T.col[0]];
      C1[jc] = p[T.col[1]];
      C2[jc] = p[T.col[2]];
      C3[jc] = p[T.col[3]];
      break;
    case C2_TERM_SHO: {
      double S0, w0, Q;
      sho_params(T.par, p[T.col[0]], p[T.col[1]], p[T.col[2]], S0, w0, Q);
      const bool over = Q < 0.5;   // terms.py:691
      if (T.regime == C2_SHO_UNDER) {
        if (!(Q >= 0.5)) bad = t + 1;   // (the clamped formula still gives finite coefficients; the wrapper discards them)
        sho_under(S0, w0, Q, T.eps, C0[jc], C1[jc], C2[jc], C3[jc]);
      } else if (T.regime == C2_SHO_OVER) {
        if (!over) bad = t + 1;
        sho_over(S0, w0, Q, T.eps, R0[jr], R0[jr + 1], R1[jr], R1[jr + 1]);
      } else {   // mixed: the side Q selects is filled, the other has zero amplitudes and the finite rate w0 / 2Q
        if (!(Q == Q)) bad = t + 1;
        const double rate = 0.5 * w0 / Q;
        if (over) {
          sho_over(S0, w0, Q, T.eps, R0[jr], R0[jr + 1], R1[jr], R1[jr + 1]);
          C0[jc] = 0.0; C1[jc] = 0.0; C2[jc] = rate; C3[jc] = 0.0;
        } else {
          sho_under(S0, w0, Q, T.eps, C0[jc], C1[jc], C2[jc], C3[jc]);
          R0[jr] = 0.0; R0[jr + 1] = 0.0; R1[jr] = rate; R1[jr + 1] = rate;
        }
      }
      break;
    }
    case C2_TERM_MATERN32: {   // terms.py:729-745
      const double sigma = p[T.col[0]], rho = p[T.col[1]];
      const double w0 = sqrt(3.0) / rho;
      const double S0 = sigma * sigma / w0;
      C0[jc] = w0 * S0;
      C1[jc] = w0 * w0 * S0 / T.eps;
      C2[jc] = w0;
      C3[jc] = T.eps;
      break;
    }
    case C2_TERM_ROTATION: {
      const Rot r = rot_params(p[T.col[0]], p[T.col[1]], p[T.col[2]], p[T.col[3]], p[T.col[4]]);
      if (!(r.Q2 > 0.5) || !(r.Q1 > 0.5)) bad = t + 1;   // (both oscillators under-damped, as the reference's use of the term)
      sho_under(r.S1, r.w1, r.Q1, T.eps, C0[jc], C1[jc], C2[jc], C3[jc]);
      sho_under(r.S2, r.w2, r.Q2, T.eps, C0[jc + 1], C1[jc + 1], C2[jc + 1], C3[jc + 1]);
      break;
    }
  }
}

// One record in reverse: the cotangents of its coefficient slots (R0 .. C3, read only) -> ADDED to the series' row g of bP.
template <class A>
__device__ __forceinline__ void leaf_reverse(const c2_term_rec &T, const double *p, A R0, A R1, A C0, A C1, A C2, A C3,
                                             double *g) {
  const int jr = T.jr, jc = T.jc;
  switch (T.kind) {
    case C2_TERM_REAL:
      g[T.col[0]] += R0[jr];
      g[T.col[1]] += R1[jr];
      break;
    case C2_TERM_COMPLEX:
      g[T.col[0]] += C0[jc];
      g[T.col[1]] += C1[jc];
      g[T.col[2]] += C2[jc];
      g[T.col[3]] += C3[jc];
      break;
    case C2_TERM_SHO: {
      const double p0 = p[T.col[0]], p1 = p[T.col[1]], p2 = p[T.col[2]];
      double S0, w0, Q;
      sho_params(T.par, p0, p1, p2, S0, w0, Q);
      double bS0 = 0.0, bw0 = 0.0, bQ = 0.0;
      const bool under = T.regime == C2_SHO_UNDER || (T.regime == C2_SHO_MIXED && !(Q < 0.5));
      // mixed: the inactive side's cotangents are ignored -- its amplitudes are the constant 0, and its rate cotangents
      // are proportional to those amplitudes
      if (under) sho_under_rev(S0, w0, Q, T.eps, C0[jc], C1[jc], C2[jc], C3[jc], bS0, bw0, bQ);
      else sho_over_rev(S0, w0, Q, T.eps, R0[jr], R0[jr + 1], R1[jr], R1[jr + 1], bS0, bw0, bQ);
      double g0, g1, g2;
      sho_params_rev(T.par, p0, p1, p2, S0, w0, Q, bS0, bw0, bQ, g0, g1, g2);
      g[T.col[0]] += g0;
      g[T.col[1]] += g1;
      g[T.col[2]] += g2;
      break;
    }
    case C2_TERM_MATERN32: {
      const double sigma = p[T.col[0]], rho = p[T.col[1]];
      const double w0 = sqrt(3.0) / rho;
      const double S0 = sigma * sigma / w0;
      const double bS0 = C0[jc] * w0 + C1[jc] * w0 * w0 / T.eps;
      double bw0 = C0[jc] * S0 + C1[jc] * 2.0 * w0 * S0 / T.eps + C2[jc];
      bw0 -= bS0 * S0 / w0;
      g[T.col[0]] += bS0 * 2.0 * sigma / w0;
      g[T.col[1]] -= bw0 * w0 / rho;
      break;
    }
    case C2_TERM_ROTATION: {
      const double sigma = p[T.col[0]], period = p[T.col[1]], f = p[T.col[4]];
      const Rot r = rot_params(sigma, period, p[T.col[2]], p[T.col[3]], f);
      double bS1 = 0.0, bw1 = 0.0, bQ1 = 0.0, bS2 = 0.0, bw2 = 0.0, bQ2 = 0.0;
      sho_under_rev(r.S1, r.w1, r.Q1, T.eps, C0[jc], C1[jc], C2[jc], C3[jc], bS1, bw1, bQ1);
      sho_under_rev(r.S2, r.w2, r.Q2, T.eps, C0[jc + 1], C1[jc + 1], C2[jc + 1], C3[jc + 1], bS2, bw2, bQ2);
      // S = (f) amp / (w Q);  w = k pi Q / (period sqrt(4 Q^2 - 1))
      double bamp = bS1 / (r.w1 * r.Q1) + bS2 * f / (r.w2 * r.Q2);
      double bf = bS2 * r.amp / (r.w2 * r.Q2);
      bw1 -= bS1 * r.S1 / r.w1; bQ1 -= bS1 * r.S1 / r.Q1;
      bw2 -= bS2 * r.S2 / r.w2; bQ2 -= bS2 * r.S2 / r.Q2;
      const double bperiod = -(bw1 * r.w1 + bw2 * r.w2) / period;
      bQ1 += bw1 * r.w1 / r.Q1 - (bw1 * r.w1 / r.g1) * 4.0 * r.Q1 / r.g1;
      bQ2 += bw2 * r.w2 / r.Q2 - (bw2 * r.w2 / r.g2) * 4.0 * r.Q2 / r.g2;
      bf -= bamp * r.amp / (1.0 + f);
      g[T.col[0]] += bamp * 2.0 * sigma / (1.0 + f);
      g[T.col[1]] += bperiod;
      g[T.col[2]] += bQ1 + bQ2;
      g[T.col[3]] += bQ1;
      g[T.col[4]] += bf;
      break;
    }
  }
}

// Host: is `prog` a well-formed flat list of records?  `width_limit`: Jr + 2 Jc above it is C2_ERR_UNSUPPORTED
// (32 for the flat program, what c2_loglik_terms takes; the leaves of an expression are only bounded by its registers).
inline int check_program(const c2_term_program *prog, int width_limit) {
  if (!prog || prog->nterms < 1 || prog->nterms > C2_TERMS_MAX || prog->np < 1 || prog->Jr < 0 || prog->Jc < 0) return C2_ERR_INVALID;
  if (prog->Jr + 2 * prog->Jc < 1) return C2_ERR_INVALID;
  if (prog->Jr + 2 * prog->Jc > width_limit) return C2_ERR_UNSUPPORTED;
  int jr = 0, jc = 0;
  for (int t = 0; t < prog->nterms; ++t) {
    const c2_term_rec &T = prog->term[t];
    int ncol, wr = 0, wc = 0;
    switch (T.kind) {
      case C2_TERM_REAL: ncol = 2; wr = 1; break;
      case C2_TERM_COMPLEX: ncol = 4; wc = 1; break;
      case C2_TERM_SHO:
        ncol = 3;
        if (T.regime == C2_SHO_UNDER) wc = 1;
        else if (T.regime == C2_SHO_OVER) wr = 2;
        else if (T.regime == C2_SHO_MIXED) { wr = 2; wc = 1; }
        else return C2_ERR_INVALID;
        if (T.par < 0 || T.par > 7) return C2_ERR_INVALID;
        break;
      case C2_TERM_MATERN32: ncol = 2; wc = 1; break;
      case C2_TERM_ROTATION: ncol = 5; wc = 2; break;
      default: return C2_ERR_INVALID;
    }
    for (int k = 0; k < ncol; ++k)
      if (T.col[k] < 0 || T.col[k] >= prog->np) return C2_ERR_INVALID;
    // slots in program order, reals and complex terms each concatenated (terms.py:233-235): every write stays inside (B, Jr|Jc)
    if (T.jr != jr || T.jc != jc) return C2_ERR_INVALID;
    jr += wr;
    jc += wc;
  }
  return (jr == prog->Jr && jc == prog->Jc) ? C2_OK : C2_ERR_INVALID;
}

}  // namespace c2leaf
