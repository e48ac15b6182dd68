// c2_term_params.hip -- term HYPER-PARAMETERS on the device: parameters -> celerite coefficients and the reverse of
// that map, plus the two hyper-parameters every model has (a jitter added to the white-noise diagonal, a constant mean).
//
// What a sampler or optimiser differentiates is S0, w0, Q (or sigma, rho, tau) of an SHO term, sigma, rho of a Matern-3/2
// term, sigma, period, Q0, dQ, f of a rotation term -- not the six coefficient arrays c2_loglik_terms takes.  The reference
// obtains that derivative by autodiff through its term classes (python/celerite2/jax/terms.py, pymc/terms.py); here the
// formulas of python/celerite2/terms.py:515-521 (RealTerm), 554-569 (ComplexTerm), 658-691 (SHOTerm), 729-745
// (Matern32Term) and 791-812 (RotationTerm) and their hand-written reverse are one kernel each, one thread per series.
//
// The model is a "program" (c2_term_program, celerite2_amd.h): the flattened sum of terms.  It travels to the kernels BY
// VALUE as a kernel argument -- no device allocation, no host read of device data -- so the wavefront walks it with
// scalar loads and uniform branches; only the per-series branch of the mixed SHO regime diverges.
//
// Mapping: k_coefficients / k_coefficients_rev one LANE per series (B x (NP + 2 Jr + 4 Jc) doubles in all: tens of
// megabytes at 65536 series, nothing to tune).  k_noise_mean_apply one block per 512-element row segment, 16 bytes per
// lane; k_noise_mean_rev one WAVEFRONT per series row, 16 bytes per lane per load, lane-strided partial sums in a fixed
// order and a __shfl_xor butterfly -- no atomics, so two runs give identical bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/celerite2_amd.h"

extern "C" void c2_internal_set_error(const char *msg);

namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559;

inline int launch_ok() {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return C2_OK;
  c2_internal_set_error(hipGetErrorString(e));
  return C2_ERR_HIP;
}

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

__global__ __launch_bounds__(256) void k_coefficients(c2_term_program prog, int64_t B, const double *__restrict__ P,
                                                      int64_t p_bs, double *__restrict__ ar, double *__restrict__ cr,
                                                      double *__restrict__ ac, double *__restrict__ bc,
                                                      double *__restrict__ cc, double *__restrict__ dc,
                                                      int32_t *__restrict__ flag) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *p = P + b * p_bs;
  const int64_t Jr = prog.Jr, Jc = prog.Jc;
  double *R0 = ar + b * Jr, *R1 = cr + b * Jr;
  double *C0 = ac + b * Jc, *C1 = bc + b * Jc, *C2 = cc + b * Jc, *C3 = dc + b * Jc;
  int32_t bad = 0;
  for (int t = 0; t < prog.nterms; ++t) {
    const c2_term_rec &T = prog.term[t];
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
  flag[b] = bad;
}

// The reverse.  Lane b owns row b of bP: it zeroes the row, then adds each term's contribution in program order (columns
// may be shared between terms), so the sum has one fixed order.  A series whose regime flag or factorisation flag is set
// gets a zero row, ll = -inf and lflag = C2_FLAG_REGIME (regime) -- the verdict never leaves the device.
__global__ __launch_bounds__(256) void k_coefficients_rev(c2_term_program prog, int64_t B, const double *__restrict__ P,
                                                          int64_t p_bs, const double *__restrict__ bar,
                                                          const double *__restrict__ bcr, const double *__restrict__ bac,
                                                          const double *__restrict__ bbc, const double *__restrict__ bcc,
                                                          const double *__restrict__ bdc, const int32_t *__restrict__ tflag,
                                                          int32_t *__restrict__ lflag, double *__restrict__ ll,
                                                          double *__restrict__ bP) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *p = P + b * p_bs;
  double *g = bP + b * prog.np;
  for (int k = 0; k < prog.np; ++k) g[k] = 0.0;
  if (tflag && tflag[b] != 0) {
    if (ll) ll[b] = -INFINITY;
    if (lflag) lflag[b] = C2_FLAG_REGIME;
    return;
  }
  if (lflag && lflag[b] != 0) return;
  const int64_t Jr = prog.Jr, Jc = prog.Jc;
  const double *R0 = bar + b * Jr, *R1 = bcr + b * Jr;
  const double *C0 = bac + b * Jc, *C1 = bbc + b * Jc, *C2 = bcc + b * Jc, *C3 = bdc + b * Jc;
  for (int t = 0; t < prog.nterms; ++t) {
    const c2_term_rec &T = prog.term[t];
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
}

// ---- jitter and mean ------------------------------------------------------------------------------------------------
constexpr int kSeg = 512;   // elements of one row segment: 256 lanes x 16 bytes

// diag = (sq ? yerr^2 : yerr) + jitter^2, r = y - mean.  Block = one segment of one row (flat grid: B * nseg blocks, no
// grid.y, so B is not limited to 65535).  VEC: N even -> every row starts 16-byte aligned and each lane moves a double2.
template <bool VEC>
__global__ __launch_bounds__(256) void k_noise_mean_apply(int64_t N, int nseg, int sq, const double *__restrict__ yerr,
                                                          const double *__restrict__ jitter, const double *__restrict__ mean,
                                                          const double *__restrict__ y, double *__restrict__ diag,
                                                          double *__restrict__ r) {
  const int64_t b = blockIdx.x / nseg;
  const int64_t n0 = (int64_t)(blockIdx.x % nseg) * kSeg;
  const double j = jitter ? jitter[b] : 0.0, m = mean ? mean[b] : 0.0;
  const double j2 = j * j;
  const int64_t row = b * N;
  if constexpr (VEC) {
    const int64_t n = n0 + 2 * threadIdx.x;
    if (n >= N) return;
    const double2 e = *reinterpret_cast<const double2 *>(yerr + row + n);
    const double2 v = *reinterpret_cast<const double2 *>(y + row + n);
    double2 d, o;
    d.x = (sq ? e.x * e.x : e.x) + j2;
    d.y = (sq ? e.y * e.y : e.y) + j2;
    o.x = v.x - m;
    o.y = v.y - m;
    *reinterpret_cast<double2 *>(diag + row + n) = d;
    *reinterpret_cast<double2 *>(r + row + n) = o;
  } else {
    for (int k = 0; k < 2; ++k) {
      const int64_t n = n0 + threadIdx.x + 256 * k;
      if (n >= N) return;
      const double e = yerr[row + n];
      diag[row + n] = (sq ? e * e : e) + j2;
      r[row + n] = y[row + n] - m;
    }
  }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// bjitter[b] = 2 jitter[b] sum_n bdiag[b, n], bmean[b] = -sum_n by[b, n]: one wavefront per row, ONE pass over both arrays.
// Summation order: lane l adds its elements n = 2 l, 2 l + 1, 2 l + 128, ... in increasing n, then the butterfly -- fixed.
template <bool VEC>
__global__ __launch_bounds__(256) void k_noise_mean_rev(int64_t B, int64_t N, const double *__restrict__ jitter,
                                                        const double *__restrict__ bdiag, const double *__restrict__ by,
                                                        const int32_t *__restrict__ flag, double *__restrict__ bjitter,
                                                        double *__restrict__ bmean) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;   // (whole wavefronts leave together)
  const double *pd = bdiag + b * N, *py = by + b * N;
  double sd = 0.0, sy = 0.0;
  if constexpr (VEC) {
    double sd1 = 0.0, sy1 = 0.0;
    for (int64_t n = 2 * lane; n < N; n += 128) {
      const double2 d = *reinterpret_cast<const double2 *>(pd + n);
      const double2 v = *reinterpret_cast<const double2 *>(py + n);
      sd += d.x; sd1 += d.y;
      sy += v.x; sy1 += v.y;
    }
    sd += sd1;
    sy += sy1;
  } else {
    for (int64_t n = lane; n < N; n += 64) {
      sd += pd[n];
      sy += py[n];
    }
  }
  sd = wave_sum(sd);
  sy = wave_sum(sy);
  if (lane == 0) {
    const bool dead = flag && flag[b] != 0;
    if (bjitter) bjitter[b] = dead ? 0.0 : 2.0 * (jitter ? jitter[b] : 0.0) * sd;
    if (bmean) bmean[b] = dead ? 0.0 : -sy;
  }
}

int check_program(const c2_term_program *prog) {
  if (!prog || prog->nterms < 1 || prog->nterms > C2_TERMS_MAX || prog->np < 1 || prog->Jr < 0 || prog->Jc < 0) return C2_ERR_INVALID;
  if (prog->Jr + 2 * prog->Jc < 1) return C2_ERR_INVALID;
  if (prog->Jr + 2 * prog->Jc > 32) return C2_ERR_UNSUPPORTED;   // what c2_loglik_terms takes
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

inline unsigned blocks_for(int64_t B) { return (unsigned)((B + 255) / 256); }

}  // namespace

extern "C" {

int c2_term_coefficients(const c2_term_program *prog, int64_t B, const double *P, int64_t p_bs, double *ar, double *cr,
                         double *ac, double *bc, double *cc, double *dc, int32_t *flag, c2_stream_t stream) {
  if (const int rc = check_program(prog)) return rc;
  if (B < 1 || !P || !flag || (p_bs != 0 && p_bs != prog->np)) return C2_ERR_INVALID;
  if ((prog->Jr && (!ar || !cr)) || (prog->Jc && (!ac || !bc || !cc || !dc))) return C2_ERR_INVALID;
  hipLaunchKernelGGL(k_coefficients, dim3(blocks_for(B)), dim3(256), 0, (hipStream_t)stream, *prog, B, P, p_bs, ar, cr, ac,
                     bc, cc, dc, flag);
  return launch_ok();
}

int c2_term_coefficients_rev(const c2_term_program *prog, int64_t B, const double *P, int64_t p_bs, const double *bar,
                             const double *bcr, const double *bac, const double *bbc, const double *bcc,
                             const double *bdc, const int32_t *tflag, int32_t *lflag, double *ll, double *bP,
                             c2_stream_t stream) {
  if (const int rc = check_program(prog)) return rc;
  if (B < 1 || !P || !bP || (p_bs != 0 && p_bs != prog->np)) return C2_ERR_INVALID;
  if ((prog->Jr && (!bar || !bcr)) || (prog->Jc && (!bac || !bbc || !bcc || !bdc))) return C2_ERR_INVALID;
  hipLaunchKernelGGL(k_coefficients_rev, dim3(blocks_for(B)), dim3(256), 0, (hipStream_t)stream, *prog, B, P, p_bs, bar, bcr,
                     bac, bbc, bcc, bdc, tflag, lflag, ll, bP);
  return launch_ok();
}

int c2_noise_mean_apply(int64_t B, int64_t N, const double *yerr, int yerr_is_sigma, const double *jitter,
                        const double *mean, const double *y, double *diag, double *r, c2_stream_t stream) {
  if (B < 1 || N < 1 || !yerr || !y || !diag || !r) return C2_ERR_INVALID;
  const int64_t nseg = (N + kSeg - 1) / kSeg;
  if (B * nseg > 0x7fffffffLL) return C2_ERR_INVALID;
  const dim3 grid((unsigned)(B * nseg));
  if (N % 2 == 0)
    hipLaunchKernelGGL(k_noise_mean_apply<true>, grid, dim3(256), 0, (hipStream_t)stream, N, (int)nseg, yerr_is_sigma, yerr,
                       jitter, mean, y, diag, r);
  else
    hipLaunchKernelGGL(k_noise_mean_apply<false>, grid, dim3(256), 0, (hipStream_t)stream, N, (int)nseg, yerr_is_sigma, yerr,
                       jitter, mean, y, diag, r);
  return launch_ok();
}

int c2_noise_mean_rev(int64_t B, int64_t N, const double *jitter, const double *bdiag, const double *by,
                      const int32_t *flag, double *bjitter, double *bmean, c2_stream_t stream) {
  if (B < 1 || N < 1 || !bdiag || !by || (!bjitter && !bmean)) return C2_ERR_INVALID;
  const dim3 grid((unsigned)((B + 3) / 4));
  if (N % 2 == 0)
    hipLaunchKernelGGL(k_noise_mean_rev<true>, grid, dim3(256), 0, (hipStream_t)stream, B, N, jitter, bdiag, by, flag,
                       bjitter, bmean);
  else
    hipLaunchKernelGGL(k_noise_mean_rev<false>, grid, dim3(256), 0, (hipStream_t)stream, B, N, jitter, bdiag, by, flag,
                       bjitter, bmean);
  return launch_ok();
}

}  // extern "C"
