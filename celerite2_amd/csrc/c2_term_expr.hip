// c2_term_expr.hip -- TERM ALGEBRA on the device: sums, products (python/celerite2/terms.py:238-301), derivatives
// (terms.py:304-330) and the exposure-time convolution (terms.py:333-410) of the leaf terms of c2_term_params.hip, as a
// map parameters -> celerite coefficients (+ one diagonal shift per series) and its hand-written reverse.  A product of two
// celerite kernels is again a celerite kernel, so the fused likelihood kernels are untouched: this file sits in front of
// c2_loglik_terms[_grad] exactly where c2_term_coefficients[_rev] sits for a plain sum.
//
// The model is an EXPRESSION (c2_term_expr, celerite2_amd.h): the leaf program, then operation records in post-order.  It
// travels BY VALUE as a kernel argument, so a wavefront walks it with scalar loads and uniform branches -- front to back in
// k_expr_coefficients, and (after replaying the forward) back to front in k_expr_coefficients_rev.
//
// Mapping: one LANE per series, as the flat kernels.  What is new are the INTERMEDIATE coefficient lists: which registers
// an operation reads comes from the program at run time, and a run-time-indexed per-thread array would live in scratch.
// So the registers live in the caller's `work` buffer as [field of register][series]: lane b touches work[slot * B + b],
// consecutive lanes consecutive addresses, every access a coalesced 512-byte row of the wavefront; the kernels keep no
// per-thread array at all.  Every register is written exactly once in the forward (check_expr: results are allocated in
// increasing order), so the reverse can accumulate cotangents with += in one fixed order: no atomics, same bits every run.
//
// The convolution is complex arithmetic on (a - i b) and z = (c - i d) delta; where the reference's closed forms
// (cosh z - 1, z - sinh z) cancel, at small |z|, power series take over (conv_fg).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/celerite2_amd.h"
#include "c2_term_leaf.hpp"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace {

using namespace c2leaf;

// One field of the registers of ONE series: element k is `stride` doubles after element k - 1.
struct Strided {
  double *base;
  int64_t stride;
  __device__ __forceinline__ double &operator[](int k) const { return base[(int64_t)k * stride]; }
};

// The register file of one series inside work ([slot][series]): real register k = slots 2k (a), 2k + 1 (c); complex
// register k = slots 2 NR + 4k + (0: a, 1: b, 2: c, 3: d).
struct Regs {
  double *w;        // work + b (+ the cotangent half's offset)
  int64_t B, cb;    // cb = 2 NR
  __device__ __forceinline__ double &r(int k, int f) const { return w[(int64_t)(2 * k + f) * B]; }
  __device__ __forceinline__ double &c(int k, int f) const { return w[(cb + 4 * k + f) * B]; }
  __device__ __forceinline__ Strided rf(int f) const { return Strided{w + f * B, 2 * B}; }
  __device__ __forceinline__ Strided cf(int f) const { return Strided{w + (cb + f) * B, 4 * B}; }
};

struct Cx {
  double re, im;
};
__device__ __forceinline__ Cx cmul(Cx a, Cx b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ Cx cdiv(Cx a, Cx b) {
  const double n = b.re * b.re + b.im * b.im;
  return Cx{(a.re * b.re + a.im * b.im) / n, (a.im * b.re - a.re * b.im) / n};
}
__device__ __forceinline__ Cx conj(Cx a) { return Cx{a.re, -a.im}; }

// The two functions of the boxcar convolution at z = rate * delta and their derivatives:
//   F(z) = 2 (cosh z - 1) / z^2   (amplitude factor, terms.py:384-410),   F' = 2 sinh z / z^2 - 2 F / z
//   G(z) = 2 (z - sinh z) / z^2   (diagonal shift, terms.py:350-380),     G' = -F - 2 G / z
// The closed forms cancel: cosh z - 1 loses 2 / |z|^2 in relative accuracy, F' six times that -- and an exposure time is
// short against the kernel's time scales, |z| ~ 1e-2.  So below |z| = 1/2 the power series (nine terms: the first one
// dropped is below 1e-18) are summed instead, F = sum 2 w^k / (2k+2)!, G = -z sum 2 w^k / (2k+3)!, w = z^2; from
// |z| = 1/2 on the closed forms lose at most 8 (48 for the derivatives) units of rounding.
constexpr int kSeries = 9;
__device__ __forceinline__ double inv_factorial(int n) {
  double f = 1.0;
  for (int k = 2; k <= n; ++k) f *= (double)k;
  return 1.0 / f;
}
template <bool DERIV>
__device__ __forceinline__ void conv_fg(Cx z, Cx &F, Cx &G, Cx &dF, Cx &dG) {
  const Cx w = cmul(z, z);
  if (z.re * z.re + z.im * z.im < 0.25) {
    Cx f{0.0, 0.0}, g{0.0, 0.0}, df{0.0, 0.0}, dg{0.0, 0.0};
#pragma unroll
    for (int k = kSeries - 1; k >= 0; --k) {   // Horner in w (the factorials fold to constants)
      const double fk = 2.0 * inv_factorial(2 * k + 2), gk = -2.0 * inv_factorial(2 * k + 3);
      f = cmul(f, w); f.re += fk;
      g = cmul(g, w); g.re += gk;
      if constexpr (DERIV) {
        df = cmul(df, w); df.re += 2.0 * (k + 1) * 2.0 * inv_factorial(2 * k + 4);
        dg = cmul(dg, w); dg.re += (2 * k + 1) * gk;
      }
    }
    F = f;
    G = cmul(z, g);
    if constexpr (DERIV) {
      dF = cmul(z, df);
      dG = dg;
    }
    return;
  }
  const double ch = cosh(z.re), sh = sinh(z.re);
  double sy, cy;
  sincos(z.im, &sy, &cy);
  const Cx coshz{ch * cy, sh * sy}, sinhz{sh * cy, ch * sy};
  F = cdiv(Cx{2.0 * (coshz.re - 1.0), 2.0 * coshz.im}, w);
  G = cdiv(Cx{2.0 * (z.re - sinhz.re), 2.0 * (z.im - sinhz.im)}, w);
  if constexpr (DERIV) {
    const Cx a = cdiv(Cx{2.0 * sinhz.re, 2.0 * sinhz.im}, w), b = cdiv(F, z), c = cdiv(G, z);
    dF = Cx{a.re - 2.0 * b.re, a.im - 2.0 * b.im};
    dG = Cx{-F.re - 2.0 * c.re, -F.im - 2.0 * c.im};
  }
}

// ---- forward: leaves, then the operations front to back.  Returns the shift; `bad` as leaf_forward. ------------------
__device__ __forceinline__ double expr_forward(const c2_term_expr &E, const double *p, Regs V, int32_t &bad) {
  for (int t = 0; t < E.leaves.nterms; ++t)
    leaf_forward<Strided>(E.leaves.term[t], t, p, V.rf(0), V.rf(1), V.cf(0), V.cf(1), V.cf(2), V.cf(3), bad);
  double shift = 0.0;
  for (int i = 0; i < E.nops; ++i) {
    const c2_term_op &O = E.op[i];
    const c2_term_range A = O.a, Bq = O.b, D = O.out;
    switch (O.op) {
      case C2_OP_SUM: {
        for (int j = 0; j < A.nr; ++j)
          for (int f = 0; f < 2; ++f) V.r(D.r0 + j, f) = V.r(A.r0 + j, f);
        for (int j = 0; j < Bq.nr; ++j)
          for (int f = 0; f < 2; ++f) V.r(D.r0 + A.nr + j, f) = V.r(Bq.r0 + j, f);
        for (int j = 0; j < A.nc; ++j)
          for (int f = 0; f < 4; ++f) V.c(D.c0 + j, f) = V.c(A.c0 + j, f);
        for (int j = 0; j < Bq.nc; ++j)
          for (int f = 0; f < 4; ++f) V.c(D.c0 + A.nc + j, f) = V.c(Bq.c0 + j, f);
        break;
      }
      case C2_OP_PRODUCT: {   // terms.py:261-301, in its order
        int o = D.r0;
        for (int j = 0; j < A.nr; ++j) {
          const double aj = V.r(A.r0 + j, 0), cj = V.r(A.r0 + j, 1);
          for (int k = 0; k < Bq.nr; ++k, ++o) {
            V.r(o, 0) = aj * V.r(Bq.r0 + k, 0);
            V.r(o, 1) = cj + V.r(Bq.r0 + k, 1);
          }
        }
        int q = D.c0;
        for (int side = 0; side < 2; ++side) {   // real(a) x complex(b), then real(b) x complex(a)
          const c2_term_range X = side ? Bq : A, Y = side ? A : Bq;
          for (int j = 0; j < X.nr; ++j) {
            const double aj = V.r(X.r0 + j, 0), cj = V.r(X.r0 + j, 1);
            for (int k = 0; k < Y.nc; ++k, ++q) {
              V.c(q, 0) = aj * V.c(Y.c0 + k, 0);
              V.c(q, 1) = aj * V.c(Y.c0 + k, 1);
              V.c(q, 2) = cj + V.c(Y.c0 + k, 2);
              V.c(q, 3) = V.c(Y.c0 + k, 3);
            }
          }
        }
        for (int j = 0; j < A.nc; ++j) {
          const double aj = V.c(A.c0 + j, 0), bj = V.c(A.c0 + j, 1), cj = V.c(A.c0 + j, 2), dj = V.c(A.c0 + j, 3);
          for (int k = 0; k < Bq.nc; ++k, q += 2) {
            const double ak = V.c(Bq.c0 + k, 0), bk = V.c(Bq.c0 + k, 1), ck = V.c(Bq.c0 + k, 2), dk = V.c(Bq.c0 + k, 3);
            V.c(q, 0) = 0.5 * (aj * ak + bj * bk);
            V.c(q, 1) = 0.5 * (bj * ak - aj * bk);
            V.c(q, 2) = cj + ck;
            V.c(q, 3) = dj - dk;
            V.c(q + 1, 0) = 0.5 * (aj * ak - bj * bk);
            V.c(q + 1, 1) = 0.5 * (bj * ak + aj * bk);
            V.c(q + 1, 2) = cj + ck;
            V.c(q + 1, 3) = dj + dk;
          }
        }
        break;
      }
      case C2_OP_DIFF: {   // terms.py:319-330
        for (int j = 0; j < A.nr; ++j) {
          const double a = V.r(A.r0 + j, 0), c = V.r(A.r0 + j, 1);
          V.r(D.r0 + j, 0) = -a * c * c;
          V.r(D.r0 + j, 1) = c;
        }
        for (int j = 0; j < A.nc; ++j) {
          const double a = V.c(A.c0 + j, 0), b = V.c(A.c0 + j, 1), c = V.c(A.c0 + j, 2), d = V.c(A.c0 + j, 3);
          const double q = (d - c) * (d + c), m = 2.0 * c * d;   // (d^2 - c^2 without the cancellation of two rounded squares)
          V.c(D.c0 + j, 0) = a * q + b * m;
          V.c(D.c0 + j, 1) = b * q - a * m;
          V.c(D.c0 + j, 2) = c;
          V.c(D.c0 + j, 3) = d;
        }
        break;
      }
      case C2_OP_CONVOLVE: {   // terms.py:350-410: (a - i b) <- (a - i b) F(z), shift += Re (a - i b) G(z), z = (c - i d) delta
        const double dt = p[O.col];
        for (int j = 0; j < A.nr; ++j) {
          const double a = V.r(A.r0 + j, 0), c = V.r(A.r0 + j, 1);
          Cx F, G, u0, u1;
          conv_fg<false>(Cx{c * dt, 0.0}, F, G, u0, u1);
          V.r(D.r0 + j, 0) = a * F.re;
          V.r(D.r0 + j, 1) = c;
          shift += a * G.re;
        }
        for (int j = 0; j < A.nc; ++j) {
          const double a = V.c(A.c0 + j, 0), b = V.c(A.c0 + j, 1), c = V.c(A.c0 + j, 2), d = V.c(A.c0 + j, 3);
          Cx F, G, u0, u1;
          conv_fg<false>(Cx{c * dt, -d * dt}, F, G, u0, u1);
          const Cx al{a, -b};
          const Cx w = cmul(al, F);
          V.c(D.c0 + j, 0) = w.re;
          V.c(D.c0 + j, 1) = -w.im;
          V.c(D.c0 + j, 2) = c;
          V.c(D.c0 + j, 3) = d;
          shift += cmul(al, G).re;
        }
        break;
      }
    }
  }
  return shift;
}

__device__ __forceinline__ c2_term_range result_range(const c2_term_expr &E) {
  if (E.nops > 0) return E.op[E.nops - 1].out;
  return c2_term_range{0, E.leaves.Jr, 0, E.leaves.Jc};
}

__global__ __launch_bounds__(256) void k_expr_coefficients(c2_term_expr E, int64_t B, const double *__restrict__ P,
                                                           int64_t p_bs, double *__restrict__ ar, double *__restrict__ cr,
                                                           double *__restrict__ ac, double *__restrict__ bc,
                                                           double *__restrict__ cc, double *__restrict__ dc,
                                                           double *__restrict__ shift, int32_t *__restrict__ flag,
                                                           double *__restrict__ work) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *p = P + b * p_bs;
  const Regs V{work + b, B, 2 * (int64_t)E.NR};
  int32_t bad = 0;
  const double s = expr_forward(E, p, V, bad);
  const c2_term_range D = result_range(E);
  for (int j = 0; j < D.nr; ++j) {
    ar[b * D.nr + j] = V.r(D.r0 + j, 0);
    cr[b * D.nr + j] = V.r(D.r0 + j, 1);
  }
  for (int j = 0; j < D.nc; ++j) {
    ac[b * D.nc + j] = V.c(D.c0 + j, 0);
    bc[b * D.nc + j] = V.c(D.c0 + j, 1);
    cc[b * D.nc + j] = V.c(D.c0 + j, 2);
    dc[b * D.nc + j] = V.c(D.c0 + j, 3);
  }
  shift[b] = s;
  flag[b] = bad;
}

// The reverse.  Lane b: zero its row of bP and settle the flags as k_coefficients_rev; replay the forward into the value
// half of work; zero the cotangent half, load the result's cotangents, walk the operations last to first (+= into the
// operands' cotangents, one fixed order), then the leaves in program order.
__global__ __launch_bounds__(256) void k_expr_coefficients_rev(
    c2_term_expr E, int64_t B, const double *__restrict__ P, int64_t p_bs, const double *__restrict__ bar,
    const double *__restrict__ bcr, const double *__restrict__ bac, const double *__restrict__ bbc,
    const double *__restrict__ bcc, const double *__restrict__ bdc, const double *__restrict__ bshift,
    const int32_t *__restrict__ tflag, int32_t *__restrict__ lflag, double *__restrict__ ll, double *__restrict__ bP,
    double *__restrict__ work) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double *p = P + b * p_bs;
  double *g = bP + b * E.leaves.np;
  for (int k = 0; k < E.leaves.np; ++k) g[k] = 0.0;
  if (tflag && tflag[b] != 0) {
    if (ll) ll[b] = -INFINITY;
    if (lflag) lflag[b] = C2_FLAG_REGIME;
    return;
  }
  if (lflag && lflag[b] != 0) return;
  const int64_t nslots = 2 * (int64_t)E.NR + 4 * (int64_t)E.NC;
  const Regs V{work + b, B, 2 * (int64_t)E.NR};
  const Regs G{work + nslots * B + b, B, 2 * (int64_t)E.NR};
  int32_t bad = 0;
  expr_forward(E, p, V, bad);
  for (int64_t s = 0; s < nslots; ++s) G.w[s * B] = 0.0;
  const c2_term_range R = result_range(E);
  for (int j = 0; j < R.nr; ++j) {
    G.r(R.r0 + j, 0) = bar[b * R.nr + j];
    G.r(R.r0 + j, 1) = bcr[b * R.nr + j];
  }
  for (int j = 0; j < R.nc; ++j) {
    G.c(R.c0 + j, 0) = bac[b * R.nc + j];
    G.c(R.c0 + j, 1) = bbc[b * R.nc + j];
    G.c(R.c0 + j, 2) = bcc[b * R.nc + j];
    G.c(R.c0 + j, 3) = bdc[b * R.nc + j];
  }
  const double gs = bshift ? bshift[b] : 0.0;
  for (int i = E.nops - 1; i >= 0; --i) {
    const c2_term_op &O = E.op[i];
    const c2_term_range A = O.a, Bq = O.b, D = O.out;
    switch (O.op) {
      case C2_OP_SUM: {
        for (int j = 0; j < A.nr; ++j)
          for (int f = 0; f < 2; ++f) G.r(A.r0 + j, f) += G.r(D.r0 + j, f);
        for (int j = 0; j < Bq.nr; ++j)
          for (int f = 0; f < 2; ++f) G.r(Bq.r0 + j, f) += G.r(D.r0 + A.nr + j, f);
        for (int j = 0; j < A.nc; ++j)
          for (int f = 0; f < 4; ++f) G.c(A.c0 + j, f) += G.c(D.c0 + j, f);
        for (int j = 0; j < Bq.nc; ++j)
          for (int f = 0; f < 4; ++f) G.c(Bq.c0 + j, f) += G.c(D.c0 + A.nc + j, f);
        break;
      }
      case C2_OP_PRODUCT: {
        int o = D.r0;
        for (int j = 0; j < A.nr; ++j) {
          const double aj = V.r(A.r0 + j, 0);
          for (int k = 0; k < Bq.nr; ++k, ++o) {
            const double ga = G.r(o, 0), gc = G.r(o, 1);
            G.r(A.r0 + j, 0) += ga * V.r(Bq.r0 + k, 0);
            G.r(Bq.r0 + k, 0) += ga * aj;
            G.r(A.r0 + j, 1) += gc;
            G.r(Bq.r0 + k, 1) += gc;
          }
        }
        int q = D.c0;
        for (int side = 0; side < 2; ++side) {
          const c2_term_range X = side ? Bq : A, Y = side ? A : Bq;
          for (int j = 0; j < X.nr; ++j) {
            const double aj = V.r(X.r0 + j, 0);
            for (int k = 0; k < Y.nc; ++k, ++q) {
              const double ga = G.c(q, 0), gb = G.c(q, 1), gc = G.c(q, 2), gd = G.c(q, 3);
              G.r(X.r0 + j, 0) += ga * V.c(Y.c0 + k, 0) + gb * V.c(Y.c0 + k, 1);
              G.r(X.r0 + j, 1) += gc;
              G.c(Y.c0 + k, 0) += ga * aj;
              G.c(Y.c0 + k, 1) += gb * aj;
              G.c(Y.c0 + k, 2) += gc;
              G.c(Y.c0 + k, 3) += gd;
            }
          }
        }
        for (int j = 0; j < A.nc; ++j) {
          const double aj = V.c(A.c0 + j, 0), bj = V.c(A.c0 + j, 1);
          for (int k = 0; k < Bq.nc; ++k, q += 2) {
            const double ak = V.c(Bq.c0 + k, 0), bk = V.c(Bq.c0 + k, 1);
            const double ga0 = G.c(q, 0), gb0 = G.c(q, 1), gc0 = G.c(q, 2), gd0 = G.c(q, 3);
            const double ga1 = G.c(q + 1, 0), gb1 = G.c(q + 1, 1), gc1 = G.c(q + 1, 2), gd1 = G.c(q + 1, 3);
            // a0 = (aj ak + bj bk)/2, b0 = (bj ak - aj bk)/2, a1 = (aj ak - bj bk)/2, b1 = (bj ak + aj bk)/2
            const double sa = 0.5 * (ga0 + ga1), da = 0.5 * (ga0 - ga1), sb = 0.5 * (gb0 + gb1), db = 0.5 * (gb1 - gb0);
            G.c(A.c0 + j, 0) += sa * ak + db * bk;
            G.c(A.c0 + j, 1) += da * bk + sb * ak;
            G.c(Bq.c0 + k, 0) += sa * aj + sb * bj;
            G.c(Bq.c0 + k, 1) += da * bj + db * aj;
            G.c(A.c0 + j, 2) += gc0 + gc1;
            G.c(Bq.c0 + k, 2) += gc0 + gc1;
            G.c(A.c0 + j, 3) += gd0 + gd1;
            G.c(Bq.c0 + k, 3) += gd1 - gd0;
          }
        }
        break;
      }
      case C2_OP_DIFF: {
        for (int j = 0; j < A.nr; ++j) {
          const double a = V.r(A.r0 + j, 0), c = V.r(A.r0 + j, 1);
          const double ga = G.r(D.r0 + j, 0);
          G.r(A.r0 + j, 0) -= ga * c * c;
          G.r(A.r0 + j, 1) += G.r(D.r0 + j, 1) - 2.0 * a * c * ga;
        }
        for (int j = 0; j < A.nc; ++j) {
          const double a = V.c(A.c0 + j, 0), bb = V.c(A.c0 + j, 1), c = V.c(A.c0 + j, 2), d = V.c(A.c0 + j, 3);
          const double ga = G.c(D.c0 + j, 0), gb = G.c(D.c0 + j, 1);
          const double q = (d - c) * (d + c), m = 2.0 * c * d;   // (d^2 - c^2 without the cancellation of two rounded squares)
          G.c(A.c0 + j, 0) += ga * q - gb * m;
          G.c(A.c0 + j, 1) += ga * m + gb * q;
          G.c(A.c0 + j, 2) += G.c(D.c0 + j, 2) + 2.0 * (ga * (bb * d - a * c) - gb * (bb * c + a * d));
          G.c(A.c0 + j, 3) += G.c(D.c0 + j, 3) + 2.0 * (ga * (a * d + bb * c) + gb * (bb * d - a * c));
        }
        break;
      }
      case C2_OP_CONVOLVE: {   // G_u = conj(F'(u)) G_w for a holomorphic step w = F(u), gradients as (d/dRe, d/dIm)
        const double dt = p[O.col];
        for (int j = 0; j < A.nr; ++j) {
          const double a = V.r(A.r0 + j, 0), c = V.r(A.r0 + j, 1);
          Cx F, Gz, dF, dG;
          conv_fg<true>(Cx{c * dt, 0.0}, F, Gz, dF, dG);
          const double ga = G.r(D.r0 + j, 0);
          G.r(A.r0 + j, 0) += ga * F.re + gs * Gz.re;
          G.r(A.r0 + j, 1) += G.r(D.r0 + j, 1) + dt * a * (ga * dF.re + gs * dG.re);
        }
        for (int j = 0; j < A.nc; ++j) {
          const double a = V.c(A.c0 + j, 0), bb = V.c(A.c0 + j, 1), c = V.c(A.c0 + j, 2), d = V.c(A.c0 + j, 3);
          Cx F, Gz, dF, dG;
          conv_fg<true>(Cx{c * dt, -d * dt}, F, Gz, dF, dG);
          const Cx al{a, -bb};
          const Cx gw{G.c(D.c0 + j, 0), -G.c(D.c0 + j, 1)}, gv{gs, 0.0};
          const Cx x0 = cmul(conj(F), gw), x1 = cmul(conj(Gz), gv);
          const Cx y0 = cmul(conj(cmul(al, dF)), gw), y1 = cmul(conj(cmul(al, dG)), gv);
          const Cx gal{x0.re + x1.re, x0.im + x1.im}, gz{y0.re + y1.re, y0.im + y1.im};
          G.c(A.c0 + j, 0) += gal.re;
          G.c(A.c0 + j, 1) -= gal.im;
          G.c(A.c0 + j, 2) += G.c(D.c0 + j, 2) + dt * gz.re;
          G.c(A.c0 + j, 3) += G.c(D.c0 + j, 3) - dt * gz.im;
        }
        break;
      }
    }
  }
  for (int t = 0; t < E.leaves.nterms; ++t)
    leaf_reverse<Strided>(E.leaves.term[t], p, G.rf(0), G.rf(1), G.cf(0), G.cf(1), G.cf(2), G.cf(3), g);
}

inline bool range_ok(const c2_term_range &r, int rlim, int clim) {
  return r.r0 >= 0 && r.nr >= 0 && r.c0 >= 0 && r.nc >= 0 && r.r0 + r.nr <= rlim && r.c0 + r.nc <= clim;
}

// Every register index the kernels form is checked here, before any launch: operands lie below the result, results are
// allocated in increasing order from the end of the leaves, and the last result ends exactly at (NR, NC).
int check_expr(const c2_term_expr *E) {
  if (!E) return C2_ERR_INVALID;
  if (const int rc = check_program(&E->leaves, 2 * C2_EXPR_REGS_MAX)) return rc == C2_ERR_UNSUPPORTED ? C2_ERR_INVALID : rc;
  if (E->nops < 0 || E->nops > C2_EXPR_OPS_MAX || E->NR < 0 || E->NC < 0 || E->NR > C2_EXPR_REGS_MAX || E->NC > C2_EXPR_REGS_MAX)
    return C2_ERR_INVALID;
  int nr = E->leaves.Jr, nc = E->leaves.Jc;   // registers written so far
  if (nr > E->NR || nc > E->NC) return C2_ERR_INVALID;
  int Jr = nr, Jc = nc;
  for (int i = 0; i < E->nops; ++i) {
    const c2_term_op &O = E->op[i];
    const bool binary = O.op == C2_OP_SUM || O.op == C2_OP_PRODUCT;
    if (!binary && O.op != C2_OP_DIFF && O.op != C2_OP_CONVOLVE) return C2_ERR_INVALID;
    if (O.op == C2_OP_CONVOLVE && (i != E->nops - 1 || O.col < 0 || O.col >= E->leaves.np)) return C2_ERR_INVALID;
    // operands: inside what has been written; the result: fresh registers right after it
    if (!range_ok(O.a, nr, nc) || (binary && !range_ok(O.b, nr, nc))) return C2_ERR_INVALID;
    if (O.out.r0 != nr || O.out.c0 != nc || O.out.nr < 0 || O.out.nc < 0) return C2_ERR_INVALID;
    int64_t wr, wc;
    if (O.op == C2_OP_SUM) {
      wr = (int64_t)O.a.nr + O.b.nr;
      wc = (int64_t)O.a.nc + O.b.nc;
    } else if (O.op == C2_OP_PRODUCT) {
      wr = (int64_t)O.a.nr * O.b.nr;
      wc = (int64_t)O.a.nr * O.b.nc + (int64_t)O.b.nr * O.a.nc + 2 * (int64_t)O.a.nc * O.b.nc;
    } else {
      wr = O.a.nr;
      wc = O.a.nc;
    }
    if (wr != O.out.nr || wc != O.out.nc) return C2_ERR_INVALID;
    if (nr + wr > E->NR || nc + wc > E->NC) return C2_ERR_INVALID;
    nr += (int)wr;
    nc += (int)wc;
    Jr = (int)wr;
    Jc = (int)wc;
  }
  if (nr != E->NR || nc != E->NC || Jr + 2 * Jc < 1) return C2_ERR_INVALID;
  return Jr + 2 * Jc > 32 ? C2_ERR_UNSUPPORTED : C2_OK;   // what c2_loglik_terms takes
}

inline size_t slots_bytes(const c2_term_expr *E, int64_t B, int halves) {
  return (size_t)halves * (size_t)(2 * E->NR + 4 * E->NC) * (size_t)B * sizeof(double);
}

inline unsigned blocks_for(int64_t B) { return (unsigned)((B + 255) / 256); }

}  // namespace

extern "C" {

size_t c2_term_expr_workspace_bytes(const c2_term_expr *expr, int64_t B) {
  if (check_expr(expr) != C2_OK || B < 1) return 0;
  return slots_bytes(expr, B, 2);
}

int c2_term_expr_coefficients(const c2_term_expr *expr, int64_t B, const double *P, int64_t p_bs, double *ar, double *cr,
                              double *ac, double *bc, double *cc, double *dc, double *shift, int32_t *flag, void *work,
                              size_t work_bytes, c2_stream_t stream) {
  if (const int rc = check_expr(expr)) return rc;
  if (B < 1 || !P || !flag || !shift || !work || (p_bs != 0 && p_bs != expr->leaves.np)) return C2_ERR_INVALID;
  const c2_term_range D = expr->nops ? expr->op[expr->nops - 1].out : c2_term_range{0, expr->leaves.Jr, 0, expr->leaves.Jc};
  if ((D.nr && (!ar || !cr)) || (D.nc && (!ac || !bc || !cc || !dc))) return C2_ERR_INVALID;
  if (work_bytes < slots_bytes(expr, B, 1)) return C2_ERR_INVALID;
  hipLaunchKernelGGL(k_expr_coefficients, dim3(blocks_for(B)), dim3(256), 0, (hipStream_t)stream, *expr, B, P, p_bs, ar, cr,
                     ac, bc, cc, dc, shift, flag, (double *)work);
  return c2::launch_ok();
}

int c2_term_expr_coefficients_rev(const c2_term_expr *expr, int64_t B, const double *P, int64_t p_bs, const double *bar,
                                  const double *bcr, const double *bac, const double *bbc, const double *bcc,
                                  const double *bdc, const double *bshift, const int32_t *tflag, int32_t *lflag,
                                  double *ll, double *bP, void *work, size_t work_bytes, c2_stream_t stream) {
  if (const int rc = check_expr(expr)) return rc;
  if (B < 1 || !P || !bP || !work || (p_bs != 0 && p_bs != expr->leaves.np)) return C2_ERR_INVALID;
  const c2_term_range D = expr->nops ? expr->op[expr->nops - 1].out : c2_term_range{0, expr->leaves.Jr, 0, expr->leaves.Jc};
  if ((D.nr && (!bar || !bcr)) || (D.nc && (!bac || !bbc || !bcc || !bdc))) return C2_ERR_INVALID;
  if (work_bytes < slots_bytes(expr, B, 2)) return C2_ERR_INVALID;
  hipLaunchKernelGGL(k_expr_coefficients_rev, dim3(blocks_for(B)), dim3(256), 0, (hipStream_t)stream, *expr, B, P, p_bs, bar,
                     bcr, bac, bbc, bcc, bdc, bshift, tflag, lflag, ll, bP, (double *)work);
  return c2::launch_ok();
}

}  // extern "C"
