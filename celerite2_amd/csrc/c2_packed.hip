// c2_packed.hip -- RAGGED BATCHES (c2_packed_api.h): the log-likelihood and its gradient of B series of different lengths,
// row-packed with offsets, in memory that grows like rows x J.  No counterpart in the reference, whose factor and solve
// (forward.hpp:69-170) take one series at a time.
//
// The recursion is that of the streaming filter from the empty state (c2_filter.hip: S, F unpropagated behind the last row,
// p := 0 for the first row of a series), and so is the mapping: a GROUP of G lanes per series, lane j owns column j (= row j)
// of S, the vectors p, u, w are shared through LDS, u^T g and u^T F are one interleaved DPP butterfly.  What differs:
//
//   rows      The row base of a series is offsets[b], the trip count of a wavefront its longest series; grid slot s works on
//             series order[s].  Nothing a series computes depends on its neighbours in the wavefront, so neither does a bit of
//             its results depend on `order`.
//   forward   Series are thousands of rows long and k_filter's row loop waits for each row's loads before it starts on the
//             row.  Here the five values of a row a lane needs (t, a, y, u_j, v_j) are loaded kAhead = 4 rows ahead into a
//             rotating set of registers (the loop is unrolled by kAhead, so the set is addressed statically and the compiler
//             counts the loads down with vmcnt instead of draining them).  A row of width 8 takes a few hundred cycles and a
//             load that misses every cache about 900: four rows ahead covers one miss per wavefront, and the other
//             wavefronts of the SIMD (the kernel needs few registers: several are resident) cover the rest.
//   reverse   Two-level checkpointing.  With C = ceil(sqrt(Nmax)) for every series, the forward pass of the gradient call
//             keeps d, W, z of every row (J + 2 doubles) and (F, S) after every C-th row; the reverse walks a series'
//             segments of C rows from the last to the first, REPLAYS a segment's states from its checkpoint into a ring of C
//             slots with the update line of the forward pass (no division, the same expression: the same bits) and then
//             walks the segment's rows backwards with the row of k_filter_rev (c2_filter_rev.hip has the formulas).  The state
//             cotangent -- Fb, the symmetric representative Sb, the carry of bt -- stays in registers from segment to
//             segment.  The forward recursion is never run backwards (profiles/r06_records.md: that inverts a contraction).
//             A lane reads back from the checkpoints and the ring only what it wrote itself.  Both passes over a segment
//             keep the next rows' records in flight as the forward pass does (four rows, two from G = 16 on), filled anew
//             at each segment: one exposed load latency per pass and segment instead of one per row.
//
// One writer per output element, no atomics, no allocation: two calls give identical bits.  B is in grid.x.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "c2_packed_api.h"
#include "c2_internal.hpp"
#include "c2_launch.hpp"

namespace c2 {
namespace packed {

constexpr int kAhead = 4;   // rows in flight in front of the row in hand (forward pass)
constexpr int64_t kMaxRows = 1LL << 30;   // of one series (row counters are int, with room for a segment on top)

// The contractions over a column in chunks of 8 with the scheduler held at the chunk's end from G = 16 on, as in
// c2_filter_rev.hip: left to itself it issues the LDS reads of a whole contraction ahead of the arithmetic.
template <int G>
__device__ __forceinline__ void chunk_end() {
  if constexpr (G > 8) __builtin_amdgcn_sched_barrier(0);
}

// Elements 0 .. J-1 of a row of a checkpoint or of the ring into a register column, zeros behind them.  All G loads are
// issued, at immediate offsets of one address, and the elements from J on are dropped by a select: they lie in the rows,
// slots or series behind this one or in the kPad doubles behind the ring, so they are inside `work` (what they hold is
// never used).  A load behind a branch on J each costs the G = 16 kernel its registers (it spills), a clamped index an
// address per element.
constexpr int kPad = 32;
template <int G>
__device__ __forceinline__ void load_row(double (&col)[G], const double *row, int J) {
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const double x = row[i];
    col[i] = i < J ? x : 0.0;
  }
}

// The series of this lane's grid slot and its rows [lo, lo + cnt): offsets clamped into [0, R], a negative length 0, a
// length beyond nmax cut there (the workspace of the gradient call is sized by it).
struct Rows {
  int64_t b, lo;
  int cnt, top;   // top: the longest series of the wavefront
  __device__ __forceinline__ Rows(int64_t slot, int64_t B, int64_t R, int nmax, const int64_t *offsets, const int32_t *order) {
    int64_t s = order ? (int64_t)order[slot] : slot;
    b = s < 0 ? 0 : (s >= B ? B - 1 : s);
    int64_t o0 = offsets[b], o1 = offsets[b + 1];
    o0 = o0 < 0 ? 0 : o0;
    o1 = o1 > R ? R : o1;
    int64_t n = o1 - o0;
    n = n < 0 ? 0 : (n > nmax ? nmax : n);
    lo = o0;
    cnt = (int)n;
    top = cnt;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const int x = __shfl_xor(top, o, kWave);
      top = x > top ? x : top;
    }
  }
};

struct RowIn {
  double t, a, y, u, v;
};
struct RowRec {
  double t, d, z, w;
};
struct RowBack {
  double t, tp, d, z, u, w;
};

// REC: the forward pass of the gradient call -- d, W, z are the records in `work` (never null) and ck (B, C, J + J^2)
// takes the state after every C-th row that has rows behind it.
template <int G, bool REC>
__global__ __launch_bounds__(kWave) void k_packed_fwd(int64_t B, int64_t R, int nmax, int C, int J,
                                                      const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
                                                      const double *__restrict__ t, const double *__restrict__ c, int64_t c_bs,
                                                      const double *__restrict__ a, const double *__restrict__ U,
                                                      const double *__restrict__ V, const double *__restrict__ y,
                                                      double *__restrict__ ll, int32_t *__restrict__ flag, double *__restrict__ d,
                                                      double *__restrict__ W, double *__restrict__ z, double *__restrict__ ck) {
  // No contraction of a product with a later sum (k_filter): the lanes of a group must agree on d to the bit, and S stay
  // symmetric to the bit.
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sp[kWave], su[kWave], sw[kWave];
  const Geo<G> L(B, J);
  const int j = L.j, g0 = (L.lane / G) * G;
  const bool act = L.act, wr = L.valid && L.act, wr0 = L.valid && j == 0;
  const Rows S(L.b, B, R, nmax, offsets, order);
  const int cnt = S.cnt;
  const int64_t lo = S.lo;
  const double cj = act ? c[S.b * c_bs + L.jj] : 0.0;   // (an idle lane reads column 0 and drops it, here and below)
  const int64_t WS = J + (int64_t)J * J;

  auto fetch = [&](int k) {   // row k of the series, 0 <= k < cnt
    const int64_t r = lo + k;
    RowIn x;
    x.t = t[r]; x.a = a[r]; x.y = y[r];
    x.u = U[r * J + L.jj]; x.v = V[r * J + L.jj];
    return x;
  };
  RowIn q[kAhead];
#pragma unroll
  for (int s = 0; s < kAhead; ++s) {
    q[s] = RowIn{0.0, 0.0, 0.0, 0.0, 0.0};
    if (cnt > 0) q[s] = fetch(s < cnt ? s : cnt - 1);
  }

  double tl = 0.0, ld = 0.0, qq = 0.0, F = 0.0;
  double Sc[G];
#pragma unroll
  for (int i = 0; i < G; ++i) Sc[i] = 0.0;
  bool empty = true;
  int fail = 0;
  int ckm = C;   // the next row count a checkpoint is due at

  for (int m0 = 0; m0 < S.top; m0 += kAhead) {
#pragma unroll
    for (int s = 0; s < kAhead; ++s) {
      const int m = m0 + s;
      if (m < cnt && fail == 0) {   // (uniform over the group)
        const RowIn x = q[s];
        {
          const int k = m + kAhead;
          q[s] = fetch(k < cnt ? k : cnt - 1);
        }
        const double tm = x.t, am = x.a, ym = x.y;
        double p = empty ? 0.0 : exp_decay(cj * (tl - tm));
        p = act ? p : 0.0;
        const double um = act ? x.u : 0.0, vm = act ? x.v : 0.0;
        sp[L.lane] = p; su[L.lane] = um;
        lds_order();
        F = p * F;
        double g = 0.0;
#pragma unroll
        for (int i = 0; i < G; ++i) {
          Sc[i] = (sp[g0 + i] * p) * Sc[i];
          g = fma(Sc[i], su[g0 + i], g);
        }
        double s1 = g * um, r1 = um * F;
        gsum2<G>(s1, r1);
        const double dm = am - s1, zm = ym - r1;
        if (dm <= 0.0) {   // (a NaN pivot passes)
          fail = m + 1;
          if (wr0 && (REC || d)) d[lo + m] = dm;
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
          tl = tm; empty = false;
          if (wr0) {
            if (REC || d) d[lo + m] = dm;
            if (REC || z) z[lo + m] = zm;
          }
          if (wr && (REC || W)) W[(lo + m) * J + j] = w;
          if constexpr (REC) {
            if (m + 1 == ckm) {
              ckm += C;
              if (wr && m + 1 < cnt) {
                double *o = ck + (S.b * C + (m + 1) / C) * WS;
                o[j] = F;
#pragma unroll
                for (int i = 0; i < G; ++i)
                  if (i < J) o[J + j * J + i] = Sc[i];
              }
            }
          }
        }
        lds_order();   // (the next row overwrites the vectors)
      }
    }
  }

  if (L.valid) {
    if (j == 0) {
      flag[S.b] = fail;
      ll[S.b] = fail ? -__builtin_inf() : -0.5 * (qq + ld) - 0.5 * ((double)cnt * kLog2Pi);
    }
    if (!REC && fail) {   // the failing row's W, z and everything behind it: NaN
      const double nan = __builtin_nan("");
      for (int m = fail - 1; m < cnt; ++m) {
        if (j == 0) {
          if (d && m >= fail) d[lo + m] = nan;
          if (z) z[lo + m] = nan;
        }
        if (act && W) W[(lo + m) * J + j] = nan;
      }
    }
  }
}

// The reverse.  d, W, z: the records of k_packed_fwd<G, true>; ck its checkpoints; ring (B, C, J + J^2).
template <int G>
__global__ __launch_bounds__(kWave) void k_packed_rev(int64_t B, int64_t R, int nmax, int C, int J,
                                                      const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
                                                      const double *__restrict__ t, const double *__restrict__ c, int64_t c_bs,
                                                      const double *__restrict__ U, const double *__restrict__ W,
                                                      const double *__restrict__ d, const double *__restrict__ z,
                                                      const int32_t *__restrict__ flag, const double *__restrict__ ck,
                                                      double *ring, double *__restrict__ bt, double *__restrict__ bc,
                                                      double *__restrict__ ba, double *__restrict__ bU, double *__restrict__ bV,
                                                      double *__restrict__ by) {
  // No contraction, as in k_filter_rev: the replay has to give the bits of the forward pass, and Sb stays symmetric to the bit.
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double sp[kWave], su[kWave], sw[kWave], sg[kWave];
  constexpr int CH = G < 8 ? G : 8;
  const Geo<G> L(B, J);
  const int j = L.j, g0 = (L.lane / G) * G;
  const bool act = L.act, wr = L.valid && L.act;
  const int64_t WS = J + (int64_t)J * J;
  Rows S(L.b, B, R, nmax, offsets, order);
  const int len = S.cnt;
  const int64_t lo = S.lo;
  const bool failed = flag[S.b] != 0;
  const int cnt = failed ? 0 : len;   // a failed series is not walked: NaN below
  int top = cnt;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int x = __shfl_xor(top, o, kWave);
    top = x > top ? x : top;
  }
  const double cj = act ? c[S.b * c_bs + L.jj] : 0.0;
  const double *ckb = ck + S.b * C * WS;
  double *rb = ring + S.b * C * WS;

  constexpr int AH = G <= 8 ? kAhead : 2;   // (the wide groups have no registers for more, and their rows take longer)
  auto fetch_rec = [&](int k) {    // what the replay reads of row k, 0 <= k < cnt
    const int64_t r = lo + k;
    return RowRec{t[r], d[r], z[r], W[r * J + L.jj]};
  };
  auto fetch_back = [&](int k) {   // ... and the backward walk (tp: the time before it; row 0 never uses its own)
    const int64_t r = lo + k;
    return RowBack{t[r], t[k > 0 ? r - 1 : r], d[r], z[r], U[r * J + L.jj], W[r * J + L.jj]};
  };

  const double lb = -0.5, qb = -0.5;   // the cotangents of sum log d and sum z^2 / d
  double carry = 0.0;                  // what bt of the row in hand has received from behind it
  double Fb = 0.0, bcj = 0.0;
  double Sb[G];
#pragma unroll
  for (int i = 0; i < G; ++i) Sb[i] = 0.0;

  double S0[G];   // (the elements i >= J stay 0: a row is loaded up to J)
#pragma nounroll
  for (int seg = (top + C - 1) / C - 1; seg >= 0; --seg) {
    const int m_lo = seg * C, m_hi = m_lo + C < top ? m_lo + C : top;
    const int end = m_hi < cnt ? m_hi : cnt;   // this series' rows of the segment: m_lo .. end-1

    // ---- replay: the state every row of the segment starts from -> ring ---------------------------------------------------
    {
      double F = 0.0, tl = 0.0;
      double (&Sc)[G] = S0;   // (one column for the replayed state and, below, for the state a row starts from)
#pragma unroll
      for (int i = 0; i < G; ++i) Sc[i] = 0.0;
      const bool empty0 = seg == 0;
      if (!empty0 && m_lo < cnt) {   // (uniform over the group)
        const double *o = ckb + seg * WS;
        const double f0 = o[L.jj];
        F = act ? f0 : 0.0;
        load_row<G>(Sc, o + J + L.jj * J, J);
        tl = t[lo + m_lo - 1];
      }
      bool empty = empty0;
      RowRec qr[AH];   // the records of the next AH rows, in flight (as q of k_packed_fwd)
#pragma unroll
      for (int s = 0; s < AH; ++s) {
        qr[s] = RowRec{0.0, 0.0, 0.0, 0.0};
        if (m_lo < end) qr[s] = fetch_rec(m_lo + s < end ? m_lo + s : end - 1);
      }
#pragma nounroll
      for (int m0 = m_lo; m0 < m_hi; m0 += AH) {
#pragma unroll
       for (int s = 0; s < AH; ++s) {
        const int m = m0 + s;
        if (m < end) {   // (uniform over the group)
          if (wr) {
            double *o = rb + (m - m_lo) * WS;
            o[j] = F;
#pragma unroll
            for (int i = 0; i < G; ++i)
              if (i < J) o[J + j * J + i] = Sc[i];
          }
          if (m + 1 < end) {   // (the state behind the segment's last row is the next checkpoint)
            chunk_end<G>();
            const RowRec x = qr[s];
            {
              const int k = m + AH;
              qr[s] = fetch_rec(k < end ? k : end - 1);
            }
            const double tm = x.t;
            double p = empty ? 0.0 : exp_decay(cj * (tl - tm));
            p = act ? p : 0.0;
            const double dm = x.d, zm = x.z;
            const double w = act ? x.w : 0.0;
            sp[L.lane] = p; sw[L.lane] = w;
            lds_order();
#pragma unroll
            for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
              for (int i = i0; i < i0 + CH; ++i) Sc[i] = fma(sw[g0 + i] * w, dm, (sp[g0 + i] * p) * Sc[i]);
              chunk_end<G>();
            }
            F = fma(w, zm, p * F);
            tl = tm; empty = false;
            lds_order();   // (the next row overwrites the vectors)
          }
        }
       }
      }
    }

    // ---- the segment's rows backwards (the row of k_filter_rev with bd = bW = bz = 0) -----------------------------------------
    const bool has = m_lo < end;   // this series has rows in the segment
    auto row_of = [&](int k) { return k < m_lo ? m_lo : (k < end ? k : end - 1); };
    RowBack qb_[AH];   // the next AH rows in flight; a series that ends inside the segment idles first, so every lane loads
#pragma unroll
    for (int s = 0; s < AH; ++s) {
      qb_[s] = RowBack{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (has) qb_[s] = fetch_back(row_of(m_hi - 1 - s));
    }
#pragma nounroll
    for (int m1 = m_hi - 1; m1 >= m_lo; m1 -= AH) {
#pragma unroll
     for (int s = 0; s < AH; ++s) {
      const int m = m1 - s;
      const RowBack x = qb_[s];
      if (has && m - AH >= m_lo) qb_[s] = fetch_back(row_of(m - AH));
      if (m >= m_lo && m < end) {   // (uniform over the group)
        chunk_end<G>();   // (nothing of the row before moves in here)
        const double *o = rb + (m - m_lo) * WS;
        const double f0 = o[L.jj];
        const double F0 = act ? f0 : 0.0;
        load_row<G>(S0, o + J + L.jj * J, J);
        const bool emp = m == 0;
        const double tm = x.t, tp = x.tp;
        double p = emp ? 0.0 : exp_decay(cj * (tp - tm));
        p = act ? p : 0.0;
        const double dm = x.d, zm = x.z;
        const double u = act ? x.u : 0.0, w = act ? x.w : 0.0;
        sp[L.lane] = p; su[L.lane] = u; sw[L.lane] = w;
        lds_order();
        const double Ft = p * F0;
        double g = 0.0, Sw = 0.0;
#pragma unroll
        for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
          for (int i = i0; i < i0 + CH; ++i) {
            S0[i] = (sp[g0 + i] * p) * S0[i];   // St from here on
            g = fma(S0[i], su[g0 + i], g);
            Sw = fma(Sb[i], sw[g0 + i], Sw);
          }
          chunk_end<G>();
        }
        double s1 = w * Sw, s2 = Fb * w;
        gsum2<G>(s1, s2);
        const double rd = rcp_nr(dm), zr = zm * rd;
        double db = lb * rd - qb * (zr * zr) + s1;
        const double zb = 2.0 * (qb * zr) + s2;
        const double wb = zm * Fb + 2.0 * (dm * Sw);
        double ub = -(zb * Ft);
        const double Ftb = Fb - zb * u;
        const double bv = wb * rd;
        double s3 = wb * w;
        s3 = gsum<G>(s3);
        db -= s3 * rd;
        ub -= db * g;
        const double gb = -bv - db * u;
        sg[L.lane] = act ? gb : 0.0;
        lds_order();
        double acc = 0.0, pb = 0.0;
#pragma unroll
        for (int i0 = 0; i0 < G; i0 += CH) {
#pragma unroll
          for (int i = i0; i < i0 + CH; ++i) {
            acc = fma(S0[i], sg[g0 + i], acc);
            const double Stb = Sb[i] + 0.5 * (sg[g0 + i] * u + su[g0 + i] * gb);
            pb = fma(Stb, S0[i], pb);
            Sb[i] = (sp[g0 + i] * p) * Stb;
          }
          chunk_end<G>();
        }
        pb = 2.0 * pb + Ftb * Ft;   // p o pb: only that product is used, and St = (p p^T) o S0 already has both factors
        Fb = p * Ftb;
        double s4 = cj * pb;
        s4 = gsum<G>(s4);
        const double Db = emp ? 0.0 : -s4;   // cotangent of t_m - t_{m-1}
        bcj -= emp ? 0.0 : (tm - tp) * pb;
        if (L.valid) {
          if (j == 0) { bt[lo + m] = carry + Db; ba[lo + m] = db; by[lo + m] = zb; }
          if (act) { bU[(lo + m) * J + j] = ub + acc; bV[(lo + m) * J + j] = bv; }
        }
        carry = 0.0 - Db;
        lds_order();   // (the next row overwrites the vectors)
      }
     }
    }
  }

  if (L.valid) {
    const double nan = __builtin_nan("");
    if (failed) {
      for (int m = 0; m < len; ++m) {
        if (j == 0) { bt[lo + m] = nan; ba[lo + m] = nan; by[lo + m] = nan; }
        if (act) { bU[(lo + m) * J + j] = nan; bV[(lo + m) * J + j] = nan; }
      }
    }
    if (act) bc[S.b * J + j] = failed ? nan : bcj;
  }
}

inline int64_t interval(int64_t nmax) {   // max(1, ceil(sqrt(nmax)))
  int64_t C = 1;
  while (C * C < nmax) ++C;
  return C;
}

inline bool sizes_ok(int64_t B, int64_t R, int64_t J) { return B >= 1 && R >= 0 && J >= 1; }

}  // namespace packed
}  // namespace c2

using namespace c2;
using namespace c2::packed;

extern "C" size_t c2_packed_loglik_grad_workspace_bytes(int64_t B, int64_t R, int64_t Nmax, int64_t J) {
  if (!sizes_ok(B, R, J) || J > C2_FAST_WIDTH || Nmax < 0 || Nmax > kMaxRows) return 0;
  const int64_t C = interval(Nmax);
  return sizeof(double) * (size_t)(R * (J + 2) + 2 * B * C * (J * J + J) + kPad);
}

extern "C" int c2_packed_loglik(int64_t B, int64_t R, int64_t J, const int64_t *offsets, const int32_t *order, const double *t,
                                const double *c, int64_t c_bs, const double *a, const double *U, const double *V,
                                const double *y, double *ll, int32_t *flag, double *d, double *W, double *z,
                                c2_stream_t stream) {
  if (!sizes_ok(B, R, J)) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH) return C2_ERR_UNSUPPORTED;
  if (!offsets || !t || !c || !a || !U || !V || !y || !ll || !flag) return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    hipLaunchKernelGGL((k_packed_fwd<G, false>), dim3((unsigned)((B * G + kWave - 1) / kWave)), dim3(kWave), 0, s, B, R,
                       (int)kMaxRows, 1, (int)J, offsets, order, t, c, c_bs, a, U, V, y, ll, flag, d, W, z, (double *)nullptr);
  });
  return launch_ok();
}

extern "C" int c2_packed_loglik_grad(int64_t B, int64_t R, int64_t Nmax, int64_t J, const int64_t *offsets, const int32_t *order,
                                     const double *t, const double *c, int64_t c_bs, const double *a, const double *U,
                                     const double *V, const double *y, double *ll, double *bt, double *bc, double *ba,
                                     double *bU, double *bV, double *by, int32_t *flag, void *work, size_t work_bytes,
                                     c2_stream_t stream) {
  if (!sizes_ok(B, R, J) || Nmax < 0) return C2_ERR_INVALID;
  if (J > C2_FAST_WIDTH || Nmax > kMaxRows) return C2_ERR_UNSUPPORTED;
  if (!offsets || !t || !c || !a || !U || !V || !y || !ll || !bt || !bc || !ba || !bU || !bV || !by || !flag || !work)
    return C2_ERR_INVALID;
  if (work_bytes < c2_packed_loglik_grad_workspace_bytes(B, R, Nmax, J)) return C2_ERR_INVALID;
  if ((B * group_size(J) + kWave - 1) / kWave > 0x7fffffffLL) return C2_ERR_UNSUPPORTED;
  const int64_t C = interval(Nmax), WS = J * J + J;
  double *d = static_cast<double *>(work), *z = d + R, *W = z + R, *ck = W + R * J, *ring = ck + B * C * WS;
  hipStream_t s = (hipStream_t)stream;
  dispatch_group(J, [&](auto g) {
    constexpr int G = decltype(g)::value;
    const dim3 grid((unsigned)((B * G + kWave - 1) / kWave));
    hipLaunchKernelGGL((k_packed_fwd<G, true>), grid, dim3(kWave), 0, s, B, R, (int)Nmax, (int)C, (int)J, offsets, order, t, c,
                       c_bs, a, U, V, y, ll, flag, d, W, z, ck);
    hipLaunchKernelGGL((k_packed_rev<G>), grid, dim3(kWave), 0, s, B, R, (int)Nmax, (int)C, (int)J, offsets, order, t, c, c_bs,
                       U, W, d, z, flag, ck, ring, bt, bc, ba, bU, bV, by);
  });
  return launch_ok();
}
