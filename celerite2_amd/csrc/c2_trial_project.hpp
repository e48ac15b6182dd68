// c2_trial_project.hpp -- THE WALK of the projections on trial columns and the kernels that finish it differently:
// k_project (here; c2_trial_project.hip and c2_harmonic_trials.hip launch it), which stores the accumulators as
// P (B, K, C, R), and k_harmonic_null (c2_harmonic_trials.hip), which finishes the statistic of every (trial, vector) in
// registers after walk() and stores one value.  For every series b, trial k, column c of that trial and vector r,
//   acc[b, k, c, r] = sum_n col_c(trial k; t[b, n]) * alpha[b, n, r]
// with the columns formed in registers by the column sources the whitening sweeps use (c2_trial_columns.hpp).
//
// ONE WAVEFRONT takes 16 trials and RB = 16 NQ vectors and walks all N rows four at a time on the matrix cores,
// v_mfma_f64_16x16x4_f64 (lane maps: tools/ubench/mfma64.hip):
//   A operand: lane l forms the column value(s) of trial k0 + (l & 15) at row n0 + (l >> 4) -- one value per lane, in place;
//   B operand of vector tile q: alpha[b, n0 + (l >> 4), r0 + 16 q + (l & 15)] (16 lanes read 128 contiguous bytes);
//   C/D: one 4-register accumulator per (column, tile): lane l holds trials k0 + (l >> 4) + 4 reg, vector r0 + 16 q + (l & 15),
//        so the stores along r are contiguous.
// The accumulators spread over the vector axis across lanes, 8 registers per 16 vectors and column, where a lane per trial
// would hold 2 per vector and column.  The next step's B values and time are loaded before this step's columns are formed.
// Tails: a row n >= N loads row N - 1 and takes A = 0; a trial k >= K is the inert trial (all zeros) and stores nothing; a
// vector r >= R loads 0 and stores nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c2_common.hpp"
#include "c2_loglik_helpers.hpp"
#include "../../include/celerite2_amd.h"
#include "c2_launch.hpp"
#include "c2_trial_columns.hpp"

namespace c2 {
namespace project {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// k_project<Column, NQ>: the walk, then P.  Every element of P is written by exactly one lane: no atomics, no allocation,
// no host read, two calls give identical bits.  Blocks: B * ceil(R / RB) * ceil(K / 16) in grid.x, the trial blocks of one
// (series, vector block) next to each other (they read the same rows of alpha).
// (The walk stands in this kernel's own body and, for the kernels that finish in registers, once more in walk() below: with
// the walk behind a call the register allocation of k_project<Sinusoid, 4> and k_project<Keplerian, 8> moved -- 204 and 224
// registers to 196 and 208, or 236 and 208, by the form of the call -- and profiles/significance.md pins those kernels.)
template <class Column, int NQ>
__global__ __launch_bounds__(kWave) void k_project(int64_t N, int64_t K, int64_t R, int64_t KB, int64_t RBn,
                                                   const double *__restrict__ t, int64_t t_bs,
                                                   const double *__restrict__ trials, int64_t tr_bs,
                                                   const double *__restrict__ alpha, double *__restrict__ P,
                                                   const typename Column::Params prm) {
  constexpr int C = Column::NC;
  const int l = threadIdx.x, lo = l & 15, hi = l >> 4;
  const int64_t kb = blockIdx.x % KB, rb = (blockIdx.x / KB) % RBn, b = blockIdx.x / (KB * RBn);
  const int64_t k0 = kb * 16, r0 = rb * (16 * NQ);
  const bool live = k0 + lo < K;
  const Column lane(trials + b * tr_bs + (live ? k0 + lo : 0) * Column::WORDS, live, b, prm);

  const double *tb = t + b * t_bs, *ab = alpha + b * N * R;
  // this lane's vectors: one per tile (clamped for the load, zeroed after it)
  bool rlive[NQ];
  int64_t rcol[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int64_t r = r0 + 16 * q + lo;
    rlive[q] = r < R;
    rcol[q] = rlive[q] ? r : R - 1;
  }

  d4 acc[C][NQ];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[c][q] = d4{0.0, 0.0, 0.0, 0.0};

  // the step at rows n0 .. n0 + 3: this lane's row, clamped to the series
  auto load = [&](int64_t n0, double &tn, double (&bv)[NQ]) {
    const int64_t n = n0 + hi < N ? n0 + hi : N - 1;
    tn = tb[n];
    const double *ar = ab + n * R;
#pragma unroll
    for (int q = 0; q < NQ; ++q) bv[q] = ar[rcol[q]];
  };

  double tn, bv[NQ];
  load(0, tn, bv);
  for (int64_t n0 = 0; n0 < N; n0 += 4) {
    double tnext, bnext[NQ];
    load(n0 + 4 < N ? n0 + 4 : n0, tnext, bnext);            // (the last step loads its own rows again)
    double a[C];
    lane.columns(tn, a);
    const bool row = n0 + hi < N;
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = row ? a[c] : 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double bq = rlive[q] ? bv[q] : 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c][q] = mfma(a[c], bq, acc[c][q]);
    }
    tn = tnext;
#pragma unroll
    for (int q = 0; q < NQ; ++q) bv[q] = bnext[q];
  }

#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int64_t k = k0 + hi + 4 * reg;
    if (k < K) {
      double *Pk = P + (b * K + k) * C * R;
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          if (rlive[q]) Pk[c * R + rcol[q]] = acc[c][q][reg];
    }
  }
}

// THE WALK OF ONE WAVEFRONT for a kernel that finishes in registers: k_project's statements up to its stores.  `lane` is this
// lane's trial (k0 + lo), tb and ab the series' times and its rows of alpha, r0 the first vector of the block.  Leaves
// rlive[q], rcol[q] (this lane's vector of tile q: whether it exists, and its index clamped to R - 1) and acc[c][q][reg] of
// trial k0 + hi + 4 reg.
template <class Column, int NQ>
__device__ __forceinline__ void walk(int64_t N, int64_t R, int64_t r0, int lo, int hi, const Column &lane, const double *tb,
                                     const double *ab, bool (&rlive)[NQ], int64_t (&rcol)[NQ], d4 (&acc)[Column::NC][NQ]) {
  constexpr int C = Column::NC;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int64_t r = r0 + 16 * q + lo;
    rlive[q] = r < R;
    rcol[q] = rlive[q] ? r : R - 1;
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[c][q] = d4{0.0, 0.0, 0.0, 0.0};

  auto load = [&](int64_t n0, double &tn, double (&bv)[NQ]) {
    const int64_t n = n0 + hi < N ? n0 + hi : N - 1;
    tn = tb[n];
    const double *ar = ab + n * R;
#pragma unroll
    for (int q = 0; q < NQ; ++q) bv[q] = ar[rcol[q]];
  };

  double tn, bv[NQ];
  load(0, tn, bv);
  for (int64_t n0 = 0; n0 < N; n0 += 4) {
    double tnext, bnext[NQ];
    load(n0 + 4 < N ? n0 + 4 : n0, tnext, bnext);
    double a[C];
    lane.columns(tn, a);
    const bool row = n0 + hi < N;
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = row ? a[c] : 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double bq = rlive[q] ? bv[q] : 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c][q] = mfma(a[c], bq, acc[c][q]);
    }
    tn = tnext;
#pragma unroll
    for (int q = 0; q < NQ; ++q) bv[q] = bnext[q];
  }
}

// The checks every launch of the walk makes, in the launchers' order (sizes, limits, pointers and strides, blocks), and the
// grid: KB trial blocks, RBn vector blocks.  `kind`: what the entry point's own arguments add.
template <int NQ>
int grid(int64_t B, int64_t N, int64_t K, int64_t R, const double *t, int64_t t_bs, const double *trials, int64_t tr_bs,
         const double *alpha, const double *out, const trial::KindChecks &kind, int64_t &KB, int64_t &RBn) {
  if (B < 1 || N < 1 || K < 1 || R < 1 || kind.bad_size) return C2_ERR_INVALID;
  if (kind.too_large) return C2_ERR_UNSUPPORTED;
  if (!t || !trials || !alpha || !out || t_bs < 0 || tr_bs < 0 || kind.bad_arg) return C2_ERR_INVALID;
  KB = (K + 15) / 16, RBn = (R + 16 * NQ - 1) / (16 * NQ);
  if (KB > 0x7fffffffLL || RBn > 0x7fffffffLL / KB || B > 0x7fffffffLL / (KB * RBn)) return C2_ERR_UNSUPPORTED;   // 2^31 blocks or more
  return C2_OK;
}

// NQ: vector tiles of 16 per wavefront (RB / 16), from the headers' C2_TRIAL_*_DRAWS, C2_SHAPE_DRAWS and C2_HARMONIC_DRAWS_*
template <class Column, int DRAWS>
int launch(int64_t B, int64_t N, int64_t K, int64_t R, const double *t, int64_t t_bs, const double *trials, int64_t tr_bs,
           const double *alpha, double *P, const typename Column::Params &prm, c2_stream_t stream, const trial::KindChecks &kind = {}) {
  constexpr int NQ = DRAWS / 16;
  static_assert(DRAWS % 16 == 0 && NQ >= 1, "the draws of a wavefront are a multiple of 16");
  int64_t KB, RBn;
  if (const int rc = grid<NQ>(B, N, K, R, t, t_bs, trials, tr_bs, alpha, P, kind, KB, RBn)) return rc;
  hipLaunchKernelGGL((k_project<Column, NQ>), dim3((unsigned)(B * KB * RBn)), dim3(kWave), 0, (hipStream_t)stream, N, K, R, KB, RBn,
                     t, t_bs, trials, tr_bs, alpha, P, prm);
  return launch_ok();
}

}  // namespace project
}  // namespace c2
