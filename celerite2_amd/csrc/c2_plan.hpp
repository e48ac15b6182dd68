// c2_plan.hpp -- host only: what the plans of the fused log-likelihood entry points share ("One plan
// per entry point").  A plan is two functions next to their dispatcher: one names the lane mapping that serves a call,
// one lays that mapping's regions into the caller's workspace.  The dispatcher switches on the first and takes every
// pointer from the second; the public size query is the largest `need` over the mappings the dispatcher can reach, so
// the two cannot disagree.  c2_loglik.hip: lane_mapping / grad_layout; c2_terms.hip: terms_mapping / terms_layout.
#pragma once
#include <cstddef>
#include <cstdint>
#include "c2_loglik_helpers.hpp"

namespace c2 {

// The kernel families (the values are what the c2_internal_*_plan test hooks report).
enum class Lanes : int {
  one = 1,       // one lane per series (c2_loglik_t.hip)
  two = 2,       // two lanes per series (c2_loglik_k2.hip)
  four = 4,      // four lanes per series (c2_loglik4.hip, c2_loglik_q4.hip)
  group = 8,     // a group of G = 1 .. 32 lanes per series; the gradient's reverse sweep by the backward recursion
  replay = 9,    // the same group, reverse sweep by checkpoint + replay
  timepar = 10,  // parallel along time, verified on the device, a row-by-row form gated behind it
  newton = 11,   // forward only: d, W by Newton iterations on the chunk start states
  wide = 12,     // C2_FAST_WIDTH < J: the op chain on the workgroup-per-series kernels
  composed = 13  // coefficient level only: matrices in memory, then the matrix-level entry point
};

inline size_t al2(size_t n) { return (n + 1) & ~(size_t)1; }   // sub-arrays stay 16-byte aligned
inline size_t max2(size_t a, size_t b) { return a > b ? a : b; }

// the words in front of a lane mapping's records that decide its fallback on the device: the head + one per group of 64
// series, rounded to 16 bytes
inline size_t gate_words(int64_t B) { return (size_t)((kGateHeadWords + (B + kWave - 1) / kWave + 1) & ~(int64_t)1); }

}  // namespace c2
