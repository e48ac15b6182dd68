// c2_merge_ring.hpp -- what the two event sweeps over the MERGE OF TWO SORTED GRIDS (N data times, M query times) by a
// group of G lanes per series share: the ring's constants, its layout and pin, for k_predvar (c2_predvar.hip, both
// directions) and k_priordraw (c2_priordraw.hip), and the one account of the ring and of the tie rule.  The arithmetic of
// an event, the rows' payloads, the state's dot product and update and the few lines of the merge decision stay with each
// kernel: moved into helpers they changed the kernels' code.  ONE EVENT PER ITERATION, both kinds predicated: every
// series of a wavefront either takes its next data row or its next query, so series whose grids interleave differently
// do not serialise each other.  THE TIE RULE: at equal times the data row goes first walking up and the query first
// walking down, so that in both directions a query at a data time has that row on its lower side -- the same n = "last
// data row with t_n <= s".
//
// The ring: kRing positions of BOTH streams are resident in LDS per series (slot = position mod kRing; data slots, then
// query slots, then one spare).  The row kRing positions down the moving stream is requested at the top of an event and
// written into the ring kPend events later (the event loop is unrolled by kPend, so the pending row sits in registers
// with a static name): nobody waits for a load, and every event issues the same loads so the compiler counts them.  The
// arriving row is never the slot the event reads: that slot was left kPend events ago.  At the end of a grid the request
// is clamped to the last row; a finished series requests into the spare slot.  Per-series ring stride = G (mod 32)
// doubles: the 32/G groups of a half-wavefront that read the same slot land in distinct banks (ds_read_b64: banks of 4
// bytes, modulus 64, per 32-lane half); series at different slots conflict at random.  The broadcast vectors of an event
// are [kWave] doubles, group g at g G: 32/G distinct addresses 2 G banks apart per half -- conflict-free as they stand.
#pragma once
#include "c2_common.hpp"

namespace c2 {

constexpr int kRing = 8;    // rows of either stream resident per series
constexpr int kPend = 4;    // events between the request of a row and its arrival in the ring (= the unroll)
constexpr int kSlots = 2 * kRing + 1;   // data slots, query slots, and one where the request of a finished series goes

// doubles per series: [SCAL scalar arrays: kSlots (+1) each, the time first][row A: kSlots x G][row B: kSlots x G]
// [EXTRA further doubles per slot], padded to G (mod 32).  VECS: the [kWave] broadcast vectors the kernel keeps beside it.
template <int G, int SCAL, int EXTRA, int VECS>
struct RingLayout {
  static constexpr int kScal = kSlots + (kSlots & 1);
  static constexpr int kRaw = SCAL * kScal + 2 * kSlots * G + kSlots * EXTRA;
  static constexpr int kStride = kRaw + (((G % 32) - kRaw % 32) + 32) % 32;
  static_assert(kStride % 32 == G % 32 && kStride >= kRaw && (kWave / G) * kStride * 8 + VECS * kWave * 8 <= 64 * 1024, "ring layout");
};

// The state's update stays in the event that made it: left to itself the compiler sinks it behind the event's predicated
// store into the next event, where the vectors it needs (three per column) no longer fit the registers beside the next
// event's own at G = 32.
__device__ __forceinline__ void pin(double &x) { asm volatile("" : "+v"(x)); }

}  // namespace c2
