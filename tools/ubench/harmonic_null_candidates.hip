// harmonic_null_candidates.hip -- every candidate NQ (tiles of 16 draws a wavefront) of the two kernels of
// csrc/c2_harmonic_trials.hip, instantiated side by side so that tools/bench_harmonic_significance.py --static-only can put
// their registers in one table (device-only compile; nothing here is linked or run).  The library ships one NQ per H:
// C2_HARMONIC_DRAWS_H / 16 of include/celerite2_amd_harmonic_trials.h.
#include "../../celerite2_amd/csrc/c2_harmonic_trials.hip"

namespace c2 {
#define C2_CANDIDATE(H, NQ)                                                                                                      \
  template __global__ void harmonic_trials::k_harmonic_null<H, NQ>(int64_t, int64_t, int64_t, int64_t, int64_t, int, const double *, \
                                                                   int64_t, const double *, int64_t, const double *, const double *, \
                                                                   const double *, const double *, double *,                      \
                                                                   const trial::Sinusoid::Params);                                \
  template __global__ void project::k_project<trial::Harmonics<H>, NQ>(int64_t, int64_t, int64_t, int64_t, int64_t, const double *, \
                                                                       int64_t, const double *, int64_t, const double *, double *, \
                                                                       const trial::Sinusoid::Params);
C2_CANDIDATE(1, 1) C2_CANDIDATE(1, 2) C2_CANDIDATE(1, 4) C2_CANDIDATE(1, 8)
C2_CANDIDATE(2, 1) C2_CANDIDATE(2, 2) C2_CANDIDATE(2, 4)
C2_CANDIDATE(3, 1) C2_CANDIDATE(3, 2) C2_CANDIDATE(3, 4)
C2_CANDIDATE(4, 1) C2_CANDIDATE(4, 2) C2_CANDIDATE(4, 4)
}  // namespace c2
