/* =============================================================================
 * celerite2_amd_trials.h -- projections of many vectors on the columns of a
 * trial grid: what the Monte-Carlo false-alarm probability of the three
 * searches reads.  The sixth public header of libcelerite2_amd.so (the first,
 * celerite2_amd.h, is included for c2_stream_t and the error codes; the second
 * to fifth are celerite2_amd_linear.h, celerite2_amd_periodogram.h,
 * celerite2_amd_transit.h and celerite2_amd_kepler.h).  Same conventions:
 * float64, row-major, contiguous DEVICE pointers, a leading batch dimension B
 * of independent series, batch strides in elements (0 when shared by the
 * batch), the launch goes on `stream` and the call returns without
 * synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_TRIALS_H_
#define CELERITE2_AMD_TRIALS_H_

#include "celerite2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The kinds of trial: what `trials` holds per trial and the columns it stands for. */
#define C2_TRIAL_SINUSOID 0  /* (w): 1 double; columns cos x, sin x, x = fl(w * fl(t - t_ref))         (celerite2_amd_periodogram.h) */
#define C2_TRIAL_TRANSIT 1   /* (P, t0, w, tau): 4 doubles; one column, the box or trapezoid b_k(t)    (celerite2_amd_transit.h) */
#define C2_TRIAL_KEPLERIAN 2 /* (w, e, tp): 3 doubles; columns cos nu(t), sin nu(t)                    (celerite2_amd_kepler.h) */

/* Vectors one wavefront takes beside its 16 trials, per kind (multiples of 16): the block of R in the grid below. */
#define C2_TRIAL_SINUSOID_DRAWS 64
#define C2_TRIAL_TRANSIT_DRAWS 32
#define C2_TRIAL_KEPLERIAN_DRAWS 128

/* Projections on trial columns: for the trials of `kind`, shared by the batch (K,words) (tr_bs == 0) or (B,K,words)
 * (tr_bs == words K), and alpha (B,N,R), for every series b, trial k, column c of the trial (C = 2, or 1 for the transit) and
 * vector r
 *   P[b,k,c,r] = sum_n col_c(trial k; t[b,n]) * alpha[b,n,r]                                  (R innermost)
 * in ONE pass that forms the columns in registers -- by the rules of the three headers named above, bit for bit the values
 * the whitening sweeps c2_whitened_sinusoids / _transits / _keplerians use -- and contracts them with alpha on the matrix
 * cores (csrc/c2_trial_project.hip): a (K x N) (N x R) product whose left operand is never in memory.  The cost of forming
 * a column is paid once for all R vectors.  With K + D = L diag(d) L^T and alpha[:, r] = (K + D)^-1 (y_r - mean),
 *   P[b,k,c,r] = <L^-1 col_c, L^-1 (y_r - mean)>,   <a, b> = sum_n a_n b_n / d_n
 * which is the entry "gty" of T that a sweep would return for y_r (T[3 + P0], T[3 + Q0 + P0]; the transit: T[1 + P0]); every
 * other entry of T does not depend on y.  For a draw from the null, y_r - mean = L D^1/2 n_r with n_r ~ N(0, I):
 * alpha[:, r] = L^-T D^-1/2 n_r, one c2_solve_upper with R columns.  t_ref is read by C2_TRIAL_SINUSOID only.
 * The rule is evaluated as written for any trial; a caller masks the results of trials outside a search's domain.
 * Each element of P is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  B, N, K, R >= 1; B * ceil(K / 16) * ceil(R / C2_TRIAL_<KIND>_DRAWS) < 2^31 blocks (C2_ERR_UNSUPPORTED).  A null
 * pointer, a bad size or an unknown kind: C2_ERR_INVALID before any launch.  P must not alias an input. */
int c2_trial_projections(int kind, int64_t B, int64_t N, int64_t K, int64_t R, const double *t, int64_t t_bs,
                         const double *trials /* (K, words) | (B, K, words) */, int64_t tr_bs /* 0: shared */, double t_ref,
                         const double *alpha /* (B, N, R) */, double *P /* (B, K, C, R) */, c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_TRIALS_H_ */
