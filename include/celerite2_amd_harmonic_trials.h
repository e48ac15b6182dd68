/* =============================================================================
 * celerite2_amd_harmonic_trials.h -- projections of many vectors on the 2 H
 * columns of a multi-harmonic frequency grid, and the multi-harmonic search
 * statistic of many null draws finished in registers: what the Monte-Carlo
 * false-alarm probability of the multi-harmonic periodogram reads.  The ninth
 * public header of libcelerite2_amd.so (the first, celerite2_amd.h, is
 * included for c2_stream_t and the error codes; the sixth,
 * celerite2_amd_trials.h, has the one-term projection this one repeats per
 * harmonic; the eighth, celerite2_amd_harmonics.h, has the column rule and
 * C2_HARMONICS_MAX).  Same conventions: float64, row-major, contiguous DEVICE
 * pointers, a leading batch dimension B of independent series, batch strides
 * in elements (0 when shared by the batch), the launch goes on `stream` and
 * the call returns without synchronising.
 *
 * No counterpart in the reference; parity is pinned by dense algebra.
 * ============================================================================= */
#ifndef CELERITE2_AMD_HARMONIC_TRIALS_H_
#define CELERITE2_AMD_HARMONIC_TRIALS_H_

#include "celerite2_amd.h"
#include "celerite2_amd_harmonics.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Vectors one wavefront takes beside its 16 frequencies, per H (multiples of 16): the block RB of R in the grids below.  The
 * accumulators of a wavefront take 2 H (RB / 16) 8 registers of a lane; the values are the faster of the candidates timed in
 * profiles/harmonic_significance.md.  (A build may set another value: an A/B build.) */
#ifndef C2_HARMONIC_DRAWS_1
#define C2_HARMONIC_DRAWS_1 64
#endif
#ifndef C2_HARMONIC_DRAWS_2
#define C2_HARMONIC_DRAWS_2 32
#endif
#ifndef C2_HARMONIC_DRAWS_3
#define C2_HARMONIC_DRAWS_3 16
#endif
#ifndef C2_HARMONIC_DRAWS_4
#define C2_HARMONIC_DRAWS_4 32
#endif

/* Projections on the columns of H harmonics: for the ANGULAR trial frequencies freq, shared by the batch (F,) (f_bs == 0) or
 * (B,F) (f_bs == F), and alpha (B,N,R), for every series b, frequency f, column i of the NC = 2 H columns ordered
 * (c_1, s_1, ..., c_H, s_H) of celerite2_amd_harmonics.h (c_h = cos x_h, s_h = sin x_h, x_h = fl(fl(h w_f) * fl(t - t_ref)))
 * and vector r
 *   P[b,f,i,r] = sum_n col_i(f; t[b,n]) * alpha[b,n,r]                                        (R innermost)
 * in ONE pass over alpha that forms the columns in registers and contracts them on the matrix cores
 * (csrc/c2_harmonic_trials.hip): the walk of c2_trial_projections on a column source of H sinusoids at the frequencies
 * fl(h w_f).  P[b,f,2h-2:2h,r] is, bit for bit, what c2_trial_projections(C2_TRIAL_SINUSOID) writes for a trial that holds
 * fl(h w_f).  With alpha[:, r] = (K + D)^-1 (y_r - mean), P holds the entries "gty" of c2_whitened_harmonics' T for y_r.
 * Each element of P is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  B, N, F, H, R >= 1 (else C2_ERR_INVALID); H <= C2_HARMONICS_MAX and B * ceil(F / 16) * ceil(R / C2_HARMONIC_DRAWS_H)
 * < 2^31 blocks (else C2_ERR_UNSUPPORTED).  A null pointer or a negative stride: C2_ERR_INVALID before any launch.  P must
 * not alias an input. */
int c2_harmonic_projections(int64_t B, int64_t N, int64_t F, int64_t H, int64_t R, const double *t, int64_t t_bs,
                            const double *freq /* angular */, int64_t f_bs /* 0: shared (F,) */, double t_ref,
                            const double *alpha /* (B, N, R) */, double *P /* (B, F, 2 H, R) */, c2_stream_t stream);

/* The multi-harmonic statistic of R null draws: the same walk, and P is never written -- each lane finishes the
 * (frequency, draw) pairs whose 2 H projections its accumulators hold, and the call writes D (B,F,R) only.  Beside the
 * arguments above: the factor of every frequency's M = Gtt - X^T X (celerite2_amd/harmonics.py), M = L L^T, as
 * Lm (B,F,H (2 H + 1)), the lower triangle row-major (L_00, L_10, L_11, L_20, ...); Xt (B,F,2 H,P0) with Xt[b,f,i,:] = column
 * i of X = L0^-1 Gt0^T; and V (B,P0,R) = L0^-1 g0y_r.  P0 nuisance columns, 0 <= P0 <= 7; Xt and V may be null when P0 == 0.
 * THE RULE, line by line, for one (b, f, r), with gty_i the projection above and i = 0 .. 2 H - 1 ascending:
 *   r_i   = gty_i - (X[0,i] v[0] + X[1,i] v[1] + ...)    the sum one term after the other, p ascending (each an fma), then
 *                                                        one subtraction
 *   w_i   = (r_i - L_i0 w_0 - ... - L_i,i-1 w_i-1) / L_ii  one term after the other, k ascending (each an fma); the division
 *                                                        correctly rounded
 *   dchi2 = w_0^2 + w_1^2 + ...                           i ascending (each an fma), from 0
 *   D[b,f,r] = dchi2
 * which is r^T M^-1 r, the drop of chi2 when the 2 H columns join the fit of y_r.  The kernel has no rule of its own for
 * NaN: a frequency or a series that must hold NaN arrives with NaN in Lm and the arithmetic carries it to every draw of that
 * frequency; other frequencies and series are not touched by it.
 * Each element of D is written by exactly one lane: no atomics, two calls give identical bits.  No allocation and no host
 * read.  B, N, F, H, R >= 1 and P0 >= 0 (else C2_ERR_INVALID); H <= C2_HARMONICS_MAX, P0 <= 7 and
 * B * ceil(F / 16) * ceil(R / C2_HARMONIC_DRAWS_H) < 2^31 blocks (else C2_ERR_UNSUPPORTED).  A null pointer (Xt, V: when
 * P0 > 0) or a negative stride: C2_ERR_INVALID before any launch.  D must not alias an input. */
int c2_harmonic_null_chi2(int64_t B, int64_t N, int64_t F, int64_t H, int64_t R, int64_t P0, const double *t, int64_t t_bs,
                          const double *freq /* angular */, int64_t f_bs /* 0: shared (F,) */, double t_ref,
                          const double *alpha /* (B, N, R) */, const double *Lm /* (B, F, H (2 H + 1)) */,
                          const double *Xt /* (B, F, 2 H, P0) */, const double *V /* (B, P0, R) */, double *D /* (B, F, R) */,
                          c2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_HARMONIC_TRIALS_H_ */
