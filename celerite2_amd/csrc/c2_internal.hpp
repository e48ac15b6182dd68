// c2_internal.hpp -- the library's internal interface: every function that one .hip of this directory defines and another
// calls, declared ONCE.  The names have C linkage, so a caller's private copy of a prototype that drifted from the definition
// would still compile and link; with one declaration that callers AND the defining file include, a mismatch is a compile
// error ("conflicting types for ...").  Declarations only, grouped by the file that defines them.
//
// Not here: static helpers that carry a c2_internal_ name inside one file, and the hooks the tools load by name through
// ctypes (c2_internal_set_debug_sink, c2_internal_read_dbg, c2_internal_sweep_rev_prof_read, ...).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/celerite2_amd.h"

extern "C" {

// c2_fused.hip: the gradient as the literal op chain (the Python side loads these two by name as well)
size_t c2_loglik_grad_composite_workspace_bytes(int64_t B, int64_t N, int64_t J);
int c2_loglik_grad_composite(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                             const double *a, const double *U, const double *V, const double *y, double *ll, double *bt,
                             double *bc, double *ba, double *bU, double *bV, double *by, int32_t *flag, void *work,
                             size_t work_bytes, c2_stream_t stream);

// c2_general.hip
int64_t c2_internal_general_chunks_plan(int64_t B, int64_t M, int64_t nrhs);
size_t c2_internal_general_chunks_doubles(int64_t B, int64_t M, int64_t J, int64_t nrhs, int64_t Lc);
int c2_internal_general_chunks(int lower, int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, int64_t Lc,
                               const double *t1, int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c,
                               int64_t c_bs, const double *U, const double *V, const double *Y, double *Z, double *scratch,
                               c2_stream_t stream);
int c2_internal_generalK(int lower, int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                         int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs, const double *U,
                         const double *V, const double *Y, double *Z, double *F, int zero_z, c2_stream_t stream);

// c2_general_tile.hip
size_t c2_internal_general_tile_doubles(int64_t B, int64_t M, int64_t J, int64_t nrhs);
int c2_internal_general_tile(int lower, int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                             int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs, const double *U,
                             const double *V, const double *Y, double *Z, double *F, double *scratch, c2_stream_t stream);

// c2_loglik.hip
int c2_internal_use_timepar_solve(int64_t B, int64_t N, int64_t J);
int c2_internal_tpg_short_chunks(int64_t B, int64_t N);
double *c2_internal_get_debug_sink();   // diagnostics: where the verification words of a time-parallel call are copied
size_t c2_internal_factor_scratch_doubles(int64_t B, int64_t N, int64_t J);
int c2_internal_factor_fused_ws(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                int64_t c_bs, const double *a, const double *U, const double *V, double *d, double *W,
                                int32_t *flag, int allow_timepar, double *scratch, c2_stream_t stream);
int c2_internal_factor_fused(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                             const double *a, const double *U, const double *V, double *d, double *W, int32_t *flag,
                             int allow_timepar, c2_stream_t stream);
int c2_internal_factor_rev_long(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                int64_t c_bs, const double *U, const double *d, const double *W, const double *S,
                                const double *bd, const double *bW, double *bt, double *bc, double *ba, double *bU,
                                double *bV, c2_stream_t stream);
int c2_internal_factor_states_timepar(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                      int64_t c_bs, const double *a, const double *U, const double *V, double *d, double *W,
                                      double *S, int32_t *flag, c2_stream_t stream);
// one workgroup per wavefront of `spw` series: words[2 w] = c_max x the longest span between anchors four
// segments of C rows apart, words[2 w + 1] the same over single segments; +inf for unsorted / NaN times
int c2_internal_anchor_spans(int64_t B, int64_t N, int64_t J, int C, int spw, const double *t, int64_t t_bs, const double *c,
                             int64_t c_bs, unsigned long long *words, c2_stream_t stream);
size_t c2_internal_loglik_grad_rows_workspace_bytes(int64_t B, int64_t N, int64_t J);   // its `work` (not c2_loglik_grad's)
int c2_internal_loglik_grad_rows(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                 int64_t c_bs, const double *a, const double *U, const double *V, const double *y,
                                 double *ll, double *bt, double *bc, double *ba, double *bU, double *bV, double *by,
                                 int32_t *flag, void *work, size_t work_bytes, c2_stream_t stream);
int c2_internal_loglik_grad_replay(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                   int64_t c_bs, const double *a, const double *U, const double *V, const double *y,
                                   double *ll, double *bt, double *bc, double *ba, double *bU, double *bV, double *by,
                                   int32_t *flag, void *work, const unsigned long long *gate, c2_stream_t stream);
// coefficient-level log-likelihood with a group of J = 8, 4 or 2 lanes per series (k_loglik_fwd / k_loglik_rev<..., TT>): at
// most one wavefront per SIMD
size_t c2_internal_loglik_g8_tt_doubles(int64_t B, int64_t N, int64_t J);
int c2_internal_loglik_g8_tt_ok(int64_t B, int64_t N, int64_t J);
int c2_internal_loglik_g8_tt_grad(int64_t B, int64_t N, int64_t J, int64_t Jc, int coef_batched, const double *ar,
                                  const double *ac, const double *bc, const double *dc, const double *c, const double *x,
                                  int64_t x_bs, const double *diag, const double *y, double *ll, double *bar, double *bcr,
                                  double *bac, double *bbc, double *bcc, double *bdc, double *bx, double *bdiag, double *by,
                                  int32_t *flag, double *work, unsigned long long *guard, c2_stream_t stream);
int c2_internal_loglik_g8_tt(int64_t B, int64_t N, int64_t J, int64_t Jc, int coef_batched, const double *ar,
                             const double *ac, const double *bc, const double *dc, const double *c, const double *x,
                             int64_t x_bs, const double *diag, const double *y, double *ll, int32_t *flag,
                             unsigned long long *guard, c2_stream_t stream);
// ... and the matrix-level forward pass behind a gate word
int c2_internal_loglik_g8_gated(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                int64_t c_bs, const double *a, const double *U, const double *V, const double *y, double *ll,
                                int32_t *flag, const unsigned long long *gate, c2_stream_t stream);
// factor_rev from d, W alone (S is not read: the states are replayed), behind `gate` when it is not null
int c2_internal_factor_rev_replay(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                                  int64_t c_bs, const double *U, const double *d, const double *W, const double *S,
                                  const double *bd, const double *bW, double *bt, double *bc, double *ba, double *bU,
                                  double *bV, const unsigned long long *gate, c2_stream_t stream);

// c2_loglik4.hip: two columns per lane, J == 8
int c2_internal_loglik4(int64_t B, int64_t N, const double *t, int64_t t_bs, const double *c, int64_t c_bs, const double *a,
                        const double *U, const double *V, const double *y, double *ll, int32_t *flag, c2_stream_t stream);

// c2_loglik_k2.hip: two lanes per series, J == 8 (32 series per wavefront)
int c2_internal_loglik_k2_ok(int64_t B, int64_t N, int64_t J);
int c2_internal_loglik_k2(int64_t B, int64_t N, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                          const double *a, const double *U, const double *V, const double *y, double *ll, int32_t *flag,
                          c2_stream_t stream);
size_t c2_internal_loglik_k2_record_doubles(int64_t B, int64_t N);
int c2_internal_loglik_k2_grad(int64_t B, int64_t N, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                               const double *a, const double *U, const double *V, const double *y, double *ll, double *bt,
                               double *bc, double *ba, double *bU, double *bV, double *by, int32_t *flag, double *rec,
                               unsigned long long *guard, c2_stream_t stream);
// ... at coefficient level
int c2_internal_loglik_k2_tt(int64_t B, int64_t N, int64_t Jc, int coef_batched, const double *ar, const double *cr,
                             const double *ac, const double *bc, const double *cc, const double *dc, const double *x,
                             int64_t x_bs, const double *diag, const double *y, double *ll, int32_t *flag,
                             c2_stream_t stream);
int c2_internal_loglik_k2_tt_grad(int64_t B, int64_t N, int64_t Jc, int coef_batched, const double *ar, const double *cr,
                                  const double *ac, const double *bc, const double *cc, const double *dc, const double *x,
                                  int64_t x_bs, const double *diag, const double *y, double *ll, double *bar, double *bcr,
                                  double *bac, double *bbc, double *bcc, double *bdc, double *bx, double *bdiag, double *by,
                                  int32_t *flag, double *rec, unsigned long long *guard, c2_stream_t stream);

// c2_loglik_q4.hip: four lanes per series, gradient pair in the scaled frame, J == 8; the _tt forms at coefficient level
size_t c2_internal_loglik_q4_record_doubles(int64_t B, int64_t N);
int c2_internal_loglik_q4_grad(int64_t B, int64_t N, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                               const double *a, const double *U, const double *V, const double *y, double *ll, double *bt,
                               double *bc, double *ba, double *bU, double *bV, double *by, int32_t *flag, double *rec,
                               unsigned long long *guard, c2_stream_t stream);
int c2_internal_loglik_q4_tt(int64_t B, int64_t N, int64_t Jc, int coef_batched, const double *ar, const double *ac,
                             const double *bc, const double *dc, const double *c, const double *x, int64_t x_bs,
                             const double *diag, const double *y, double *ll, int32_t *flag, unsigned long long *words,
                             unsigned long long *guard, c2_stream_t stream);
size_t c2_internal_loglik_q4_span_words(int64_t B, int64_t N);
int c2_internal_loglik_q4_tt_grad(int64_t B, int64_t N, int64_t Jc, int coef_batched, const double *ar, const double *ac,
                                  const double *bc, const double *dc, const double *c, const double *x, int64_t x_bs,
                                  const double *diag, const double *y, double *ll, double *bar, double *bcr, double *bac,
                                  double *bbc, double *bcc, double *bdc, double *bx, double *bdiag, double *by,
                                  int32_t *flag, double *rec, unsigned long long *guard, c2_stream_t stream);

// c2_loglik_t.hip, compiled once per width (c2_loglik_t2.hip / _t4.hip / _t6.hip include it): one lane per series
#define C2_DECL_T(J_)                                                                                                   \
  int c2_internal_loglik_t##J_(int64_t B, int64_t N, const double *t, int64_t t_bs, const double *c, int64_t c_bs,     \
                               const double *a, const double *U, const double *V, const double *y, double *ll,        \
                               int32_t *flag, c2_stream_t stream);                                                    \
  size_t c2_internal_loglik_t_record_doubles##J_(int64_t B, int64_t N);                                               \
  int c2_internal_loglik_t_grad##J_(int64_t B, int64_t N, const double *t, int64_t t_bs, const double *c, int64_t c_bs, \
                                    const double *a, const double *U, const double *V, const double *y, double *ll,   \
                                    double *bt, double *bc, double *ba, double *bU, double *bV, double *by,           \
                                    int32_t *flag, double *rec, unsigned long long *guard, c2_stream_t stream);
C2_DECL_T(8)
C2_DECL_T(6)   // rows of 6 in memory, computed as rows of 8 (c2_loglik_t6.hip)
C2_DECL_T(4)
C2_DECL_T(2)
#undef C2_DECL_T
// ... at coefficient level: U_n / V_n generated from the coefficients in the lane, no matrices in memory
#define C2_DECL_TT(J_)                                                                                                  \
  int c2_internal_loglik_tt##J_(int64_t B, int64_t N, int64_t Jc, int coef_batched, const double *ar, const double *cr, \
                                const double *ac, const double *bc, const double *cc, const double *dc,               \
                                const double *x, int64_t x_bs, const double *diag, const double *y, double *ll,       \
                                int32_t *flag, c2_stream_t stream);                                                   \
  int c2_internal_loglik_tt_grad##J_(int64_t B, int64_t N, int64_t Jc, int coef_batched, const double *ar,            \
                                     const double *cr, const double *ac, const double *bc, const double *cc,          \
                                     const double *dc, const double *x, int64_t x_bs, const double *diag,             \
                                     const double *y, double *ll, double *bar, double *bcr, double *bac, double *bbc, \
                                     double *bcc, double *bdc, double *bx, double *bdiag, double *by, int32_t *flag,  \
                                     double *rec, unsigned long long *guard, c2_stream_t stream);
C2_DECL_TT(8)
C2_DECL_TT(4)
C2_DECL_TT(2)
#undef C2_DECL_TT

// c2_mfma.hip
int c2_internal_matmul_lower_mfma(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                                  const double *c, int64_t c_bs, const double *U, const double *V, const double *d,
                                  const double *Y, double *Z, int zero_z, c2_stream_t stream);

// c2_ops.hip
void c2_internal_set_error(const char *msg);
int c2_internal_matrices(int64_t B, int64_t N, int64_t Jr, int64_t Jc, const double *ar, const double *ac, const double *bc,
                         const double *dc, int coef_batched, const double *x, int64_t x_bs, const double *diag, double *a,
                         double *U, double *V, const unsigned long long *gate, c2_stream_t stream);

// c2_scan.hip
int c2_internal_matmul_chunked(int lower, int64_t B, int64_t N, int64_t J, int64_t nrhs, int64_t Lc, const double *t,
                               int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *V,
                               const double *Y, double *Z, double *F, int zero_z, c2_stream_t stream);

// c2_solve_cols.hip
size_t c2_internal_solve_cols_doubles(int64_t B, int64_t N, int64_t J, int64_t nrhs);
int c2_internal_solve_cols(int lower, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                           const double *c, int64_t c_bs, const double *U, const double *W, const double *Y, double *Z,
                           double *scratch, c2_stream_t stream);

// c2_sweep.hip
int c2_internal_sweep1(int lower, int solve, int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                       int64_t c_bs, const double *U, const double *V, const double *Y, double *Z, double *F, int zero_z,
                       c2_stream_t stream);
int c2_internal_sweep1_rev(int lower, int solve, int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs,
                           const double *c, int64_t c_bs, const double *U, const double *V, const double *Y, const double *Z,
                           const double *F, const double *bZ, double *bt, double *bc, double *bU, double *bV, double *bY,
                           c2_stream_t stream);
int c2_internal_sweepK(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                       const double *c, int64_t c_bs, const double *U, const double *V, const double *Y, double *Z,
                       double *F, int zero_z, c2_stream_t stream);

// c2_sweep_cols.hip
int c2_internal_sweep_cols(int lower, int solve, int64_t B, int64_t N, int64_t Jw, int64_t nrhs, const double *t,
                           int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Y,
                           double *Z, int64_t *B8, c2_stream_t stream);
int c2_internal_sweep_cols_rev(int lower, int solve, int64_t B, int64_t N, int64_t Jw, int64_t nrhs, const double *t,
                               int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *V,
                               const double *Y, const double *Z, const double *F, const double *bZ, double *bt, double *bc,
                               double *bU, double *bV, double *bY, int64_t *B8, c2_stream_t stream);

// c2_sweep_rev.hip
int c2_internal_sweepK_rev(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t,
                           int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Y,
                           const double *Z, const double *F, const double *bZ, double *bt, double *bc, double *bU,
                           double *bV, double *bY, c2_stream_t stream);
int c2_internal_sweep_rev_long(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t,
                               int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *V,
                               const double *Y, const double *Z, const double *F, const double *bZ, double *bt, double *bc,
                               double *bU, double *bV, double *bY, c2_stream_t stream);

// c2_sweep_small.hip
int c2_internal_sweepT(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                       const double *c, int64_t c_bs, const double *U, const double *V, const double *Y, double *Z,
                       double *F, int zero_z, c2_stream_t stream);

// c2_sweep_small_rev.hip
int c2_internal_sweepT_rev(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t,
                           int64_t t_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Y,
                           const double *Z, const double *F, const double *bZ, double *bt, double *bc, double *bU,
                           double *bV, double *bY, c2_stream_t stream);

// c2_timepar.hip: forward pass, factor and single-rhs solves parallel along time (chunk elements / affine chunk maps)
size_t c2_internal_timepar_doubles(int64_t B, int64_t N, int64_t J);
size_t c2_internal_loglik_timepar_doubles(int64_t B, int64_t N, int64_t J);
// width 8: the exact chunk start states X from the scanned chunk elements (chunks of R rows)
size_t c2_internal_e8_states_doubles(int64_t B, int64_t N, int64_t R);
int c2_internal_e8_states(int64_t B, int64_t N, int64_t R, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                          const double *a, const double *U, const double *V, double *X, double *work,
                          unsigned long long *guard, c2_stream_t stream);
int c2_internal_loglik_timepar(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                               const double *a, const double *U, const double *V, const double *y, double *ll, int32_t *flag,
                               double *work, unsigned long long *guard, c2_stream_t stream);
int c2_internal_factor_timepar(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                               const double *a, const double *U, const double *V, double *d, double *W, int32_t *flag,
                               double *work, unsigned long long *guard, c2_stream_t stream);
size_t c2_internal_timepar_solve_doubles(int64_t B, int64_t N, int64_t J);
int c2_internal_solve_timepar(int lower, int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,
                              int64_t c_bs, const double *U, const double *W, const double *Y, double *Z, double *scratch,
                              c2_stream_t stream);

// c2_timepar_grad.hip, compiled once per chunk length (c2_timepar_grad16.hip / _grad32.hip include it): gradient, Newton
// factor, wide log-likelihood, factor_rev and S rows parallel along time (widths 1 .. 8)
#define C2_DECL_TPG(R_)                                                                                                 \
  size_t c2_internal_timepar_grad_doubles##R_(int64_t B, int64_t N, int64_t J);                                        \
  int c2_internal_loglik_grad_timepar##R_(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs,              \
                                          const double *c, int64_t c_bs, const double *a, const double *U,             \
                                          const double *V, const double *y, double *ll, double *bt, double *bc,        \
                                          double *ba, double *bU, double *bV, double *by, int32_t *flag, double *work, \
                                          c2_stream_t stream);                                                         \
  size_t c2_internal_factor_iter_doubles##R_(int64_t B, int64_t N, int64_t J);                                         \
  int c2_internal_factor_iter##R_(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,     \
                                  int64_t c_bs, const double *a, const double *U, const double *V, double *d,          \
                                  double *W, int32_t *flag, double *work, const unsigned long long **last_word,        \
                                  c2_stream_t stream);                                                                 \
  size_t c2_internal_loglik_wide_doubles##R_(int64_t B, int64_t N, int64_t J);                                         \
  int c2_internal_loglik_wide##R_(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,     \
                                  int64_t c_bs, const double *a, const double *U, const double *V, const double *y,    \
                                  double *ll, int32_t *flag, double *work, c2_stream_t stream);                        \
  size_t c2_internal_factor_rev_timepar_doubles##R_(int64_t B, int64_t N, int64_t J);                                  \
  int c2_internal_factor_rev_timepar##R_(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs,               \
                                         const double *c, int64_t c_bs, const double *U, const double *V,              \
                                         const double *d, const double *W, const double *bd, const double *bW,         \
                                         double *bt, double *bc, double *ba, double *bU, double *bV, double *work,     \
                                         c2_stream_t stream);                                                          \
  size_t c2_internal_s_rows_doubles##R_(int64_t B, int64_t N, int64_t J);                                              \
  int c2_internal_s_rows##R_(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c,          \
                             int64_t c_bs, const double *d, const double *W, const int32_t *flag, double *Sw,          \
                             double *scratch, c2_stream_t stream);
C2_DECL_TPG(64)
C2_DECL_TPG(32)
C2_DECL_TPG(16)
#undef C2_DECL_TPG
// ... the chunk-map solves
#define C2_DECL_SC(R_)                                                                                                  \
  size_t c2_internal_solve_chunks_doubles##R_(int64_t B, int64_t N, int64_t J);                                        \
  int c2_internal_solve_chunks##R_(int lower, int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs,          \
                                   const double *c, int64_t c_bs, const double *U, const double *W, const double *Y,   \
                                   double *Z, double *scratch, c2_stream_t stream, int64_t nrhs, double *F);
C2_DECL_SC(64)
C2_DECL_SC(32)
C2_DECL_SC(16)
#undef C2_DECL_SC

// c2_wide.hip: wide models (C2_FAST_WIDTH < J <= C2_MAX_WIDTH), a workgroup per series, the state in LDS
int c2_wide_factor(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                   const double *a, const double *U, const double *V, double *d, double *W, double *S, int32_t *flag,
                   c2_stream_t stream);
int c2_wide_sweep(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                  const double *c, int64_t c_bs, const double *U, const double *V, const double *Y, double *Z, double *F,
                  int zero_z, c2_stream_t stream);
int c2_wide_sweep_rev(int lower, int solve, int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                      const double *c, int64_t c_bs, const double *U, const double *V, const double *Y, const double *Z,
                      const double *F, const double *bZ, double *bt, double *bc, double *bU, double *bV, double *bY,
                      c2_stream_t stream);
int c2_wide_factor_rev(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                       const double *U, const double *d, const double *W, const double *S, const double *bd,
                       const double *bW, double *bt, double *bc, double *ba, double *bU, double *bV, int accumulate,
                       c2_stream_t stream);
int c2_wide_general(int lower, int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1, int64_t t1_bs,
                    const double *t2, int64_t t2_bs, const double *c, int64_t c_bs, const double *U, const double *V,
                    const double *Y, double *Z, double *F, int zero_z, c2_stream_t stream);
// the log-likelihood from factor + solve_lower + a reduction; its gradient is the op chain of c2_fused.hip over the wide
// kernels, failed series filled with NaN afterwards
size_t c2_wide_loglik_doubles(int64_t B, int64_t N, int64_t J);
int c2_wide_loglik(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                   const double *a, const double *U, const double *V, const double *y, double *ll, int32_t *flag,
                   double *work, c2_stream_t stream);
int c2_wide_nan_failed(int64_t B, int64_t N, int64_t J, const int32_t *flag, double *bt, double *bc, double *ba, double *bU,
                       double *bV, double *by, c2_stream_t stream);

}  // extern "C"
