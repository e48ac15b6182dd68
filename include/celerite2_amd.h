/* =============================================================================
 * celerite2_amd.h -- C-ABI of libcelerite2_amd.so (MI355X / gfx950 HIP backend)
 *
 * Drop-in boundary for ONE hot path of exoplanet-dev/celerite2: the O(N)
 * semiseparable GP linear algebra (factor / solve_* / matmul_* /
 * general_matmul_* and the *_rev reverse-mode passes).  Each entry point cites
 * the reference interface it replaces (paths relative to the reference repo).
 *
 * Conventions (all entry points)
 *   - float64 only, C-contiguous row-major, exactly like the reference's
 *     `py::array_t<double, py::array::c_style>` arguments
 *     (python/celerite2/driver.cpp:13-21).
 *   - Caller allocates every output and workspace; the library keeps no state
 *     between calls and allocates no user-visible memory (driver.cpp:13-64).
 *     Internal scratch of a few entry points (time-parallel forms, many
 *     right-hand sides) is a stream-ordered temporary from a memory pool the
 *     LIBRARY owns (one per device, up to 1 GiB kept cached between calls); the
 *     device's default pool, which the process shares with everybody else, is
 *     never reconfigured.  The c2h_* host entry points keep one staging arena,
 *     pinned bounce buffer and stream PER CALLING THREAD (re-entrant).
 *   - Alignment: every double* argument -- input, output or workspace -- is
 *     8-byte aligned, and that is all an entry point asks for: 16-byte
 *     alignment selects faster kernels and never changes results beyond
 *     rounding (a view that starts at an odd element is a valid argument).
 *   - Aliasing.  Exact-pointer aliasing the reference allows is allowed here
 *     too: d == a and W == V for factor (forward.hpp:55-58), Z == Y for
 *     solve_* / matmul_* (numpy.py:95-108).  The c2h_* host entry points also
 *     take INPUTS that are views of one array: two inputs that start at the
 *     same address and differ in length (t1 = x[:k] with t2 = x; ar and ac cut
 *     from the front of one coefficient vector) behave exactly as if the
 *     shorter one were a copy, in either argument order; views that start at
 *     different addresses are staged separately, as copies would be.  The one
 *     call they refuse (C2_ERR_INVALID) is an OUTPUT that starts at the
 *     address of an argument of another length: the reference would read
 *     rows the same call has already overwritten, a result that follows its
 *     row order and that no staged copy reproduces.
 *   - Return value: C2_OK (0) or a negative C2_ERR_* code.  A non positive
 *     definite matrix is NOT an error code: `flag[b]` receives the first row
 *     index n >= 1 with d[n] <= 0, or 0 on success (forward.hpp:128,134), and
 *     rows 0..n of d / 0..n-1 of W are already written, as in the reference.
 *   - Non-finite values.  A NaN or an infinity in a, U, V, y, a right-hand side
 *     or a cotangent is handled per series as the reference handles it: the
 *     only test is `d[n] <= 0`, which a NaN pivot passes, so such a series
 *     keeps flag 0 (-inf on the diagonal fails the test like any non-positive
 *     pivot), the NaN propagates through the recursions as IEEE arithmetic
 *     carries it (rows before it in a lower sweep or a factorisation, rows
 *     after it in an upper sweep, and every other right-hand-side column stay
 *     finite), nothing is sanitised and nothing is reported.  No other series
 *     of the batch is affected: its results are those it would have had
 *     without the poisoned neighbour, up to WHICH formulation computed them
 *     (a time-parallel form hands the whole batch to the row-by-row kernels
 *     when its device-side verification sees a NaN; either one meets the same
 *     accuracy).  Non-finite TIMES and RATES (t, c, query times, trial grids,
 *     frequencies) are outside this contract: they steer merges and searches,
 *     and the Python front end rejects such grids.
 *
 * Two families
 *   c2_*   device entry points: every pointer is a DEVICE pointer, there is a
 *          leading batch dimension B (B independent series, contiguous
 *          batch-major: t (B,N) or shared (N,), c (B,J) or shared (J,),
 *          a (B,N), U (B,N,J), Y (B,N,nrhs), S (B,N,J,J), F (B,N,J,nrhs) ...),
 *          and the launch is asynchronous on `stream` (a hipStream_t passed as
 *          void*; NULL = the default stream).  `t_bs` / `c_bs` are the batch
 *          strides of t and c in elements (N / J, or 0 when shared by the batch).
 *   c2h_*  host entry points: every pointer is a HOST pointer, B == 1, the call
 *          stages through device memory, runs the same kernels and returns
 *          after the results are back on the host.  These are what the
 *          `driver` / `backprop` pybind11 modules bind.
 *
 * Width limit: 1 <= J <= C2_MAX_WIDTH = 128.  Up to C2_FAST_WIDTH = 32 (the
 * reference's CELERITE_MAX_WIDTH, c++/include/celerite2/terms.hpp:10-12: the
 * widths it instantiates at compile time) the tuned kernels run; 33 .. 128 --
 * the reference's Eigen::Dynamic path, python/celerite2/driver.hpp:98-99 --
 * run on the workgroup-per-series kernels of csrc/c2_wide.hip.  J > 128 returns
 * C2_ERR_UNSUPPORTED, and so do the 2-D and coefficient-level extensions
 * (c2_kron_*, c2_loglik_terms*) above 32.
 * ============================================================================= */
#ifndef CELERITE2_AMD_H_
#define CELERITE2_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C2_OK 0
#define C2_ERR_INVALID (-1)     /* bad size / null pointer ("Invalid shape", driver.cpp:40-46) */
#define C2_ERR_UNSUPPORTED (-2) /* J > C2_MAX_WIDTH (or an extension entry point beyond C2_FAST_WIDTH) */
#define C2_ERR_HIP (-3)         /* HIP runtime error (no device, launch failure, OOM) */
#define C2_MAX_WIDTH 128 /* the reference's dynamic path takes any J (driver.hpp:98-99); here the J x J state must fit LDS */
#define C2_FAST_WIDTH 32 /* widths the tuned kernels cover; beyond: the workgroup-per-series kernels of csrc/c2_wide.hip.
                            The extensions without a reference counterpart (c2_kron_*, c2_loglik_terms*) stop here. */

typedef void *c2_stream_t; /* hipStream_t */

/* Library / device information. */
const char *c2_version(void);
int c2_device_count(void);         /* number of visible HIP devices, 0 if none */
const char *c2_last_error(void);   /* text of the last HIP error seen by this thread */

/* Dispatch options (celerite2_amd/csrc/c2_dispatch.hpp; no counterpart in the reference, whose code has one formulation
 * per op).  Which formulation an entry point runs -- row by row, parallel along time, which lane mapping -- follows from
 * the shape through one table of switches and measured thresholds.  The table is initialised from the environment ONCE,
 * when the library is loaded (variable names in INTEGRATION.md section 5); afterwards only c2_set_option changes it:
 * `name` is the option's name or its environment variable, `value` its new value as text, NULL / "" = back to the
 * default (switches: to the automatic choice).  Every alternative is parity-tested: options move speed, not results
 * (beyond rounding).  Not thread-safe against concurrent launches that depend on the option being changed.
 * c2_options_reload_env re-reads the environment (test harnesses that edit os.environ after loading the library). */
int c2_set_option(const char *name, const char *value);
int c2_get_option(const char *name, double *value, int *is_set);
int c2_option_count(void);
int c2_option_info(int index, const char **name, const char **env, double *default_value, int *is_switch,
                   const char **doc, const char **measured);
void c2_options_reload_env(void);

/* ---------------------------------------------------------------------------
 * DEVICE entry points (batched, asynchronous)
 * ------------------------------------------------------------------------- */

/* core::factor  -- c++/include/celerite2/forward.hpp:69-135 (with workspace S)
 * and interface.hpp:37-48 (S == NULL).  driver.factor (driver.cpp:13-64),
 * backprop.factor_fwd (backprop.cpp:12-67).
 * d (B,N), W (B,N,J), S (B,N,J,J) with S[n, i + J*j] = Sn(i,j), flag (B,) int32. */
int c2_factor(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
              const double *a, const double *U, const double *V, double *d, double *W, double *S /* nullable */,
              int32_t *flag, c2_stream_t stream);

/* core::solve_lower / solve_upper -- forward.hpp:156-170, 193-207 (F nullable:
 * interface.hpp:70-80, 102-112).  Z = L^-1 Y / L^-T Y, L = I + tril(U W^T).
 * driver.solve_lower/upper (driver.cpp:66-178).  F[n, j + J*k] = Fn(j,k). */
int c2_solve_lower(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                   int64_t c_bs, const double *U, const double *W, const double *Y, double *Z,
                   double *F /* nullable */, c2_stream_t stream);
int c2_solve_upper(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                   int64_t c_bs, const double *U, const double *W, const double *Y, double *Z,
                   double *F /* nullable */, c2_stream_t stream);

/* core::matmul_lower / matmul_upper -- forward.hpp:228-239, 260-271.
 * Z += tril(U V^T) Y / Z += triu(V U^T) Y: ACCUMULATES into the caller's Z
 * (driver.cpp:180-292).  The backprop *_fwd variants zero Z first
 * (backprop.cpp:505,511): pass zero_z != 0. */
int c2_matmul_lower(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                    int64_t c_bs, const double *U, const double *V, const double *Y, double *Z,
                    double *F /* nullable */, int zero_z, c2_stream_t stream);
int c2_matmul_upper(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                    int64_t c_bs, const double *U, const double *V, const double *Y, double *Z,
                    double *F /* nullable */, int zero_z, c2_stream_t stream);

/* core::general_matmul_lower / upper -- forward.hpp:285-332, 346-392
 * (driver.cpp:294-420, backprop.cpp:761-901).  t1 (B,N) / t2 (B,M) sorted;
 * U (B,N,J), V (B,M,J), Y (B,M,nrhs), Z (B,N,nrhs) accumulated,
 * F (B,M,J,nrhs) nullable, row-major F[m, j*nrhs + k]. */
int c2_general_matmul_lower(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                            int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs,
                            const double *U, const double *V, const double *Y, double *Z, double *F /* nullable */,
                            int zero_z, c2_stream_t stream);
int c2_general_matmul_upper(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                            int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs,
                            const double *U, const double *V, const double *Y, double *Z, double *F /* nullable */,
                            int zero_z, c2_stream_t stream);

/* core::factor_rev -- c++/include/celerite2/reverse.hpp:10-85
 * (backprop.factor_rev, backprop.cpp:68-150).  Outputs fully overwritten:
 * bt (B,N), bc (B,J), ba (B,N), bU (B,N,J), bV (B,N,J).  S must be the workspace of c2_factor for these d, W (as in the
 * reference); on small batches of series of 512 rows and more the states are replayed from d, W instead of read from S
 * (the reverse pass parallel along time), which is the same thing for a consistent S. */
int c2_factor_rev(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                  const double *a, const double *U, const double *V, const double *d, const double *W,
                  const double *S, const double *bd, const double *bW, double *bt, double *bc, double *ba,
                  double *bU, double *bV, c2_stream_t stream);

/* core::solve_lower_rev / solve_upper_rev / matmul_lower_rev / matmul_upper_rev
 * -- reverse.hpp:87-217 over internal::forward_rev / backward_rev
 * (internal.hpp:191-303); backprop.cpp:216-302, 368-454, 520-606, 672-758.
 * Outputs fully overwritten: bt (B,N), bc (B,J), bU, bW|bV (B,N,J), bY (B,N,nrhs). */
int c2_solve_lower_rev(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                       int64_t c_bs, const double *U, const double *W, const double *Y, const double *Z,
                       const double *F, const double *bZ, double *bt, double *bc, double *bU, double *bW, double *bY,
                       c2_stream_t stream);
int c2_solve_upper_rev(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                       int64_t c_bs, const double *U, const double *W, const double *Y, const double *Z,
                       const double *F, const double *bZ, double *bt, double *bc, double *bU, double *bW, double *bY,
                       c2_stream_t stream);
int c2_matmul_lower_rev(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                        const double *c, int64_t c_bs, const double *U, const double *V, const double *Y,
                        const double *Z, const double *F, const double *bZ, double *bt, double *bc, double *bU,
                        double *bV, double *bY, c2_stream_t stream);
int c2_matmul_upper_rev(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs,
                        const double *c, int64_t c_bs, const double *U, const double *V, const double *Y,
                        const double *Z, const double *F, const double *bZ, double *bt, double *bc, double *bU,
                        double *bV, double *bY, c2_stream_t stream);

/* driver::get_celerite_matrices -- python/celerite2/driver.cpp:422-477.
 * Coefficients ar (B,Jr), ac/bc/dc (B,Jc) with batch stride coef_bs in
 * {0 = shared, 1 = per series}; x (B,N) / shared (N,) via x_bs; diag (B,N).
 * Outputs a (B,N), U (B,N,J), V (B,N,J), J = Jr + 2 Jc, complex terms at
 * interleaved columns (Jr+2j, Jr+2j+1).  No sortedness precondition, as in the
 * reference's elementwise recipe: phases |dc x| beyond 1.6e6 (raw Julian dates)
 * take the library's large-argument sincos -- whole terms when the two ENDS of
 * a series' grid say so, single rows of an unsorted grid otherwise (a second,
 * row-parallel kernel that returns at once in the common case). */
int c2_get_celerite_matrices(int64_t B, int64_t N, int64_t Jr, int64_t Jc, const double *ar, const double *ac,
                             const double *bc, const double *dc, int coef_batched, const double *x, int64_t x_bs,
                             const double *diag, double *a, double *U, double *V, c2_stream_t stream);

/* Term.get_value on two grids -- python/celerite2/terms.py:58-79 evaluated at
 * tau = t1[n] - t2[m]: K[b, n, m] = sum_r ar e^{-cr |tau|} + sum_k e^{-cc |tau|}
 * (ac cos(dc |tau|) + bc sin(dc |tau|)).  What the conditional distribution
 * forms before it calls the solves (core.py:46-54 KxsT, :142-148 the prior
 * covariance of the prediction grid).  Coefficients shared or per series
 * (coef_batched); t1 (B,N) / shared (N,) via t1_bs, t2 (B,M) / (M,) via t2_bs;
 * K (B,N,M). */
int c2_kernel_values(int64_t B, int64_t N, int64_t M, int64_t Jr, int64_t Jc, const double *ar, const double *cr,
                     const double *ac, const double *bc, const double *cc, const double *dc, int coef_batched,
                     const double *t1, int64_t t1_bs, const double *t2, int64_t t2_bs, double *K, c2_stream_t stream);

/* out[b, m] = sum_n Z[b, n, m]^2 / d[b, n]  (Z (B,N,M), d (B,N), out (B,M)): the quadratic form of the PREDICTIVE VARIANCE,
 * core.py:134-140 `kernel.get_value(0) - diagdot(KxsT, Kinv_KxsT)` (numpy.py:24-25), evaluated from the lower solve alone:
 * with K = L D L^T, diag(Kxs K^-1 Kxs^T)_m = sum_n (L^-1 KxsT)_nm^2 / d_n -- Z = c2_solve_lower(KxsT); the reference reaches
 * the same number through apply_inverse (both solves) and a second pass over the two N x M arrays.  Any B: beyond 65535
 * series the blocks stride over the batch. */
int c2_colsumsq_over_d(int64_t B, int64_t N, int64_t M, const double *Z, const double *d, double *out, c2_stream_t stream);

/* Fused log-likelihood -- the assembly the reference's callers perform around
 * factor + solve_lower (python/celerite2/numpy.py:66-87,104-109, core.py:407-428):
 *   ll[b] = -1/2 (sum log d + N log 2pi) - 1/2 sum z^2/d,  z = L^-1 y.
 * No d/W/z is materialised.  flag[b] != 0 -> ll[b] = -inf (numpy.py:78-82). */
int c2_loglik(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
              const double *a, const double *U, const double *V, const double *y, double *ll, int32_t *flag,
              c2_stream_t stream);

/* Fused log-likelihood + reverse-mode gradient w.r.t. (t, c, a, U, V, y): the
 * chain factor_fwd -> solve_lower_fwd -> [seeds] -> solve_lower_rev -> factor_rev
 * an autodiff frontend runs (python/celerite2/pymc/ops.py:104-141,
 * pymc/distribution.py:123-128), with per-series outputs bt (B,N), bc (B,J),
 * ba (B,N), bU (B,N,J), bV (B,N,J), by (B,N).  `work` is caller-provided device
 * scratch of c2_loglik_grad_workspace_bytes(B,N,J) bytes (the query follows the
 * dispatch: checkpoints + W rows + (d,z) records for the row-by-row kernels, lane-major
 * records for chip-filling batches, d / W / z / state rows / chunk maps for small
 * batches of long series, which run parallel along time).
 * Agreement with the reference's operation order: the row-by-row forward passes repeat
 * it up to FMA contraction and reduction order (1e-13 on well-conditioned data); their
 * reverse sweeps recover the forward state S_n, F_n of reverse.hpp:52-84 / internal.hpp:225-245
 * by running forward.hpp:115-123 backward from a checkpoint at most 32 rows up wherever the
 * decays in between can be inverted (c_max * span <= 2: errors grow by at most e^4), and by
 * replaying the forward steps from a checkpoint where they cannot (gaps in time) -- decided
 * on the device, per wavefront; gradients within 1e-10 of the largest
 * entry of their array either way (1.5e-11 between the two forms on the bench's batch);
 * small batches of long series run PARALLEL ALONG TIME, verified
 * on the device -- what every chunk arrives at is compared with what its
 * neighbour was given, and the row-by-row kernels recompute the batch behind
 * that gate should they disagree beyond 2e-12 -- and are held to
 *   |x - x_ref| <= 1e-10 max|x_ref| + 4 max|x_ref - x_ext|   per gradient array,
 * x_ext = the reference recursion evaluated in extended precision: a float64
 * evaluation in ANY order (the reference's own included) moves by ~0.4 eps
 * kappa^2 of the largest entry, kappa = max a_n / d_n; chunked sums reorder the
 * additions, so entries far below the largest of their array are sums of large
 * terms (profiles/r03_timepar_verification.md; option timepar_cond_limit).
 * A series whose factorisation fails (flag[b] != 0; the reference raises,
 * driver.hpp:13-19) gets ll[b] = -inf and ALL SIX gradients filled with NaN
 * -- defined, never stale memory; the other series of the batch are unaffected. */
size_t c2_loglik_grad_workspace_bytes(int64_t B, int64_t N, int64_t J);
int c2_loglik_grad(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                   const double *a, const double *U, const double *V, const double *y, double *ll, double *bt,
                   double *bc, double *ba, double *bU, double *bV, double *by, int32_t *flag, void *work,
                   size_t work_bytes, c2_stream_t stream);

/* Conditioning of the factorisation, per series: kappa[b] = max_n a_n / d_n (+inf where the factorisation fails,
 * flag[b] = the failing row as in c2_factor).  d_n = a_n - U_n S_n U_n^T (forward.hpp:126-128) is a difference: a
 * float64 evaluation of the recursion IN ANY ORDER -- the reference's own included -- carries a rounding error of
 * ~0.4 eps kappa^2 relative to the largest entry of a gradient array (oracle vs its own extended-precision
 * evaluation: tests/test_oracle.py, tools/kappa_sweep.py).  north_star's 1e-10 agreement with the reference is
 * therefore attainable where kappa <~ 1e3 (0.4 * 2.2e-16 * kappa^2 <= 1e-10): a caller who needs to know whether a
 * result can be held to that tolerance asks here.  (bench.py reports the timed batch's largest kappa; the synthetic
 * series of SURVEY.md 8d at N = 4096, J = 8 sit at kappa ~ 290 median, 380 at most: a floor of 1.3e-11.)  Replaces nothing in the reference (which reports no conditioning);
 * costs one `factor` pass on library temporaries (slices of 4096 series). */
int c2_condition(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                 const double *a, const double *U, const double *V, double *kappa, int32_t *flag, c2_stream_t stream);

/* 2-D (multi-band) extension, rank-1 band covariance K = T (x) alpha alpha^T + diag over N epochs x M bands
 * (observations interleaved epoch-major: row n*M + m).  EXTENSION -- the reference has no 2-D code (no core2.hpp;
 * README.md:14-17 only cites the paper), so this entry point replaces nothing and its parity is pinned by the dense
 * Kronecker matrix and by the 1-D recursions on the interleaved series, not by the reference.
 * Inputs: the 1-D celerite matrices of the EPOCH grid built with zero white noise -- t (B,N)|(N,), c (B,J)|(J,),
 * a (B,N) = k(0), U, V (B,N,J) -- plus alpha (B,M)|(M,) (alpha_bs = M or 0), diag (B,N,M) and y (B,N,M).
 * method: C2_KRON_COLLAPSED (each epoch's M bands fold into one effective observation; needs diag > 0; the
 * recursion runs over N rows) or C2_KRON_INTERLEAVED (the 1-D recursions on the N*M series with U' = U (x) alpha).
 * flag[b]: first failing row in the method's own series (epoch index / interleaved row), -1 for a non-positive
 * band variance under the collapsed method -- or for alpha == 0 in every band (the collapse divides by A = sum alpha^2 /
 * D: an epoch whose bands carry no signal has no effective observation; the interleaved method has no such restriction).  Gradients: bt (B,N), bc (B,J), ba (B,N), bU, bV (B,N,J),
 * balpha (B,M) (per series, also when alpha is shared), bdiag (B,N,M), by (B,N,M).  Any B: beyond 65535 series the
 * blocks of the collapse and fold kernels stride over the batch. */
#define C2_KRON_COLLAPSED 0
#define C2_KRON_INTERLEAVED 1
size_t c2_kron_loglik_workspace_bytes(int64_t B, int64_t N, int64_t M, int64_t J, int method, int grad);
int c2_kron_loglik(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *c,
                   int64_t c_bs, const double *a, const double *U, const double *V, const double *alpha,
                   int64_t alpha_bs, const double *diag, const double *y, double *ll, int32_t *flag, int method,
                   void *work, size_t work_bytes, c2_stream_t stream);
int c2_kron_loglik_grad(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *c,
                        int64_t c_bs, const double *a, const double *U, const double *V, const double *alpha,
                        int64_t alpha_bs, const double *diag, const double *y, double *ll, double *bt, double *bc,
                        double *ba, double *bU, double *bV, double *balpha, double *bdiag, double *by, int32_t *flag,
                        int method, void *work, size_t work_bytes, c2_stream_t stream);

/* Log-likelihood (+ gradient) from the celerite COEFFICIENTS: the chain
 * get_celerite_matrices (driver.cpp:422-477, terms.py:117-177) -> factor -> solve_lower -> reductions and its
 * reverse, which the reference's jax / pymc frontends obtain by autodiff of their term code
 * (python/celerite2/jax/terms.py, pymc/terms.py), kept on the device.  Coefficients ar, cr (B,Jr), ac, bc, cc, dc
 * (B,Jc), all per series (coef_batched = 1) or all shared by the batch (0); x (B,N) / shared (N,) via x_bs;
 * diag, y (B,N).  J = Jr + 2 Jc <= C2_MAX_WIDTH.  Gradients (per series, also for shared coefficients):
 * bar, bcr (B,Jr); bac, bbc, bcc, bdc (B,Jc); bx, bdiag, by (B,N).  A failed series: ll = -inf, NaN gradients.
 * Widths J = 8, 4, 2 and chip-filling batches run kernels that form U_n, V_n inside the recursion (no matrices in memory);
 * everything else the composed chain on matrices kept in `work` (same results).  `work` is
 * sized for either. */
size_t c2_loglik_terms_workspace_bytes(int64_t B, int64_t N, int64_t Jr, int64_t Jc, int grad);
int c2_loglik_terms(int64_t B, int64_t N, int64_t Jr, int64_t Jc, const double *ar, const double *cr, const double *ac,
                    const double *bc, const double *cc, const double *dc, int coef_batched, const double *x,
                    int64_t x_bs, const double *diag, const double *y, double *ll, int32_t *flag, void *work,
                    size_t work_bytes, c2_stream_t stream);
int c2_loglik_terms_grad(int64_t B, int64_t N, int64_t Jr, int64_t Jc, const double *ar, const double *cr,
                         const double *ac, const double *bc, const double *cc, const double *dc, int coef_batched,
                         const double *x, int64_t x_bs, const double *diag, const double *y, double *ll, double *bar,
                         double *bcr, double *bac, double *bbc, double *bcc, double *bdc, double *bx, double *bdiag,
                         double *by, int32_t *flag, void *work, size_t work_bytes, c2_stream_t stream);

/* Term HYPER-PARAMETERS on the device (csrc/c2_term_params.hip): what the reference's jax / pymc frontends get by
 * autodiff through their term classes (python/celerite2/jax/terms.py, pymc/terms.py).  A model is a PROGRAM, the flattened
 * sum of terms (terms.py:233-235), passed by value: each record names its kind, its parameterisation, the columns of the
 * parameter matrix P (B,NP) | shared (NP,) (p_bs = NP or 0) it reads, and its first real / complex coefficient slot
 * (jr, jc: slots in program order, reals and complex terms each concatenated, as TermSum.get_coefficients does).
 *   C2_TERM_REAL      col = (a, c)                       terms.py:515-521   1 real slot
 *   C2_TERM_COMPLEX   col = (a, b, c, d)                 terms.py:554-569   1 complex slot
 *   C2_TERM_SHO       col = (S0|sigma, w0|rho, Q|tau)    terms.py:644-691   par = OR of C2_SHO_SIGMA / _RHO / _TAU
 *   C2_TERM_MATERN32  col = (sigma, rho)                 terms.py:729-745   1 complex slot
 *   C2_TERM_ROTATION  col = (sigma, period, Q0, dQ, f)   terms.py:791-812   2 complex slots
 * SHO regime: C2_SHO_UNDER (1 complex slot) / C2_SHO_OVER (2 real slots): the whole batch on one side of Q = 1/2
 * (terms.py:691), a series on the wrong side gets flag[b] = 1 + its term's index; C2_SHO_MIXED: 2 real AND 1 complex
 * slot (width 4 instead of 2), each series fills the side its Q selects and the other side gets amplitudes 0, the rate
 * w0 / 2Q and dc = 0.  eps as in the reference (sqrt(max(., eps)); where it clamps nothing flows through f in reverse).
 * Widths: Jr + 2 Jc <= 32, what c2_loglik_terms takes. */
#define C2_TERM_REAL 0
#define C2_TERM_COMPLEX 1
#define C2_TERM_SHO 2
#define C2_TERM_MATERN32 3
#define C2_TERM_ROTATION 4
#define C2_SHO_SIGMA 1
#define C2_SHO_RHO 2
#define C2_SHO_TAU 4
#define C2_SHO_UNDER 0
#define C2_SHO_OVER 1
#define C2_SHO_MIXED 2
#define C2_TERMS_MAX 16
#define C2_FLAG_REGIME (-2)
typedef struct {
  int32_t kind, par, regime, jr, jc;
  int32_t col[5];
  double eps;
} c2_term_rec;
typedef struct {
  int32_t nterms, np, Jr, Jc;
  c2_term_rec term[C2_TERMS_MAX];
} c2_term_program;
/* P -> ar, cr (B,Jr), ac, bc, cc, dc (B,Jc) (always per series: coef_batched = 1 downstream) and flag (B,). */
int c2_term_coefficients(const c2_term_program *prog, int64_t B, const double *P, int64_t p_bs, double *ar, double *cr,
                         double *ac, double *bc, double *cc, double *dc, int32_t *flag, c2_stream_t stream);
/* The reverse: cotangents bar .. bdc (what c2_loglik_terms_grad writes) -> bP (B,NP), per series also for a shared P.
 * tflag (nullable): the flag of c2_term_coefficients; lflag (nullable): the flag of c2_loglik_terms_grad; ll (nullable).
 * A series with tflag != 0 gets a zero row, ll = -inf and lflag = C2_FLAG_REGIME; one with lflag != 0 a zero row. */
int c2_term_coefficients_rev(const c2_term_program *prog, int64_t B, const double *P, int64_t p_bs, const double *bar,
                             const double *bcr, const double *bac, const double *bbc, const double *bcc,
                             const double *bdc, const int32_t *tflag, int32_t *lflag, double *ll, double *bP,
                             c2_stream_t stream);
/* The two hyper-parameters every model has (core.py:262-310: diag = yerr^2 + ..., core.py:407-428: y - mean), one pass:
 * diag[b,n] = (yerr_is_sigma ? yerr[b,n]^2 : yerr[b,n]) + jitter[b]^2, r[b,n] = y[b,n] - mean[b].  jitter, mean (B,),
 * nullable (= 0).  The outputs must not alias the inputs. */
int c2_noise_mean_apply(int64_t B, int64_t N, const double *yerr, int yerr_is_sigma, const double *jitter,
                        const double *mean, const double *y, double *diag, double *r, c2_stream_t stream);
/* ... and its reverse, one pass over bdiag and by (B,N) with a fixed summation order (deterministic):
 * bjitter[b] = 2 jitter[b] sum_n bdiag[b,n], bmean[b] = -sum_n by[b,n]; either output may be NULL; a series with
 * flag[b] != 0 (nullable) gets zeros. */
int c2_noise_mean_rev(int64_t B, int64_t N, const double *jitter, const double *bdiag, const double *by,
                      const int32_t *flag, double *bjitter, double *bmean, c2_stream_t stream);

/* TERM ALGEBRA on the device (csrc/c2_term_expr.hip): sums, PRODUCTS (terms.py:238-301), DERIVATIVES (terms.py:304-330)
 * and the exposure-time CONVOLUTION (terms.py:333-410) of the five term kinds above.  A product of two celerite kernels is
 * again a celerite kernel, so all of it is a map parameters -> coefficients in front of c2_loglik_terms[_grad]; only the
 * convolution adds something new, one number per series: `shift`, which the caller adds to the diagonal
 * (c2_noise_mean_shift_apply) and whose cotangent is the row sum of bdiag (c2_noise_mean_shift_rev).
 *
 * An EXPRESSION (c2_term_expr, passed by value to the kernels like c2_term_program) is the leaf program followed by
 * operation records in post-order.  Coefficients live in REGISTERS: real register k holds one (ar, cr) pair, complex
 * register k one (ac, bc, cc, dc) quadruple.  The leaves fill real registers [0, leaves.Jr) and complex registers
 * [0, leaves.Jc) (their jr / jc, exactly as in the flat program, but without its width limit); operation i reads the
 * register ranges a and b (b unused by DIFF and CONVOLVE) and writes `out`, which starts at the first register no leaf
 * and no earlier operation wrote (so a result never overlaps anything still needed, and every register is written once):
 *   C2_OP_SUM       out = a followed by b                                  out.nr = a.nr + b.nr, out.nc = a.nc + b.nc
 *   C2_OP_PRODUCT   reals a x b; complex: real(a) x complex(b), real(b) x complex(a), then per complex pair the
 *                   (dj - dk) and the (dj + dk) term                       out.nr = a.nr b.nr,
 *                                                                          out.nc = a.nr b.nc + b.nr a.nc + 2 a.nc b.nc
 *   C2_OP_DIFF      ar <- -ar cr^2; (a, b) <- (a (d^2 - c^2) + 2 b c d, b (d^2 - c^2) - 2 a c d); same sizes
 *   C2_OP_CONVOLVE  boxcar of width delta = P[col] (data: its column of bP stays 0); same sizes; LAST operation only;
 *                   shift[b] = delta_diag of terms.py:350-380
 * The result of the expression is `out` of the last operation (the leaf registers themselves when nops = 0); its width
 * out.nr + 2 out.nc <= 32.  NR / NC = registers in all (leaves + results), at most C2_EXPR_REGS_MAX each.
 * The registers are kept in the caller's `work` buffer as [field of register][series] (consecutive lanes, consecutive
 * addresses): 2 NR + 4 NC doubles per series forward, twice that in reverse (values + cotangents). */
#define C2_OP_SUM 0
#define C2_OP_PRODUCT 1
#define C2_OP_DIFF 2
#define C2_OP_CONVOLVE 3
#define C2_EXPR_OPS_MAX 16
#define C2_EXPR_REGS_MAX 256
typedef struct {
  int32_t r0, nr, c0, nc; /* real registers [r0, r0 + nr), complex registers [c0, c0 + nc) */
} c2_term_range;
typedef struct {
  int32_t op, col; /* col: CONVOLVE only, the column of P that holds delta */
  c2_term_range a, b, out;
} c2_term_op;
typedef struct {
  c2_term_program leaves;
  int32_t nops, NR, NC, reserved;
  c2_term_op op[C2_EXPR_OPS_MAX];
} c2_term_expr;
/* Bytes of `work` for B series (the reverse's need; the forward takes half). 0 for an invalid expression. */
size_t c2_term_expr_workspace_bytes(const c2_term_expr *expr, int64_t B);
/* P -> the coefficients of the expression's result, (B,Jr) / (B,Jc) with (Jr, Jc) = (out.nr, out.nc) of the last
 * operation, shift (B,) (0 without a convolution) and flag (B,) as c2_term_coefficients (a leaf SHO on the wrong side). */
int c2_term_expr_coefficients(const c2_term_expr *expr, int64_t B, const double *P, int64_t p_bs, double *ar, double *cr,
                              double *ac, double *bc, double *cc, double *dc, double *shift, int32_t *flag, void *work,
                              size_t work_bytes, c2_stream_t stream);
/* The reverse: the forward is replayed into `work`, the operation records are reversed (last to first) into cotangents of
 * the leaf registers, then the leaves as c2_term_coefficients_rev.  bshift (B,) nullable (= 0).  tflag / lflag / ll are
 * settled as in c2_term_coefficients_rev. */
int c2_term_expr_coefficients_rev(const c2_term_expr *expr, int64_t B, const double *P, int64_t p_bs, const double *bar,
                                  const double *bcr, const double *bac, const double *bbc, const double *bcc,
                                  const double *bdc, const double *bshift, const int32_t *tflag, int32_t *lflag,
                                  double *ll, double *bP, void *work, size_t work_bytes, c2_stream_t stream);
/* c2_noise_mean_apply with one more per-series term: diag[b,n] = yerr[b,n]^2 (or yerr[b,n]) + jitter[b]^2 + shift[b]
 * (shift nullable = the kernel without it, bit for bit) ... */
int c2_noise_mean_shift_apply(int64_t B, int64_t N, const double *yerr, int yerr_is_sigma, const double *jitter,
                              const double *mean, const double *shift, const double *y, double *diag, double *r,
                              c2_stream_t stream);
/* ... and c2_noise_mean_rev with bshift[b] = sum_n bdiag[b,n] (the row sum bjitter is formed from: same fixed order, no
 * atomics); any of the three outputs may be NULL; a series with flag[b] != 0 or tflag[b] != 0 (both nullable) gets zeros. */
int c2_noise_mean_shift_rev(int64_t B, int64_t N, const double *jitter, const double *bdiag, const double *by,
                            const int32_t *flag, const int32_t *tflag, double *bjitter, double *bmean, double *bshift,
                            c2_stream_t stream);

/* dot_tril -- python/celerite2/numpy.py:100-102: Z = Y * sqrt(d)[:,None];
 * Z += tril(U W^T) Z.  Y == Z allowed. */
int c2_dot_tril(int64_t B, int64_t N, int64_t J, int64_t nrhs, const double *t, int64_t t_bs, const double *c,
                int64_t c_bs, const double *U, const double *W, const double *d, const double *Y, double *Z,
                c2_stream_t stream);

/* Diagonal of the inverse of the factored matrix, q[b, n] = [(K + D)^-1]_nn, from d, W of c2_factor in ONE backward sweep
 * with a symmetric J x J state (csrc/c2_invdiag.hip; O(N J^2) per series, the cost class of factor).  No counterpart in
 * the reference, whose predictive variance at the observed times solves against the N x N cross-covariance
 * (core.py:134-140) and which has no leave-one-out entry point; parity is pinned by the dense inverse.  With D the
 * diagonal the caller added to the kernel:  variance of the process at the data = D_n - D_n^2 q_n;  leave-one-out mean
 * y_n - alpha_n / q_n and variance 1 / q_n.  With z (B,N) -- the c2_solve_lower output of the residual -- the same pass
 * also carries the one-column upper solve alpha = L^-T (z / d) = (K + D)^-1 (y - mean) (forward.hpp:193-207): it reads
 * the same t, U, W, d rows in the same order.  z and alpha are both given or both NULL; alpha may alias z, and that is
 * the only aliasing allowed (q must not alias d, z or alpha; alpha must not alias d).  Rows of a series whose factorisation failed hold garbage (never another series'). */
int c2_inverse_diag(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                    const double *U, const double *W, const double *d, const double *z /* nullable */, double *q,
                    double *alpha /* nullable iff z is */, c2_stream_t stream);

/* c2_inverse_diag that also stores what its reverse pass reads (the pattern of c2_factor's S): for every row n the state
 * ENTERING it, before the row's decay is applied --
 *   Mws (B,N,J,J): Mws[b,n,j,:] is column j of the symmetric M behind row n (zeros at n = N-1);
 *   Fws (B,N,J), with z only: the upper solve's F behind row n, u_{n+1} alpha_{n+1} already added (zeros at n = N-1).
 * 8 B N J (J + 1) bytes, written once: 2.4 MB per series at N = 4096, J = 8 -- callers with large batches chunk the batch.
 * q and alpha have the bits c2_inverse_diag gives.  z, alpha, Fws are all given or all NULL.  No output may alias an
 * input or another output (alpha == z is NOT allowed here: the reverse pass reads z).  J <= C2_FAST_WIDTH; wider models
 * return C2_ERR_UNSUPPORTED.  No atomics, no allocation, no host read: capturable. */
int c2_inverse_diag_fwd(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                        const double *U, const double *W, const double *d, const double *z /* nullable */, double *q,
                        double *alpha /* nullable iff z is */, double *Mws, double *Fws /* nullable iff z is */,
                        c2_stream_t stream);
/* The reverse of c2_inverse_diag (csrc/c2_invdiag_rev.hip): cotangents bq (B,N) of q and balpha (B,N) of alpha
 * (nullable iff z is) -> bt (B,N), bc (B,J), bU, bW (B,N,J), bd (B,N), bz (B,N; nullable iff z is), per series also when
 * t or c is shared by the batch (the caller sums).  One upward sweep, n = 0 .. N-1, with a symmetric J x J adjoint state;
 * q, alpha, Mws, Fws: what c2_inverse_diag_fwd returned for the same t, c, U, W, d, z.  No output may alias an input or
 * another output.  J <= C2_FAST_WIDTH; wider models return C2_ERR_UNSUPPORTED.  Every output element has one writer: no
 * atomics (two calls give identical bits), no allocation, no host read: capturable.  Rows of a series whose factorisation
 * failed hold garbage (never another series'). */
int c2_inverse_diag_rev(int64_t B, int64_t N, int64_t J, const double *t, int64_t t_bs, const double *c, int64_t c_bs,
                        const double *U, const double *W, const double *d, const double *z /* nullable */, const double *q,
                        const double *alpha /* nullable iff z is */, const double *Mws,
                        const double *Fws /* nullable iff z is */, const double *bq,
                        const double *balpha /* nullable iff z is */, double *bt, double *bc, double *bU, double *bW,
                        double *bd, double *bz /* nullable iff z is */, c2_stream_t stream);

/* The reverse of c2_get_celerite_matrices (csrc/c2_terms.hip, the kernel inside c2_loglik_terms_grad): cotangents
 * bt (B,N), bcv (B,J), ba (B,N), bU, bV (B,N,J) of (t, c, a, U, V), with J = Jr + 2 Jc and V the matrix the forward call
 * returned (it holds the cos / sin of the phases) -> bar, bcr (B,Jr), bac, bbc, bcc, bdc (B,Jc), per series also when the
 * coefficients are shared, bx (B,N) = bt + the phases' part, bdiag (B,N) = ba.  Sums in a fixed order: two calls give
 * identical bits.  A handful of long series (B < 64, N >= 8192) is split over slices of the rows and needs `work` of
 * c2_get_celerite_matrices_rev_workspace_bytes (0 otherwise; work may then be NULL).  No output may alias an input or
 * another output.  J <= C2_FAST_WIDTH. */
size_t c2_get_celerite_matrices_rev_workspace_bytes(int64_t B, int64_t N, int64_t Jr, int64_t Jc);
int c2_get_celerite_matrices_rev(int64_t B, int64_t N, int64_t Jr, int64_t Jc, const double *ac, const double *bc,
                                 const double *dc, int coef_batched, const double *x, int64_t x_bs, const double *V,
                                 const double *bt, const double *bcv, const double *ba, const double *bU,
                                 const double *bV, double *bar, double *bcr, double *bac, double *bbc, double *bcc,
                                 double *bdc, double *bx, double *bdiag, void *work, size_t work_bytes,
                                 c2_stream_t stream);

/* Explained variance at NEW times, r[b, m] = k*_m^T (K + D)^-1 k*_m for M sorted query times ts against the matrix
 * c2_factor factored on the N sorted data times t (csrc/c2_predvar.hip): the predictive variance of the process at ts is
 * k(0) - r.  Two stream-ordered sweeps over the merge of the two grids -- the forward state of c2_factor rebuilt from d, W,
 * then the backward state of c2_inverse_diag -- O((N + M) J^2) work and O((N + M) J) memory per series.  No counterpart in
 * the reference, which forms the N x M cross-covariance and solves against M right-hand sides (core.py:134-140); parity is
 * pinned by dense algebra and by the reference's own predictive variances.  Us, Vs (B,M,J): the U and V rows of the
 * queries (c2_get_celerite_matrices at ts); U, W, d: the data's, as c2_inverse_diag takes them.  ts_bs: batch stride of
 * ts like t_bs (0 = shared).  A query at a data time may fall on either side of it: the value is the same.
 * work: caller-owned, B * M * J doubles, overwritten.  r (B,M) and work must not alias any input or each other.
 * J <= C2_FAST_WIDTH; wider models return C2_ERR_UNSUPPORTED.  No atomics (two calls give identical bits), no
 * allocation, no host read: capturable.  Rows of a series whose factorisation failed hold garbage (never another series'). */
int c2_explained_variance(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *ts,
                          int64_t ts_bs, const double *c, int64_t c_bs, const double *U, const double *W, const double *d,
                          const double *Us, const double *Vs, double *r, double *work, c2_stream_t stream);

/* c2_explained_variance that also stores what its reverse pass reads: for every data row n the state AFTER its update --
 *   Sws (B,N,J,J): Sws[b,n,j,:] is column j of the forward state S'_n (the S of c2_factor after row n);
 *   Rws (B,N,J,J): Rws[b,n,j,:] is column j of the backward state R_n (the M of c2_inverse_diag after row n).
 * 16 B N J^2 bytes, written once: 4.2 MB per series at N = 4096, J = 8 -- callers with large batches chunk the batch.
 * r and work have the bits c2_explained_variance gives.  No output may alias an input or another output.
 * J <= C2_FAST_WIDTH; wider models return C2_ERR_UNSUPPORTED.  No atomics, no allocation, no host read: capturable. */
int c2_explained_variance_fwd(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *ts,
                              int64_t ts_bs, const double *c, int64_t c_bs, const double *U, const double *W,
                              const double *d, const double *Us, const double *Vs, double *r, double *work, double *Sws,
                              double *Rws, c2_stream_t stream);
/* The reverse of c2_explained_variance (csrc/c2_predvar_rev.hip): the cotangent br (B,M) of r -> bt (B,N), bts (B,M),
 * bc (B,J), bU, bW (B,N,J), bd (B,N), bUs, bVs (B,M,J), per series also when t, ts or c is shared by the batch (the caller
 * sums); every element is overwritten.  work, Sws, Rws: what c2_explained_variance_fwd wrote for the same arguments; the
 * states are read, never re-derived.  With n(m) the last data row with t_n <= s_m (-1 in front of the data), two
 * stream-ordered launches over the merge of the two grids:
 *   pass A walks upwards with the adjoint Rb = 0 of the backward state (a query before the data row above it):
 *     query m, n(m) = n-1:  lag = t_n - s, eps = exp(-c lag), x = eps o X_m;  Rb += br_m x x^T;  bx = 2 br_m R_n x;
 *                           bVs_m = eps o bx;  k = x o bx;  bc -= lag k;  bt_n -= c.k;  bts_m += c.k
 *     data n:  p = exp(-c (t_{n+1} - t_n)), G = (p p^T) o R_{n+1} (n = N-1: G = 0, p = 1);  g = G w;  q = 1/d_n + w.g;
 *              Mu = Rb u;  qb = u.Mu;  gb = -2 Mu + qb w;  bU_n = -2 Rb g + 2 q Mu;  bd_n = -qb / d_n^2;  bW_n = qb g + G gb;
 *              Gb = Rb + (gb w^T + w gb^T) / 2;  n < N-1: pb = 2 (Gb o R_{n+1}) p, k = pb o p, bc -= (t_{n+1} - t_n) k,
 *              bt_{n+1} -= c.k, bt_n += c.k;  Rb <- (p p^T) o Gb
 *   pass B walks downwards with the adjoint Sb = 0 of the forward state (a query before the data row below it) and adds to
 *   what pass A wrote:
 *     query m, n(m) = n >= 0:  lag = s - t_n, e = exp(-c lag), uL = u* o e, h = S'_n uL, bX = bVs_m;
 *                              bh = br_m uL - e o bX;  be = -h o bX;  buL = br_m h + S'_n bh;  Sb += (bh uL^T + uL bh^T) / 2;
 *                              bUs_m = e o buL;  be += u* o buL;  k = e o be;  bc -= lag k;  bts_m -= c.k;  bt_n += c.k
 *     data n:  bd_n += w^T Sb w;  bW_n += 2 d_n Sb w;  n > 0: p = exp(-c (t_n - t_{n-1})), pb = 2 (Sb o S'_{n-1}) p,
 *              k = pb o p, bc -= (t_n - t_{n-1}) k, bt_n -= c.k, bt_{n-1} += c.k, Sb <- (p p^T) o Sb
 * Queries with no data row above them get bVs = 0 exactly, queries in front of the data bUs = 0 exactly.  bc is summed
 * event by event from these non-negative lags.  No output may alias an input or another output.  J <= C2_FAST_WIDTH; wider
 * models return C2_ERR_UNSUPPORTED.  A fixed order, no atomics (two calls give identical bits), no allocation, no host
 * read: capturable.  Rows of a series whose factorisation failed hold garbage (never another series'). */
int c2_explained_variance_rev(int64_t B, int64_t N, int64_t M, int64_t J, const double *t, int64_t t_bs, const double *ts,
                              int64_t ts_bs, const double *c, int64_t c_bs, const double *U, const double *W,
                              const double *d, const double *Us, const double *Vs, const double *work, const double *Sws,
                              const double *Rws, const double *br, double *bt, double *bts, double *bc, double *bU,
                              double *bW, double *bd, double *bUs, double *bVs, c2_stream_t stream);

/* Joint draw of the NOISE-FREE prior process on the merge of the N sorted data times t and the M sorted query times ts
 * (csrc/c2_priordraw.hip): ft (B,N,K) and fs (B,M,K) = the Cholesky factor of the zero-noise kernel matrix on the merged
 * grid (data first on a tie) applied to the standard normals nt (B,N,K), ns (B,M,K) -- K independent draws per series.
 * It is the missing piece of a posterior draw at new times by Matheron's rule,
 * fs + K(ts, t) (K + D)^-1 (y - mean - ft - sqrt(D) ne), whose other steps are c2_solve_lower / c2_solve_upper and
 * c2_general_matmul_lower / _upper.  One forward sweep, O((N + M) (J^2 + J K)) work per series, nothing stored per row.  No
 * counterpart in the reference, which factors the dense M x M conditional covariance (numpy.py:27-32); parity is pinned
 * by dense algebra.  U, V (B,N,J) and Us, Vs (B,M,J): the kernel's rows at t and ts (c2_get_celerite_matrices; the
 * diagonal is not used).  A point whose pivot is <= 2^-44 k(0) -- one that coincides with an earlier point -- is
 * determined by the points in front of it and consumes no normal.  ft may alias nt and fs may alias ns (a row's normals
 * are read before its draw is stored); no other aliasing.  J <= C2_FAST_WIDTH; wider models return C2_ERR_UNSUPPORTED,
 * as do more than 65535 register blocks of draws (8 draws a block; 2 at J = 1).  One launch, no atomics (two calls give identical bits), no allocation, no host read: capturable. */
int c2_prior_draw(int64_t B, int64_t N, int64_t M, int64_t J, int64_t K, const double *t, int64_t t_bs, const double *ts,
                  int64_t ts_bs, const double *c, int64_t c_bs, const double *U, const double *V, const double *Us,
                  const double *Vs, const double *nt, const double *ns, double *ft, double *fs, c2_stream_t stream);

/* The reverse of c2_general_matmul_lower / _upper (csrc/c2_general_rev.hip): the cotangent bZ (B,N,nrhs) of Z ->
 * bt1 (B,N), bt2 (B,M), bc (B,J), bU (B,N,J), bV (B,M,J), bY (B,M,nrhs), per series also when t1, t2 or c is shared by the
 * batch (the caller sums); every element is overwritten.  No counterpart in the reference, whose backprop.cpp exports the
 * forward with its workspace and no reverse; parity is pinned by dense algebra.
 * Walk coordinates: position s = 0 .. M-1 along t2 and q = 0 .. N-1 along t1, with walk time tau = t and array row =
 * position (lower), tau = -t and array row = M-1-s / N-1-q (upper).  THE TIE RULE is the forward's: row s feeds output q
 * iff tau2[s] <= tau1[q] (lower) / tau2[s] < tau1[q] (upper); s(q) is the last position that feeds q.  Forward:
 *   F_0 = V_0^T Y_0,  F_s = p_s o F_{s-1} + V_s^T Y_s,  p_s = exp(-c (tau2[s] - tau2[s-1]));
 *   Z_q += (U_q o e_q) F_{s(q)},  e_q = exp(-c (tau1[q] - tau2[s(q)]))     (nothing if no row feeds q).
 * Reverse, with G = 0 (J x nrhs), walking the events backwards from the last position the forward absorbed:
 *   output q (s(q) = s):  bU_q = e_q o (F_s bZ_q),  bc -= (tau1[q] - tau2[s]) U_q o bU_q,  G += (U_q o e_q)^T bZ_q;
 *   row s:  bV_s = G Y_s,  bY_s = V_s G,  and for s >= 1  bc -= (tau2[s] - tau2[s-1]) rowsum(G o (F_s - V_s^T Y_s)),  G <- p_s o G;
 *   bt1_q = -+ c . (U_q o bU_q),  bt2_s = +- c . (V_s o bV_s)             (upper sign: lower variant).
 * bc is summed event by event from these non-negative lags (it does not cancel for times with a large offset).  Outputs
 * that no row feeds, and t2 rows behind the last output (never absorbed), get exact zeros.
 * THE WORKSPACE CONTRACT: F (B,M,J,nrhs) is what the forward call wrote for the same arguments (F != NULL there), by any of
 * its kernels.  It is read, never re-derived, and only at the rows the forward absorbed behind its start row: the start
 * row (array row 0, lower; M-1, upper, which the forward never writes) is formed from V and Y, and rows never absorbed may
 * hold anything.  No output may alias an input or another output.  J <= C2_FAST_WIDTH; wider models return
 * C2_ERR_UNSUPPORTED.  One launch per right-hand side on `stream`, each adding to what the one before wrote: a fixed
 * order, no atomics (two calls give identical bits), no allocation, no host read: capturable. */
int c2_general_matmul_lower_rev(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                                int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs,
                                const double *U, const double *V, const double *Y, const double *F, const double *bZ,
                                double *bt1, double *bt2, double *bc, double *bU, double *bV, double *bY,
                                c2_stream_t stream);
int c2_general_matmul_upper_rev(int64_t B, int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1,
                                int64_t t1_bs, const double *t2, int64_t t2_bs, const double *c, int64_t c_bs,
                                const double *U, const double *V, const double *Y, const double *F, const double *bZ,
                                double *bt1, double *bt2, double *bc, double *bU, double *bV, double *bY,
                                c2_stream_t stream);

/* ---------------------------------------------------------------------------
 * HOST entry points (B == 1, synchronous) -- what celerite2.driver /
 * celerite2.backprop bind.  Same argument meaning as the pybind11 functions of
 * python/celerite2/driver.cpp and backprop.cpp; shapes are passed explicitly.
 * c2h_factor returns C2_OK and stores the reference's flag in *flag.
 * ------------------------------------------------------------------------- */
int c2h_factor(int64_t N, int64_t J, const double *t, const double *c, const double *a, const double *U,
               const double *V, double *d, double *W, double *S /* nullable */, int64_t *flag);
int c2h_solve_lower(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                    const double *W, const double *Y, double *Z, double *F /* nullable */);
int c2h_solve_upper(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                    const double *W, const double *Y, double *Z, double *F /* nullable */);
int c2h_matmul_lower(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                     const double *V, const double *Y, double *Z, double *F /* nullable */, int zero_z);
int c2h_matmul_upper(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                     const double *V, const double *Y, double *Z, double *F /* nullable */, int zero_z);
int c2h_general_matmul_lower(int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1, const double *t2,
                             const double *c, const double *U, const double *V, const double *Y, double *Z,
                             double *F /* nullable */, int zero_z);
int c2h_general_matmul_upper(int64_t N, int64_t M, int64_t J, int64_t nrhs, const double *t1, const double *t2,
                             const double *c, const double *U, const double *V, const double *Y, double *Z,
                             double *F /* nullable */, int zero_z);
int c2h_factor_rev(int64_t N, int64_t J, const double *t, const double *c, const double *a, const double *U,
                   const double *V, const double *d, const double *W, const double *S, const double *bd,
                   const double *bW, double *bt, double *bc, double *ba, double *bU, double *bV);
int c2h_solve_lower_rev(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                        const double *W, const double *Y, const double *Z, const double *F, const double *bZ,
                        double *bt, double *bc, double *bU, double *bW, double *bY);
int c2h_solve_upper_rev(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                        const double *W, const double *Y, const double *Z, const double *F, const double *bZ,
                        double *bt, double *bc, double *bU, double *bW, double *bY);
int c2h_matmul_lower_rev(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                         const double *V, const double *Y, const double *Z, const double *F, const double *bZ,
                         double *bt, double *bc, double *bU, double *bV, double *bY);
int c2h_matmul_upper_rev(int64_t N, int64_t J, int64_t nrhs, const double *t, const double *c, const double *U,
                         const double *V, const double *Y, const double *Z, const double *F, const double *bZ,
                         double *bt, double *bc, double *bU, double *bV, double *bY);
int c2h_get_celerite_matrices(int64_t N, int64_t Jr, int64_t Jc, const double *ar, const double *ac,
                              const double *bc, const double *dc, const double *x, const double *diag, double *a,
                              double *U, double *V);

/* The c2h_* entry points stage their arguments through a per-thread device arena + pinned bounce buffer that is kept
 * between calls (memory beyond 256 MiB is given back when the call returns).  This releases everything the CALLING
 * thread holds; its next c2h_* call allocates again.  (The reference is stateless: nothing to replace.) */
void c2h_release_thread_cache(void);

#ifdef __cplusplus
}
#endif
#endif /* CELERITE2_AMD_H_ */
