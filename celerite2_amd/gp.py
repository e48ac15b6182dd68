# -*- coding: utf-8 -*-
"""Thin batched GaussianProcess frontend over the device ops.

Reproduces, for a batch of B independent series, what the reference's numpy backend does around the ops
(python/celerite2/numpy.py:66-121 and core.py:262-501): compute -> factor; log_likelihood -> solve_lower +
reductions; apply_inverse -> solve_lower, /d, solve_upper; dot_tril; sample; the conditional distribution
(core.py:9-150, numpy.py:14-32): mean at new coordinates via general_matmul_lower/upper, variance and covariance
via apply_inverse on the N x M cross-covariance (solves with M right-hand sides).  Everything stays on the GPU.
`log_likelihood_and_grad` exposes the fused kernels' gradients w.r.t. (t, c, a, U, V, y).
"""
import collections
import math

import torch

from . import ops

__all__ = ["GaussianProcess", "ConditionalDistribution", "LinearModelFit", "LinAlgError"]

LinearModelFit = collections.namedtuple("LinearModelFit", "beta cov log_likelihood marginal_log_likelihood residual")


class LinAlgError(Exception):
    pass


def _significance(self, kind, y, trials, shapes, draws, A, normalization, t_ref, dips_only, generator, normals, max_trials,
                  max_draws, nterms=1):
    """search_significance and shape_search_significance (`shapes`: its bank, None for the kinds named): what differs
    between the searches comes from significance.SEARCHES.  `nterms` = H > 1 (the periodogram): the multi-harmonic search,
    whose sweep and finish are harmonics.py's and whose per-draw statistic ops.harmonic_null_chi2 finishes in registers."""
    from . import _trial_fit, harmonics as hm, periodogram as pg, significance as sg

    self._need()
    self._check_vector(y)
    (B, N), dev = self._diag.shape, self._diag.device
    if shapes is None and kind not in sg.KINDS:
        raise ValueError("kind must be one of %s" % (sg.KINDS,))
    if normalization not in pg.NORMALIZATIONS:
        raise ValueError("normalization must be one of %s" % (pg.NORMALIZATIONS,))
    search, NS = sg.SEARCHES[kind], None
    if shapes is None:
        trials = sg.check_trials(kind, trials, B)
    else:
        trials, shapes, NS = self._shape_args(trials, shapes)
    if normals is not None:
        if not torch.is_tensor(normals) or normals.dim() != 3 or tuple(normals.shape[:2]) != (B, N):
            raise ValueError("Invalid shape: normals (must be (B, N, draws) = (%d, %d, draws))" % (B, N))
        draws = normals.shape[-1]
    draws = int(draws)
    if draws < 1:
        raise ValueError("draws must be at least 1")
    per_series = trials.dim() == (2 if kind == "periodogram" else 3)
    K = trials.shape[1 if per_series else 0]
    kstep = K if max_trials is None else int(max_trials)
    rstep = draws if max_draws is None else int(max_draws)
    if kstep < 1 or rstep < 1:
        raise ValueError("max_trials and max_draws must be at least 1")
    ok = self._flag == 0
    Z0 = self._whitened_columns(y, A)
    S0 = _trial_fit.null_products(Z0, self._d)
    if nterms > 1:
        T = ops.whitened_harmonics(self._t, self._c, self._U, self._W, self._d, Z0, trials, nterms, t_ref=t_ref)
        statistic, = self._nan_failed(hm.finish(S0, T, N, nterms, normalization, ok=ok).power)
        factors = hm.null_factors(S0, T, N, nterms, ok)                      # (what no draw changes: once)
    else:
        T = search.sweep(self._t, self._c, self._U, self._W, self._d, Z0, trials, t_ref=t_ref, shapes=shapes)
        statistic, = self._nan_failed(sg.observed_statistic(kind, S0, T, N, normalization, trials, NS, dips_only, ok))
    if normals is None:
        normals = torch.randn((B, N, draws), dtype=torch.float64, device=dev, generator=generator)
    rsd = torch.rsqrt(self._d)[..., None]
    ZA = Z0[..., :-1].transpose(1, 2)                                        # (B, P0, N)
    maxima = []
    for r0 in range(0, draws, rstep):
        n = normals[..., r0:r0 + rstep]
        scaled = (n * rsd).contiguous()                                      # D^-1/2 n_r
        s_yy, G0Y = (n * n).sum(dim=1), torch.matmul(ZA, scaled)
        alpha = ops.solve_upper(self._t, self._c, self._U, self._W, scaled)
        best = torch.full((B, n.shape[-1]), -math.inf, dtype=torch.float64, device=dev)
        if nterms > 1:
            V, chi2_0 = hm.null_draws(factors, G0Y, s_yy)
        for k0 in range(0, K, kstep):
            tk = (trials[:, k0:k0 + kstep] if per_series else trials[k0:k0 + kstep]).contiguous()
            if nterms > 1:
                Xt = None if factors.Xt is None else factors.Xt[:, k0:k0 + kstep].contiguous()
                dchi2 = ops.harmonic_null_chi2(self._t, alpha, tk, nterms, factors.Lm[:, k0:k0 + kstep].contiguous(), Xt, V,
                                               t_ref=t_ref)
                stat = hm.normalize(dchi2, chi2_0, normalization)
            else:
                P = search.project(self._t, alpha, tk, t_ref=t_ref, shapes=shapes)
                stat = sg._null_statistics(kind, S0, T[:, k0:k0 + kstep], G0Y, s_yy, P, N, normalization, tk, NS, dips_only, ok)
            best = torch.maximum(best, torch.where(torch.isnan(stat), best[:, None, :], stat).amax(dim=1))
        maxima.append(torch.where(torch.isinf(best) & (best < 0), torch.full_like(best, math.nan), best))
    null_maxima, = self._nan_failed(torch.cat(maxima, dim=1))
    # (a draw's maximum comes through the projection, the statistic through the sweep: a tie of the two to the standing
    # criterion's relative part counts as at or above -- the larger probability)
    return sg.Significance(statistic, sg.false_alarm_probability(statistic, null_maxima, rtol=1e-10), null_maxima)


class GaussianProcess:
    def __init__(self, kernel, t=None, *, mean=0.0, **kwargs):
        self.kernel = kernel
        self.mean = mean if torch.is_tensor(mean) else float(mean)   # (a 0-d device tensor stays where it is: log_likelihood_kernel differentiates it)
        self._t = None
        if t is not None:
            self.compute(t, **kwargs)

    # -- core.py:262-310 + numpy.py:66-92 -------------------------------------------------------------
    def compute(self, t, *, yerr=None, diag=None, check_sorted=True, quiet=False):
        if t.dim() not in (1, 2):
            raise ValueError("The input coordinates must be (N,) or (B, N)")
        if check_sorted and bool((t[..., 1:] < t[..., :-1]).any()):
            raise ValueError("The input coordinates must be sorted")
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        if yerr is not None:
            diag = yerr**2
        if diag is None:
            raise ValueError("'diag' or 'yerr' (B, N) is required: it defines the batch")
        if diag.dim() != 2:
            raise ValueError("diag / yerr must be (B, N)")
        if t.shape[-1] != diag.shape[-1] or (t.dim() == 2 and t.shape[0] != diag.shape[0]):
            raise ValueError("Invalid shape: t %s does not match diag %s" % (tuple(t.shape), tuple(diag.shape)))
        self._t, self._diag = t.contiguous(), diag.contiguous()
        self._size = t.shape[-1]
        self._c, self._a, self._U, self._V = self.kernel.get_celerite_matrices(self._t, self._diag)
        self._d, self._W, self._flag = ops.factor(self._t, self._c, self._a, self._U, self._V)
        failed = self._flag != 0
        if bool(failed.any()) and not quiet:
            raise LinAlgError("failed to factorize or solve matrix")
        log_det = torch.log(self._d).sum(dim=1)
        self._log_det = torch.where(failed, torch.full_like(log_det, -math.inf), log_det)
        self._norm = torch.where(failed, torch.full_like(log_det, math.inf),
                                 -0.5 * (log_det + self._size * math.log(2 * math.pi)))
        return self

    def _need(self):
        if self._t is None:
            raise RuntimeError("you must call 'compute' first")

    def _as_matrix(self, y):
        if y.dim() not in (2, 3) or tuple(y.shape[:2]) != tuple(self._diag.shape):
            raise ValueError("Invalid shape: y %s, expected (B, N) or (B, N, nrhs) with (B, N) = %s"
                             % (tuple(y.shape), tuple(self._diag.shape)))
        return (y[..., None], True) if y.dim() == 2 else (y, False)

    def _check_vector(self, y):
        if tuple(y.shape) != tuple(self._diag.shape):  # core.py:312-330 (_process_input)
            raise ValueError("Invalid shape: y %s, expected (B, N) = %s" % (tuple(y.shape), tuple(self._diag.shape)))

    # -- core.py:407-428 + numpy.py:104-109 -------------------------------------------------------------
    def log_likelihood(self, y):
        self._need()
        self._check_vector(y)
        r = (y - self.mean)[..., None].contiguous()
        z = ops.solve_lower(self._t, self._c, self._U, self._W, r)[..., 0]
        return self._norm - 0.5 * (z * z / self._d).sum(dim=1)

    def log_likelihood_fused(self, y):
        """Same value straight from the one-pass fused kernel (no d / W / z materialised)."""
        self._need()
        self._check_vector(y)
        ll, flag = ops.loglik(self._t, self._c, self._a, self._U, self._V, (y - self.mean).contiguous())
        return ll

    def log_likelihood_and_grad(self, y, work=None):
        """(ll, (bt, bc, ba, bU, bV, by), flag): gradients w.r.t. the celerite matrices and the data."""
        self._need()
        self._check_vector(y)
        return ops.loglik_grad(self._t, self._c, self._a, self._U, self._V, (y - self.mean).contiguous(), work=work)

    def log_likelihood_kernel(self, y, *, jitter=None):
        """ll (B,) of `y` as a differentiable function of the kernel's tensor hyper-parameters, of `jitter` (added in
        quadrature to the computed diagonal) and of a tensor `mean`: autograd.log_likelihood_kernel on this GP's t, diag
        and mean -- the coefficient-level kernels, not the matrices `compute` factored."""
        from . import autograd

        self._need()
        self._check_vector(y)
        return autograd.log_likelihood_kernel(self.kernel, self._t, y, diag=self._diag, jitter=jitter, mean=self.mean)

    # -- core.py:342-376 + numpy.py:94-98 ----------------------------------------------------------------
    def apply_inverse(self, y):
        self._need()
        Y, vec = self._as_matrix(y)
        z = ops.solve_lower(self._t, self._c, self._U, self._W, Y.contiguous())   # (a fresh array: the caller keeps y)
        z.div_(self._d[..., None])                                                 # ... scaled and solved again in place
        z = ops.solve_upper(self._t, self._c, self._U, self._W, z, Z=z)
        return z[..., 0] if vec else z

    # -- core.py:378-405 + numpy.py:100-102 --------------------------------------------------------------
    def dot_tril(self, y):
        self._need()
        Y, vec = self._as_matrix(y)
        z = ops.dot_tril(self._t, self._c, self._U, self._W, self._d, Y.contiguous())
        return z[..., 0] if vec else z

    # -- numpy.py:111-121 ------------------------------------------------------------------------------
    def sample(self, *, size=None, include_mean=True, generator=None):
        self._need()
        B, N = self._diag.shape
        k = 1 if size is None else size
        n = torch.randn((B, N, k), dtype=torch.float64, device=self._diag.device, generator=generator)
        out = self.dot_tril(n).transpose(1, 2)
        if include_mean:
            out = out + self.mean
        return out[:, 0] if size is None else out

    # -- the diagonal of (K + D)^-1 in linear time (ops.inverse_diag; no counterpart in the reference) ------------
    def _nan_failed(self, *xs):
        """Series whose factorisation failed (compute(..., quiet=True)) hold NaN."""
        failed = (self._flag != 0)[:, None]
        nan = torch.full((), math.nan, dtype=torch.float64, device=self._diag.device)
        return tuple(torch.where(failed, nan, x) for x in xs)

    def _q_alpha(self, y):
        self._check_vector(y)
        r = (y - self.mean)[..., None].contiguous()
        z = ops.solve_lower(self._t, self._c, self._U, self._W, r)[..., 0]   # (B, N): a view of a contiguous (B, N, 1)
        return ops.inverse_diag(self._t, self._c, self._U, self._W, self._d, z=z, alpha=z)

    def inverse_diagonal(self):
        """q (B, N): q[b, n] = [(K + D)^-1]_nn of the matrix `compute` factored, O(N J^2) per series."""
        self._need()
        return self._nan_failed(ops.inverse_diag(self._t, self._c, self._U, self._W, self._d))[0]

    def predict_observed(self, y, *, return_var=False, include_mean=True):
        """The conditional mean (B, N) of the process at the observed times, y - D alpha with alpha = (K + D)^-1 (y - mean),
        and with `return_var` its variance (B, N), D_n - D_n^2 q_n with q the diagonal of (K + D)^-1 -- from
        K (K + D)^-1 K = K - D + D (K + D)^-1 D.  One solve_lower and one inverse_diag pass: O(N J^2) per series, no
        N x N cross-covariance (`predict(y, return_var=True)` builds one and solves with N right-hand sides).

        This is the variance under the FACTORED matrix.  For every kernel but a TermConvolution that is the kernel itself
        and the result is `predict`'s; under a TermConvolution the factored matrix is the semiseparable form (exact for
        lags >= delta), whereas `predict` evaluates the piecewise kernel for its cross-covariance, so the two differ
        there and only there.  D is the diagonal given to `compute`."""
        self._need()
        q, alpha = self._q_alpha(y)
        mu = y - self._diag * alpha
        if not include_mean:
            mu = mu - self.mean
        if not return_var:
            return self._nan_failed(mu)[0]
        return self._nan_failed(mu, self._diag - self._diag * self._diag * q)

    def leave_one_out(self, y):
        """(mean, var), each (B, N): the predictive distribution of y_n from all the OTHER points,
        mean = y_n - alpha_n / q_n and var = 1 / q_n (the white noise of point n included)."""
        self._need()
        q, alpha = self._q_alpha(y)
        return self._nan_failed(y - alpha / q, 1.0 / q)

    def loo_log_predictive(self, y):
        """Leave-one-out log predictive density (B,), sum_n log N(y_n | mean_n, var_n) of `leave_one_out(y)`
        (Rasmussen & Williams 5.4.2): sum_n (log q_n - alpha_n^2 / q_n) / 2 - N log(2 pi) / 2, from one solve_lower and one
        inverse_diag pass.  Not differentiable (`loo_log_predictive_kernel` is); a failed series gets -inf."""
        self._need()
        q, alpha = self._q_alpha(y)
        v = 0.5 * (torch.log(q) - alpha * alpha / q).sum(dim=1) - 0.5 * self._size * math.log(2 * math.pi)
        return torch.where(self._flag != 0, torch.full_like(v, -math.inf), v)

    def loo_log_predictive_kernel(self, y, *, jitter=None):
        """The leave-one-out log predictive density (B,) of `y` as a differentiable function of the kernel's tensor
        hyper-parameters, of `jitter` and of a tensor `mean`: autograd.loo_log_predictive_kernel on this GP's t, diag and
        mean (as `log_likelihood_kernel` is for the marginal likelihood)."""
        from . import autograd

        self._need()
        self._check_vector(y)
        return autograd.loo_log_predictive_kernel(self.kernel, self._t, y, diag=self._diag, jitter=jitter, mean=self.mean)

    # -- the variance at NEW times in linear time (ops.explained_variance; no counterpart in the reference) ------
    def predict_at(self, y, t, *, return_var=False, include_mean=True, check_sorted=True):
        """The conditional mean (B, M) of the process at the sorted times `t` ((M,) shared or (B, M)), and with
        `return_var` its variance (B, M) = k(0) - k*^T (K + D)^-1 k*, from two sweeps over the merge of the data and the
        query grid: O((N + M) J^2) work and O((N + M) J) memory per series, where `predict(y, t, return_var=True)` builds
        the N x M cross-covariance and solves against M right-hand sides.  The mean is `predict`'s own (already linear).

        The variance uses the semiseparable form of the kernel on both sides of every query, which a TermConvolution
        does not have inside its exposure window: such a kernel is refused here -- use `predict`.  Widths J <= 32."""
        from .terms import TermConvolution

        self._need()
        self._check_vector(y)
        if isinstance(self.kernel, TermConvolution):
            raise ValueError("predict_at does not take a TermConvolution kernel (not semiseparable inside the exposure "
                             "window): use predict(y, t, return_var=True)")
        cond = ConditionalDistribution(self, y, t=t, include_mean=include_mean)
        ts = cond._xs
        if check_sorted and bool((ts[..., 1:] < ts[..., :-1]).any()):
            raise ValueError("The prediction coordinates must be sorted")
        if not return_var:
            return self._nan_failed(cond.mean)[0]
        B = self._diag.shape[0]
        zero = torch.zeros((B, ts.shape[-1]), dtype=torch.float64, device=self._diag.device)
        _, _, Us, Vs = self.kernel.get_celerite_matrices(ts, zero)
        r = ops.explained_variance(self._t, ts, self._c, self._U, self._W, self._d, Us, Vs)
        return self._nan_failed(cond.mean, cond._k0() - r)

    # -- streaming updates (stream.Filter; no counterpart in the reference) ------------------------------------------------
    def filter(self, y):
        """A stream.Filter that has absorbed the computed series and the data `y` (B, N): one solve_lower and one absorb
        of the d, W already factored -- nothing is refactored.  Rows are then appended in O(M J^2) each
        (Filter.append).  A series whose factorisation failed gets a NaN state."""
        from .stream import Filter

        if self.kernel._has_tensors():
            raise ValueError("gp.filter does not take a kernel with tensor hyper-parameters (use stream.Filter.empty)")
        self._need()
        self._check_vector(y)
        z = ops.solve_lower(self._t, self._c, self._U, self._W, (y - self.mean)[..., None].contiguous())[..., 0].contiguous()
        state = ops.filter_init(self._diag.shape[0], self._U.shape[-1], self._diag.device)
        ops.filter_absorb(state, self._t, self._c, self._W, self._d, z, out=state)
        state.masked_fill_((self._flag != 0)[:, None], math.nan)
        return Filter(self.kernel, state, mean=self.mean)

    def filter_kernel(self, y, *, jitter=None):
        """A DIFFERENTIABLE stream.Filter that has absorbed the computed series and the data `y` (B, N), for a kernel with
        tensor hyper-parameters: autograd.filter_absorb_kernel on this GP's t, diag and mean -- to `filter(y)` what
        `log_likelihood_kernel` is to `log_likelihood` (the coefficient-level chain, not the matrices `compute` factored).
        Its state carries the graph: `log_likelihood`, every later `append` and `forecast_log_density` send their gradient
        back through the absorbed rows into the hyper-parameters, `jitter`, a tensor `mean` and `y`.  A failed factorisation
        raises autograd.LinAlgError.  J <= 32."""
        from . import autograd
        from .stream import Filter

        self._need()
        self._check_vector(y)
        state = autograd.filter_absorb_kernel(self.kernel, self._t, y, diag=self._diag, jitter=jitter, mean=self.mean)
        return Filter(self.kernel, state, mean=self.mean, jitter=jitter)

    def predict_kernel(self, y, t, *, jitter=None):
        """The conditional mean (B, M) at the sorted times `t` ((M,) shared or (B, M)), mean included, as a differentiable
        function of the kernel's tensor hyper-parameters, of `jitter`, of a tensor `mean`, of `y` and of the times:
        autograd.predict_mean_kernel on this GP's t, diag and mean -- to `predict(y, t)` what `log_likelihood_kernel` is to
        `log_likelihood` (the coefficient-level chain, not the matrices `compute` factored).  J <= 32."""
        from . import autograd

        self._need()
        self._check_vector(y)
        return autograd.predict_mean_kernel(self.kernel, self._t, y, t, diag=self._diag, jitter=jitter, mean=self.mean)

    def predict_variance_kernel(self, y, t, *, jitter=None):
        """The conditional variance (B, M) at the sorted times `t` ((M,) shared or (B, M)) as a differentiable function of
        the kernel's tensor hyper-parameters, of `jitter` and of the times: autograd.predict_variance_kernel on this GP's
        t and diag -- to `predict_at(y, t, return_var=True)[1]` what `predict_kernel` is to its mean.  J <= 32."""
        from . import autograd

        self._need()
        self._check_vector(y)
        return autograd.predict_variance_kernel(self.kernel, self._t, y, t, diag=self._diag, jitter=jitter, mean=self.mean)

    def predictive_log_density_kernel(self, y, t, ys, *, jitter=None, yerr_new=None):
        """The held-out log predictive density (B,) of the values `ys` (B, M) at the sorted times `t` given `y`, as a
        differentiable function of the kernel's tensor hyper-parameters, of `jitter`, of a tensor `mean`, of `y`, `ys` and
        the times: autograd.predictive_log_density_kernel on this GP's t, diag and mean.  `yerr_new` (B, M): the noise of
        the held-out values (jitter is added to it in quadrature).  J <= 32."""
        from . import autograd

        self._need()
        self._check_vector(y)
        return autograd.predictive_log_density_kernel(self.kernel, self._t, y, t, ys, diag=self._diag, jitter=jitter,
                                                      mean=self.mean, yerr_new=yerr_new)

    # -- linear mean models in linear time (ops.whitened_gram; no counterpart in the reference) --------------------
    def _linear(self, y, A, prior_mean, prior_precision):
        """(LinearFit, r, A) on the stored factors: r = y - mean - A mu0, S from one forward sweep, the rest on (B, Q, Q)."""
        from . import autograd

        self._need()
        self._check_vector(y)
        B, N = self._diag.shape
        autograd._check_design(A, B, N, prior_mean, prior_precision)
        r = autograd._prior_residual(y - self.mean, A, prior_mean)
        S = ops.whitened_gram(self._t, self._c, self._U, self._W, self._d, A.contiguous(), r.contiguous())
        fit, _ = autograd._linear_fit(S, self._log_det, N, prior_mean, prior_precision, ok=self._flag == 0)
        return fit, r

    def fit_linear(self, y, A, *, prior_mean=None, prior_precision=None):
        """Generalized least squares of `y` on the design matrix `A` ((N, P) shared | (B, N, P)) under the factored
        covariance: the model y = mean + A beta + GP.  Returns LinearModelFit(beta (B, P), cov (B, P, P), log_likelihood (B,),
        marginal_log_likelihood (B,), residual (B, N)) -- autograd.gls's LinearFit (its docstring has the formulas and the
        Gaussian prior `prior_mean` (P,) | (B, P), `prior_precision` (P, P) | (B, P, P); flat without) plus
        residual = y - mean - A beta.  One forward sweep over the stored factors that never writes L^-1 [A | y]
        (ops.whitened_gram), then a P x P Cholesky per series.  The stochastic part of the data is then

            gp.predict(fit.residual + gp.mean, t)

        Not differentiable (`marginal_log_likelihood_kernel` is) and never raising under compute(..., quiet=True): a series
        whose factorisation failed or whose A is rank-deficient holds NaN beta / cov / residual and -inf likelihoods.
        J <= 32, P <= 31."""
        fit, r = self._linear(y, A, prior_mean, prior_precision)
        delta = fit.beta if prior_mean is None else fit.beta - prior_mean
        return LinearModelFit(*fit, r - torch.matmul(A, delta[..., None])[..., 0])

    def marginal_log_likelihood(self, y, A, *, prior_mean=None, prior_precision=None, profiled=False):
        """(B,): the log-likelihood of `y` under mean + A beta + GP with beta marginalised out under the Gaussian prior
        (prior_mean, prior_precision), or a flat one -- `fit_linear`'s marginal_log_likelihood (`profiled=True`: its
        log_likelihood, at the fitted beta).  -inf for a failed or rank-deficient series."""
        fit, _ = self._linear(y, A, prior_mean, prior_precision)
        return fit.log_likelihood if profiled else fit.marginal_log_likelihood

    def marginal_log_likelihood_kernel(self, y, A, *, jitter=None, prior_mean=None, prior_precision=None, profiled=False):
        """`marginal_log_likelihood` as a differentiable function of the kernel's tensor hyper-parameters, of `jitter`, of a
        tensor `mean`, of `y` and of `A`: autograd.marginal_log_likelihood_kernel on this GP's t, diag and mean (the
        coefficient-level chain, not the matrices `compute` factored; it raises LinAlgError where this class gives -inf)."""
        from . import autograd

        self._need()
        self._check_vector(y)
        return autograd.marginal_log_likelihood_kernel(self.kernel, self._t, y, A, diag=self._diag, jitter=jitter, mean=self.mean,
                                                       prior_mean=prior_mean, prior_precision=prior_precision, profiled=profiled)

    def _whitened_columns(self, y, A):
        """Z0 (B, N, P0 + 1) = L^-1 [A0 | y - mean] for the nuisance columns `A` of periodogram and transit_search: "mean" (a
        column of ones), None (none) or a design matrix (N, P0) | (B, N, P0) with P0 <= 7."""
        B, N = self._diag.shape
        r = (y - self.mean)[..., None]
        if A is None:
            Y0 = r
        else:
            if isinstance(A, str):
                if A != "mean":
                    raise ValueError("A must be \"mean\", None or a design matrix")
                A = torch.ones((N, 1), dtype=torch.float64, device=self._diag.device)
            if A.dim() not in (2, 3) or tuple(A.shape[-2:-1]) != (N,) or (A.dim() == 3 and A.shape[0] != B) \
                    or not 1 <= A.shape[-1] <= 7:
                raise ValueError("Invalid shape: A %s (must be (N, P0) or (B, N, P0) with (B, N) = %s, 1 <= P0 <= 7)"
                                 % (tuple(A.shape), (B, N)))
            Y0 = torch.cat([A.expand(B, N, A.shape[-1]), r], dim=-1)
        return ops.solve_lower(self._t, self._c, self._U, self._W, Y0.contiguous())

    def _nan_failed_fit(self, fit):
        """`fit`, a named tuple of (B, ...) tensors, with NaN in the series whose factorisation failed."""
        B = self._diag.shape[0]
        return type(fit)(*[self._nan_failed(x.reshape(B, -1))[0].reshape(x.shape) for x in fit])

    # -- the periodogram under the factored covariance (ops.whitened_sinusoids; no counterpart in the reference) -------
    def periodogram(self, y, freq, *, A="mean", normalization="standard", t_ref=0.0, return_fit=False, nterms=1):
        """The generalized Lomb-Scargle periodogram of `y` (B, N) under the factored covariance, (B, F): for each ANGULAR trial
        frequency of `freq` ((F,) shared | (B, F)) the model y = mean + A beta0 + alpha cos w(t - t_ref) + beta sin w(t - t_ref)
        + GP is fitted by generalized least squares and compared with the fit without the sinusoid (chi2_null - chi2 = dchi2).
        `A`: the nuisance columns -- "mean" (a column of ones: the floating-mean periodogram), None (none), or a design
        matrix (N, P0) | (B, N, P0) with P0 <= 7.  `normalization`: "standard" (dchi2 / chi2_null, in [0, 1]), "chi2" (dchi2)
        or "log_likelihood" (dchi2 / 2, the log-likelihood ratio at fixed hyper-parameters).  `return_fit=True`:
        periodogram.Periodogram(power (B, F), amplitude (B, F, 2) = (alpha, beta), chi2_null (B,)).
        One solve_lower with P0 + 1 columns, one sweep with a lane per frequency (ops.whitened_sinusoids), then torch on
        (B, F, .) arrays (celerite2_amd/periodogram.py has the formulas).  Not differentiable and never raising under
        compute(..., quiet=True): a frequency at which the sinusoid is not identifiable (w = 0 beside a constant column),
        a series whose factorisation failed or whose A is rank-deficient, and every frequency when N < P0 + 3 hold NaN.
        Times with a large offset keep their phase accuracy with `t_ref` at the offset.  J <= 32.
        `nterms` = H in 2 .. 4: the MULTI-HARMONIC periodogram -- the model carries alpha_h cos x_h + beta_h sin x_h for
        h = 1 .. H, harmonic h at the frequency h w, fitted jointly (ops.whitened_harmonics, one sweep with H lanes per
        frequency; celerite2_amd/harmonics.py has the formulas) -- and `return_fit=True` gives harmonics.Harmonics(power
        (B, F), amplitude (B, F, 2 H) = (alpha_1, beta_1, ..., alpha_H, beta_H), chi2_null (B,)); a frequency at which a
        harmonic aliases onto the constant or onto another harmonic, and every frequency when N < P0 + 2 H + 1, hold NaN;
        harmonics.waveform evaluates the fitted periodic part.  nterms = 1 is the one-term path, untouched."""
        from . import harmonics as hm, periodogram as pg, significance as sg

        if isinstance(nterms, bool) or not isinstance(nterms, int) or not 1 <= nterms <= ops.HARMONICS_MAX:
            raise ValueError("nterms must be an integer from 1 to %d (got %r)" % (ops.HARMONICS_MAX, nterms))

        self._need()
        self._check_vector(y)
        B, N = self._diag.shape
        if normalization not in pg.NORMALIZATIONS:
            raise ValueError("normalization must be one of %s" % (pg.NORMALIZATIONS,))
        freq = sg.check_trials("periodogram", freq, B, "freq", "F")
        Z0 = self._whitened_columns(y, A)
        if nterms > 1:
            T = ops.whitened_harmonics(self._t, self._c, self._U, self._W, self._d, Z0, freq, nterms, t_ref=t_ref)
            fit = self._nan_failed_fit(hm.finish(hm.null_products(Z0, self._d), T, N, nterms, normalization, ok=self._flag == 0))
            return fit if return_fit else fit.power
        T = ops.whitened_sinusoids(self._t, self._c, self._U, self._W, self._d, Z0, freq, t_ref=t_ref)
        fit = self._nan_failed_fit(pg.finish(pg.null_products(Z0, self._d), T, N, normalization, ok=self._flag == 0))
        return fit if return_fit else fit.power

    # -- the transit search under the factored covariance (ops.whitened_transits; no counterpart in the reference) -----
    def transit_search(self, y, trials, *, A="mean", return_fit=False):
        """Box least squares of `y` (B, N) under the factored covariance, (B, K): for each trial (period P, epoch t0,
        duration w, ingress tau) of `trials` ((K, 4) shared | (B, K, 4); transit.trial_grid makes a folded grid) the model
        y = mean + A beta0 + delta b_k(t) + GP is fitted by generalized least squares and compared with the fit without the
        template (chi2_null - chi2 = delta_chi2).  b_k is a box (tau = 0) or a trapezoid of full width w with ramps of length
        tau, +1 in transit, folded at P or a single event at t0 when P = 0 (include/celerite2_amd_transit.h has the rule): a
        dip has a negative depth.  `A`: the nuisance columns, as for `periodogram`.  `return_fit=True`:
        transit.TransitSearch(delta_chi2, depth, depth_err, snr (each (B, K)), chi2_null (B,)).
        One solve_lower with P0 + 1 columns, one sweep with a lane per trial (ops.whitened_transits), then torch on (B, K, .)
        arrays (celerite2_amd/transit.py has the formulas).  Not differentiable and never raising under
        compute(..., quiet=True): a trial with no sample in transit, one whose template lies in the span of A, one outside
        w > 0, 0 <= tau <= w / 2, P >= 0, w <= P (P > 0), a series whose factorisation failed or whose A is rank-deficient, and
        every trial when N < P0 + 2 hold NaN.  A TermConvolution kernel is accepted: only the factored matrix is used.
        J <= 32."""
        from . import _trial_fit, significance as sg, transit as tr

        self._need()
        self._check_vector(y)
        B, N = self._diag.shape
        trials = sg.check_trials("transit", trials, B)
        Z0 = self._whitened_columns(y, A)
        T = ops.whitened_transits(self._t, self._c, self._U, self._W, self._d, Z0, trials)
        fit = self._nan_failed_fit(tr.finish(_trial_fit.null_products(Z0, self._d), T, N, ok=self._flag == 0, trials=trials))
        return fit if return_fit else fit.delta_chi2

    # -- the Keplerian search under the factored covariance (ops.whitened_keplerians; no counterpart in the reference) ---
    def keplerian_search(self, y, trials, *, A="mean", normalization="standard", return_fit=False):
        """The Keplerian periodogram of `y` (B, N) under the factored covariance, (B, K): for each trial (angular frequency
        w = 2 pi / P, eccentricity e, time of periastron tp) of `trials` ((K, 3) shared | (B, K, 3); kepler.trial_grid makes
        a regular grid) the model y = mean + A beta0 + K [cos(nu(t) + omega) + e cos omega] + GP, nu the true anomaly of
        the orbit, is fitted by generalized least squares in (alpha, beta) = (K cos omega, -K sin omega) and compared with
        the fit without the orbit (chi2_null - chi2 = dchi2).  `A`: the nuisance columns, as for `periodogram`; the
        orbit's constant K e cos omega needs a constant column among them ("mean" has it).  `normalization`: as for
        `periodogram`.  `return_fit=True`: kepler.KeplerianSearch(power (B, K), amplitude (B, K, 2) = (alpha, beta),
        semi_amplitude (B, K), omega (B, K), chi2_null (B,)).
        One solve_lower with P0 + 1 columns, one sweep with a lane per trial that solves Kepler's equation in registers
        (ops.whitened_keplerians; include/celerite2_amd_kepler.h has the rule), then torch on (B, K, .) arrays
        (celerite2_amd/kepler.py).  Not differentiable and never raising under compute(..., quiet=True): a trial outside
        w > 0, 0 <= e <= 0.99, tp finite, one at which the two columns are not identifiable beside A, a series whose
        factorisation failed or whose A is rank-deficient, and every trial when N < P0 + 3 hold NaN.  Times with a large
        offset keep their accuracy with tp at the offset.  J <= 32."""
        from . import _trial_fit, kepler as kp, periodogram as pg, significance as sg

        self._need()
        self._check_vector(y)
        B, N = self._diag.shape
        if normalization not in pg.NORMALIZATIONS:
            raise ValueError("normalization must be one of %s" % (pg.NORMALIZATIONS,))
        trials = sg.check_trials("keplerian", trials, B)
        Z0 = self._whitened_columns(y, A)
        T = ops.whitened_keplerians(self._t, self._c, self._U, self._W, self._d, Z0, trials)
        fit = self._nan_failed_fit(kp.finish(_trial_fit.null_products(Z0, self._d), T, N, normalization, ok=self._flag == 0,
                                             trials=trials))
        return fit if return_fit else fit.power

    def keplerian_periodogram(self, y, freq, ecc, n_phase, *, A="mean", normalization="standard", t0=0.0, max_trials=None):
        """`keplerian_search` on the regular grid kepler.trial_grid(freq, ecc, n_phase, t0=t0) -- ANGULAR frequencies `freq`
        (F,), eccentricities `ecc` (E), n_phase times of periastron over a period -- profiled over eccentricity and
        periastron: (power (B, F), best_trial (B, F, 3), amplitude (B, F, 2)), the maximum over the E n_phase trials of each
        frequency (NaN trials ignored; NaN where all are), the maximising (w, e, tp) and its (alpha, beta).
        `max_trials`: run the search in blocks of whole frequencies of at most that many trials, so that the (B, K, 3 + 2 Q0)
        products stay bounded (ValueError when one frequency's E n_phase trials exceed it); the result does not depend on
        it, to the bit."""
        from . import kepler as kp

        self._need()
        grid = kp.trial_grid(freq, ecc, n_phase, t0=t0).to(self._diag.device)
        F = int(torch.as_tensor(freq).numel())
        if F < 1 or grid.shape[0] < F:
            raise ValueError("Invalid shape: freq, ecc (at least one frequency and one eccentricity)")
        per = grid.shape[0] // F
        if max_trials is None:
            step = F
        else:
            step = int(max_trials) // per
            if step < 1:
                raise ValueError("max_trials = %d is below the %d trials of one frequency (E n_phase)" % (int(max_trials), per))
        power, index, amplitude = [], [], []
        for f0 in range(0, F, step):
            f1 = min(F, f0 + step)
            fit = self.keplerian_search(y, grid[f0 * per:f1 * per], A=A, normalization=normalization, return_fit=True)
            p, idx = kp.profile(fit, f1 - f0)
            power.append(p)
            amplitude.append(torch.gather(fit.amplitude, 1, idx[..., None].expand(-1, -1, 2)))
            index.append(idx + f0 * per)
        index = torch.cat(index, dim=1)
        return torch.cat(power, dim=1), grid[index], torch.cat(amplitude, dim=1)

    # -- false-alarm probabilities of the three searches (ops.trial_projections; no counterpart in the reference) -------
    def search_significance(self, kind, y, trials, *, draws=1000, A="mean", normalization="standard", t_ref=0.0,
                            dips_only=False, generator=None, normals=None, max_trials=None, max_draws=None, nterms=1):
        """The search `kind` ("periodogram", "transit" or "keplerian") on `y` (B, N) with the Monte-Carlo false-alarm
        probability of every trial: significance.Significance(statistic (B, K), fap (B, K), null_maxima (B, draws)).
        `trials`: what the search takes -- ANGULAR frequencies (F,) | (B, F) for the periodogram, (K, 4) | (B, K, 4) for the
        transit, (K, 3) | (B, K, 3) for the keplerian.  `statistic` is that search's result: the power of `periodogram` /
        `keplerian_search` in `normalization`; for the transit delta_chi2 / chi2_null ("standard"), delta_chi2 ("chi2") or
        half of it ("log_likelihood"), and with `dips_only` 0 where the fitted depth is positive.  `null_maxima[b, r]` is
        the largest statistic over the trials (NaN ones ignored) of the same search on the r-th draw
        y_r = mean + L D^1/2 n_r from the factored covariance, and
        fap = (1 + #{r : null_maxima[b, r] >= statistic}) / (draws + 1): the probability that noise alone puts the
        HIGHEST peak of the grid at or above this trial's statistic (a maximum within 1e-10 of the statistic, relative,
        counts as at it).

        THE PROBABILITY IS CONDITIONAL ON THE HYPER-PARAMETERS: the draws come from the covariance `compute` factored and
        the kernel is not refitted per draw, as it would be on real data; where the hyper-parameters were fitted to `y`
        itself, a signal absorbed by the kernel is not counted.

        One sweep on `y` (the search's own) gives the statistic and every product that does not depend on the data; a
        draw adds one column to one solve_upper and to ops.trial_projections, which forms each trial's column(s) once for
        all draws (celerite2_amd/significance.py has the identities) -- no sweep per draw.  `normals` (B, N, draws): the
        standard normals n_r, for reproducibility; otherwise torch.randn(..., generator=generator).  `max_trials`,
        `max_draws`: take the trials / draws in blocks of at most that many, which bounds the (B, K, C, draws) and
        (B, K, draws) arrays; the result does not depend on `max_trials`, to the bit, and on `max_draws` to rounding (the
        solve may take another kernel at another column count).  `A`, `t_ref`: as for the searches.  Not differentiable
        and never raising under compute(..., quiet=True): a series whose factorisation failed holds NaN.  J <= 32.
        `nterms` = H in 2 .. 4 (the periodogram only): the MULTI-HARMONIC periodogram's significance -- `statistic` is
        `periodogram(..., nterms=H)`'s power, and the statistic of every (frequency, draw) is finished in the registers of
        the pass that projects the draws on the 2 H columns (ops.harmonic_null_chi2; harmonics.null_statistics is its
        torch form), so a draw costs (B, F) values, not (B, F, 2 H).  nterms = 1 is the route above, untouched."""
        if isinstance(nterms, bool) or not isinstance(nterms, int) or not 1 <= nterms <= ops.HARMONICS_MAX:
            raise ValueError("nterms must be an integer from 1 to %d (got %r)" % (ops.HARMONICS_MAX, nterms))
        if nterms > 1 and kind != "periodogram":
            raise ValueError("nterms = %d needs kind = \"periodogram\" (got %r): the other searches have one term" % (nterms, kind))
        return _significance(self, kind, y, trials, None, draws, A, normalization, t_ref, dips_only, generator, normals, max_trials,
                                  max_draws, nterms)

    # -- the tabulated-shape search under the factored covariance (ops.whitened_shapes; no counterpart in the reference) --
    def _shape_args(self, trials, shapes):
        """(trials, shapes, NS) contiguous, after the shape checks of shape_search and shape_search_significance."""
        from . import significance as sg

        B = self._diag.shape[0]
        trials = sg.check_trials("shape", trials, B)
        if not torch.is_tensor(shapes) or shapes.dim() not in (2, 3) or (shapes.dim() == 3 and shapes.shape[0] != B):
            raise ValueError("Invalid shape: shapes (must be (NS, S) or (B, NS, S) with B = %d)" % B)
        return trials, shapes.contiguous(), shapes.shape[-2]

    def shape_search(self, y, trials, shapes, *, A="mean", return_fit=False):
        """Least squares of `y` (B, N) with an event of a TABULATED SHAPE under the factored covariance, (B, K): for each
        trial (period P, epoch t0, width w, shape index s) of `trials` ((K, 4) shared | (B, K, 4); shapes.trial_grid makes a
        folded grid) the model y = mean + A beta0 + delta b_k(t) + GP is fitted by generalized least squares and compared
        with the fit without the event (chi2_null - chi2 = delta_chi2).  b_k is the s-th row of the bank `shapes` ((NS, S)
        shared | (B, NS, S), NS * S <= 1024; shapes.limb_darkened, flare, trapezoid, box and stack build one), S values on a
        uniform grid from the leading to the trailing edge of an event of full width w centred on t0, linearly interpolated,
        zero outside, folded at P or a single event when P = 0 (include/celerite2_amd_shapes.h has the rule).  `A`: the
        nuisance columns, as for `periodogram`.  `return_fit=True`: shapes.ShapeSearch(delta_chi2, amplitude,
        amplitude_err, snr (each (B, K)), chi2_null (B,)); a dip under a shape with peak +1 has a negative amplitude.
        One solve_lower with P0 + 1 columns, one sweep with a lane per trial (ops.whitened_shapes), then torch on (B, K, .)
        arrays (celerite2_amd/shapes.py).  Not differentiable and never raising under compute(..., quiet=True): a trial with
        no sample in the event, one whose column lies in the span of A, one outside w > 0, P >= 0, w <= P (P > 0), (P, t0, w)
        finite, s an integer in [0, NS), a series whose factorisation failed or whose A is rank-deficient, and every trial
        when N < P0 + 2 hold NaN.  J <= 32."""
        from . import _trial_fit, shapes as sh

        self._need()
        self._check_vector(y)
        N = self._diag.shape[1]
        trials, shapes, NS = self._shape_args(trials, shapes)
        Z0 = self._whitened_columns(y, A)
        T = ops.whitened_shapes(self._t, self._c, self._U, self._W, self._d, Z0, trials, shapes)
        fit = self._nan_failed_fit(sh.finish(_trial_fit.null_products(Z0, self._d), T, N, ok=self._flag == 0, trials=trials,
                                             n_shapes=NS))
        return fit if return_fit else fit.delta_chi2

    def shape_search_significance(self, y, trials, shapes, *, draws=1000, A="mean", normalization="standard", dips_only=False,
                                  generator=None, normals=None, max_trials=None, max_draws=None):
        """`shape_search` on `y` (B, N) with the Monte-Carlo false-alarm probability of every trial:
        significance.Significance(statistic (B, K), fap (B, K), null_maxima (B, draws)) -- `search_significance`'s transit
        branch with the tabulated column: `statistic` is delta_chi2 / chi2_null ("standard"), delta_chi2 ("chi2") or half
        of it ("log_likelihood"), with `dips_only` 0 where the fitted amplitude is positive; `null_maxima[b, r]` the largest
        statistic over the trials (NaN ones ignored) of the same search on the r-th draw y_r = mean + L D^1/2 n_r, and
        fap = (1 + #{r : null_maxima[b, r] >= statistic}) / (draws + 1).  The probability is CONDITIONAL ON THE
        HYPER-PARAMETERS, as there.  One sweep on `y`; a draw adds one column to one solve_upper and to
        ops.shape_projections -- no sweep per draw.  `normals`, `generator`, `max_trials` (same bits), `max_draws` (to
        rounding), `A`: as for `search_significance`.  Not differentiable and never raising under
        compute(..., quiet=True): a series whose factorisation failed holds NaN.  J <= 32."""
        return _significance(self, "shape", y, trials, shapes, draws, A, normalization, 0.0, dips_only, generator, normals, max_trials,
                                  max_draws)

    # -- draws at NEW times in linear time (ops.prior_draw + Matheron's rule; no counterpart in the reference) ----
    def sample_at(self, y, t, *, size=None, include_mean=True, generator=None, normals=None, check_sorted=True):
        """Draws (B, M) -- (B, size, M) when `size` is given -- from the conditional distribution of the process at the
        sorted times `t` ((M,) shared or (B, M)) given `y`, without the M x M covariance that `condition(y, t).sample`
        factors.  By Matheron's rule, with (f_t, f_s) a joint draw of the noise-free prior process on the data and the query
        times (ops.prior_draw, one sweep over the merge of the two grids) and eps ~ N(0, D),

            f_s + K(s, t) (K + D)^-1 (y - mean - f_t - eps)    (+ mean)

        is such a draw: apply_inverse with `size` right-hand sides and the two general products of the conditional mean.
        O((N + M) (J^2 + J size)) work per series, no array larger than (N + M) x size.

        `normals`: a triple (nt (B, N, K), ns (B, M, K), ne (B, N, K)) of standard normals, K = size (1 for None), for
        reproducibility; otherwise the three are drawn, in that order, with torch.randn(..., generator=generator).  A
        query that coincides with a data time or an earlier query takes that point's process value (its normals are not
        used).  A TermConvolution kernel is refused, for predict_at's reason -- use `condition(y, t).sample`.  J <= 32."""
        from .terms import TermConvolution

        self._need()
        self._check_vector(y)
        if isinstance(self.kernel, TermConvolution):
            raise ValueError("sample_at does not take a TermConvolution kernel (not semiseparable inside the exposure "
                             "window): use condition(y, t).sample(...)")
        cond = ConditionalDistribution(self, y, t=t, include_mean=include_mean)
        ts = cond._xs
        if check_sorted and bool((ts[..., 1:] < ts[..., :-1]).any()):
            raise ValueError("The prediction coordinates must be sorted")
        (B, N), M, dev = self._diag.shape, ts.shape[-1], self._diag.device
        K = 1 if size is None else int(size)
        if normals is None:
            nt, ns, ne = (torch.randn((B, L, K), dtype=torch.float64, device=dev, generator=generator) for L in (N, M, N))
            ft, fs = nt, ns      # (ours: drawn in place)
        else:
            nt, ns, ne = normals
            for name, x, L in (("nt", nt, N), ("ns", ns, M), ("ne", ne, N)):
                if tuple(x.shape) != (B, L, K):
                    raise ValueError("Invalid shape: normals %s %s, expected %s" % (name, tuple(x.shape), (B, L, K)))
            ft = fs = None       # (the caller's: left as they are)
        cond._mats2 = self.kernel.get_celerite_matrices(ts, torch.zeros((B, M), dtype=torch.float64, device=dev))
        _, _, Us, Vs = cond._mats2
        ft, fs = ops.prior_draw(self._t, ts, self._c, self._U, self._V, Us, Vs, nt.contiguous(), ns.contiguous(), ft=ft, fs=fs)
        resid = (y - self.mean)[..., None] - ft - torch.sqrt(self._diag)[..., None] * ne
        out = cond._do_dot(self.apply_inverse(resid), fs).transpose(1, 2)   # (B, K, M)
        if include_mean:
            out = out + self.mean
        out = self._nan_failed(out.reshape(B, K * M))[0].reshape(B, K, M)
        return out[:, 0] if size is None else out

    # -- conditional distribution, core.py:430-478 ------------------------------------------------------
    def condition(self, y, t=None, *, include_mean=True, kernel=None):
        self._need()
        self._check_vector(y)
        return ConditionalDistribution(self, y, t=t, include_mean=include_mean, kernel=kernel)

    def predict(self, y, t=None, *, return_cov=False, return_var=False, include_mean=True, kernel=None):
        """core.py:430-472: the conditional mean (B, M), and with `return_var` its variance (B, M), with `return_cov`
        its covariance (B, M, M) -- `apply_inverse` on the N x M cross-covariance, i.e. solves with M right-hand sides
        (SURVEY.md 8f-4)."""
        cond = self.condition(y, t=t, include_mean=include_mean, kernel=kernel)
        if return_var:
            return cond.mean, cond.variance
        if return_cov:
            return cond.mean, cond.covariance
        return cond.mean


class ConditionalDistribution:
    """Batched mirror of core.py:9-150 (BaseConditionalDistribution) + numpy.py:14-32: the distribution of the process at
    coordinates `t` (B, M) | (M,) -- default: the observed grid -- given observations `y` (B, N).  Properties are evaluated
    on demand and cached like the reference's (`KxsT`, `Kinv_KxsT`)."""

    def __init__(self, gp, y, t=None, *, include_mean=True, kernel=None):
        self.gp, self.y, self.t, self.include_mean, self.kernel = gp, y, t, include_mean, kernel
        self._KxsT = self._Kinv_KxsT = self._Linv_KxsT = self._mean = None
        self._mats2 = self._mats1 = None
        if t is None:
            self._xs = gp._t
        else:
            if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != gp._diag.shape[0]):
                raise ValueError("'t' must be (M,) or (B, M)")   # core.py:39-40
            self._xs = t.contiguous()

    def _kernel(self):
        return self.gp.kernel if self.kernel is None else self.kernel

    def _batched(self, x):
        B = self.gp._diag.shape[0]
        return x if x.dim() == 2 else x[None].expand(B, x.shape[0])

    @property
    def KxsT(self):      # core.py:46-54: k(t_n - xs_m), (B, N, M)
        if self._KxsT is None:
            self._KxsT = self._kernel().get_value_grid(self.gp._t, self._xs, B=self.gp._diag.shape[0])
        return self._KxsT

    @property
    def Linv_KxsT(self):  # L^-1 KxsT (K = L D L^T): the lower solve with M right-hand sides, shared by variance and Kinv_KxsT
        if self._Linv_KxsT is None:
            gp = self.gp
            self._Linv_KxsT = ops.solve_lower(gp._t, gp._c, gp._U, gp._W, self.KxsT.contiguous())
        return self._Linv_KxsT

    @property
    def Kinv_KxsT(self):  # core.py:56-60: apply_inverse on the N x M matrix -- solves with M right-hand sides
        if self._Kinv_KxsT is None:
            gp = self.gp
            z = self.Linv_KxsT / gp._d[..., None]
            self._Kinv_KxsT = ops.solve_upper(gp._t, gp._c, gp._U, gp._W, z, Z=z)
        return self._Kinv_KxsT

    def _do_dot(self, inp, target):
        """core.py:68-113 + numpy.py:15-22: target += K(xs, t) inp through general_matmul_lower/upper.  (Under a
        TermConvolution these semiseparable products are exact for lags >= delta, the reference's behaviour.)"""
        gp = self.gp
        if self.kernel is None:
            U1, V1 = gp._U, gp._V
        else:
            if self._mats1 is None:
                self._mats1 = self.kernel.get_celerite_matrices(gp._t, torch.zeros_like(gp._diag))
            U1, V1 = self._mats1[2], self._mats1[3]
        if self._mats2 is None:
            B = gp._diag.shape[0]
            zero = torch.zeros((B, self._xs.shape[-1]), dtype=torch.float64, device=gp._diag.device)
            self._mats2 = self._kernel().get_celerite_matrices(self._xs, zero)
        c, _, U2, V2 = self._mats2
        vec = inp.dim() == 2
        if vec:
            inp, target = inp[..., None], target[..., None]
        inp, target = inp.contiguous(), target.contiguous()
        target = ops.general_matmul_lower(self._xs, gp._t, c, U2, V1, inp, Z=target)
        target = ops.general_matmul_upper(self._xs, gp._t, c, V2, U1, inp, Z=target)
        return target[..., 0] if vec else target

    @property
    def mean(self):      # core.py:115-132 (computed once per distribution: predict(return_var / return_cov) and sample() reuse it)
        if self._mean is None:
            gp = self.gp
            alpha = gp.apply_inverse(self.y - gp.mean)
            if self.t is None and self.kernel is None:
                mu = self.y - gp._diag * alpha
                self._mean = mu if self.include_mean else mu - gp.mean
            else:
                B = gp._diag.shape[0]
                mu = torch.zeros((B, self._xs.shape[-1]), dtype=torch.float64, device=gp._diag.device)
                mu = self._do_dot(alpha, mu)
                self._mean = mu + gp.mean if self.include_mean else mu
        return self._mean

    @property
    def variance(self):  # core.py:134-140 + numpy.py:24-25: k(0) - diag(KxsT' K^-1 KxsT), (B, M)
        # diag(Kxs K^-1 KxsT)_m = sum_n (L^-1 KxsT)_nm^2 / d_n: the lower solve and ONE pass over its result
        # (ops.colsumsq_over_d) -- the reference's apply_inverse + diagdot (numpy.py:24-25) is both solves and a pass over
        # two N x M arrays for the same number
        return self._k0() - ops.colsumsq_over_d(self.Linv_KxsT, self.gp._d)

    def _k0(self):
        """k(0) = sum ar + sum ac (terms.py:58-79 at tau = 0), plus delta_diag under a TermConvolution (its piecewise k(0),
        terms.py:421-482): a python float, or (B, 1) on the device for per-series coefficients."""
        kernel, B, dev = self._kernel(), self.gp._diag.shape[0], self.gp._diag.device
        shift = kernel._k0_shift(B, dev)
        if kernel._has_tensors():
            co = kernel._device_coefs(B)[0]
            return (co[0].sum(dim=-1) + co[2].sum(dim=-1))[:, None] + shift
        co = kernel.get_coefficients()
        if all(v.ndim == 1 for v in co):
            return float(co[0].sum() + co[2].sum()) + shift
        co, _ = kernel._dev_coefs(dev, B)
        return (co[0].sum(dim=-1) + co[2].sum(dim=-1))[:, None] + shift

    @property
    def covariance(self):  # core.py:142-150: k(xs - xs') - K(xs, t) K^-1 K(t, xs), (B, M, M)
        neg_cov = -self._kernel().get_value_grid(self._xs, self._xs, B=self.gp._diag.shape[0])
        neg_cov = self._do_dot(self.Kinv_KxsT, neg_cov)
        return -neg_cov

    def sample(self, *, size=None, regularize=None, generator=None):
        """numpy.py:27-32: draws from N(mean, covariance), O(M^3) per series (a dense Cholesky of the M x M covariance
        by torch -- outside the hot path, as in the reference)."""
        mu, cov = self.mean, self.covariance
        if regularize is not None:
            cov = cov + regularize * torch.eye(cov.shape[-1], dtype=cov.dtype, device=cov.device)
        L = torch.linalg.cholesky(0.5 * (cov + cov.transpose(1, 2)))
        k = 1 if size is None else size
        n = torch.randn((cov.shape[0], cov.shape[-1], k), dtype=torch.float64, device=cov.device, generator=generator)
        out = (L @ n).transpose(1, 2) + mu[:, None, :]
        return out[:, 0] if size is None else out
