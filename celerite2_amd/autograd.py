# -*- coding: utf-8 -*-
"""torch.autograd adapter over the fused kernels (framework adapter on the device path).

`log_likelihood(t, c, a, U, V, y)` is differentiable w.r.t. every argument: the forward call runs
c2_loglik_grad once (value and the six cotangents come out of the same checkpoint/replay pass, exactly what the
reference's PyMC/JAX ops do in two steps -- pymc/ops.py:104-141), backward just scales the saved gradients by
the incoming cotangent.  Shared `t` (N,) / `c` (J,) receive the batch-summed gradient.

`loo_log_predictive[_kernel]` is the leave-one-out log predictive density (Rasmussen & Williams 5.4.2) as a training
objective, through `inverse_diag` and its reverse sweep (csrc/c2_invdiag_rev.hip).

`predict_mean[_kernel]` is the conditional mean at new times as a differentiable function of everything it depends on,
through `general_matmul_lower` / `general_matmul_upper` and their reverse sweep (csrc/c2_general_rev.hip).

`whitened_gram`, `gls` and `marginal_log_likelihood_kernel` are linear mean models under the GP noise model: the Q x Q
Gram matrix [A | y]^T (K + D)^-1 [A | y] in one forward sweep (csrc/c2_gram.hip), generalized least squares on it, and the
likelihood with the linear coefficients profiled or marginalised out.

`filter_append[_kernel]` is a streaming append (csrc/c2_filter.hip) with its reverse (csrc/c2_filter_rev.hip): the cotangent of
a filter state is carried from one call to the previous one, so the predictive log density of each night's rows trains the
hyper-parameters without revisiting the old rows.  `filter_forecast[_kernel]` and `filter_absorb[_kernel]` are the other two
streaming entry points with theirs (csrc/c2_filter_stream_rev.hip): the log density of what arrives h nights after a forecast
is a training objective, and a filter warm-started from a factored archive sends its gradient back into the archive's rows.

`factor`, `solve_lower`, `solve_upper`, `matmul_lower`, `matmul_upper` are the reference's five differentiable ops
(python/celerite2/pymc/ops.py:61-141, jax/ops.py:33-172: forward = `backprop.<op>_fwd` with its workspace, gradient =
`backprop.<op>_rev`), batched, on the device kernels -- for models that compose the ops themselves."""
import collections
import math

import torch

from . import ops

__all__ = ["log_likelihood", "log_likelihood_terms", "term_coefficients", "log_likelihood_kernel", "factor", "solve_lower", "solve_upper", "matmul_lower", "matmul_upper", "inverse_diag", "loo_log_predictive", "loo_log_predictive_kernel", "general_matmul_lower", "general_matmul_upper", "get_celerite_matrices", "predict_mean", "predict_mean_kernel", "explained_variance", "predict_variance", "predictive_log_density", "predict_variance_kernel", "predictive_log_density_kernel", "whitened_gram", "gls", "marginal_log_likelihood_kernel", "filter_append", "filter_append_kernel", "filter_forecast", "filter_absorb", "filter_forecast_kernel", "filter_absorb_kernel", "LinearFit", "LinAlgError"]


class LinAlgError(RuntimeError):
    """failed to factorize or solve matrix (driver.hpp:13-19); `.flag` holds the per-series first bad row."""


class _LogLik(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, c, a, U, V, y):
        args = [x.detach().contiguous() for x in (t, c, a, U, V, y)]
        needs_grad = any(x.requires_grad for x in (t, c, a, U, V, y))
        if not needs_grad:
            ll, flag = ops.loglik(*args)
            ctx.grads = None
            return ll
        ll, grads, flag = ops.loglik_grad(*args)
        ctx.shared_t = t.dim() == 1
        ctx.shared_c = c.dim() == 1
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable()
        return ll

    @staticmethod
    def backward(ctx, g):
        # A series whose factorisation failed has ll = -inf and NaN gradients (c2_loglik_grad, celerite2_amd.h).
        # A series that receives a ZERO cotangent contributes exactly zero -- so masking failed series out of the
        # objective keeps the batch-summed gradients of a shared t / c finite; left in, they turn NaN, never garbage.
        bt, bc, ba, bU, bV, by = ctx.saved_tensors
        g1, g2 = g[:, None], g[:, None, None]
        z1, z2 = g1 == 0, g2 == 0
        sc = lambda x, gg, zz: torch.where(zz, torch.zeros((), dtype=x.dtype, device=x.device), x * gg)
        gt = sc(bt, g1, z1).sum(0) if ctx.shared_t else sc(bt, g1, z1)
        gc = sc(bc, g1, z1).sum(0) if ctx.shared_c else sc(bc, g1, z1)
        return gt, gc, sc(ba, g1, z1), sc(bU, g2, z2), sc(bV, g2, z2), sc(by, g1, z1)


def log_likelihood(t, c, a, U, V, y):
    """Batched GP log-likelihood (B,), differentiable through torch.autograd."""
    return _LogLik.apply(t, c, a, U, V, y)


class _LogLikTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ar, cr, ac, bc, cc, dc, x, diag, y):
        args = [v.detach().contiguous() for v in (ar, cr, ac, bc, cc, dc, x, diag, y)]
        if not any(v.requires_grad for v in (ar, cr, ac, bc, cc, dc, x, diag, y)):
            ll, flag = ops.loglik_terms(*args)
            return ll
        ll, grads, flag = ops.loglik_terms_grad(*args)
        ctx.shared = [v.dim() == 1 for v in (ar, cr, ac, bc, cc, dc, x)]
        ctx.save_for_backward(*grads)
        return ll

    @staticmethod
    def backward(ctx, g):
        grads = ctx.saved_tensors
        g1 = g[:, None]
        zero = torch.zeros((), dtype=g.dtype, device=g.device)
        out = []
        for k, gr in enumerate(grads):
            v = torch.where(g1 == 0, zero, gr * g1)   # a masked-out (failed) series contributes exactly zero
            out.append(v.sum(0) if (k < 7 and ctx.shared[k]) else v)
        return tuple(out)


def log_likelihood_terms(ar, cr, ac, bc, cc, dc, x, diag, y):
    """Batched GP log-likelihood (B,) as a differentiable function of the celerite coefficients, the times, the
    white-noise diagonal and the data -- the gradient a sampler needs, computed by the device chain of c2_terms.hip.
    Shared coefficients / times (one fewer dimension) receive the batch-summed gradient."""
    return _LogLikTerms.apply(ar, cr, ac, bc, cc, dc, x, diag, y)


class _TermCoefficients(torch.autograd.Function):
    @staticmethod
    def forward(ctx, program, P, B):
        Pd = P.detach().contiguous()
        ctx.program, ctx.shared = program, P.dim() == 1
        ctx.save_for_backward(Pd)
        if isinstance(program, ops.TermExpr):   # seven outputs: the diagonal shift of a convolution is differentiable too
            coefs, flag, shift = ops.term_coefficients(program, Pd, B)
            return coefs + (shift,)
        coefs, flag = ops.term_coefficients(program, Pd, B)
        return coefs

    @staticmethod
    def backward(ctx, *cots):
        (P,) = ctx.saved_tensors
        if isinstance(ctx.program, ops.TermExpr):
            bP = ops.term_coefficients_rev(ctx.program, P, [c.contiguous() for c in cots[:6]], bshift=cots[6].contiguous())
        else:
            bP = ops.term_coefficients_rev(ctx.program, P, [c.contiguous() for c in cots])
        return None, (bP.sum(0) if ctx.shared else bP), None


def term_coefficients(program, P, B=None, *, with_shift=False):
    """(ar, cr, ac, bc, cc, dc) (B, Jr) / (B, Jc) from the parameter matrix P (B, NP) | shared (NP,) of a term program
    (ops.TermProgram, or ops.TermExpr for products / derivatives / the exposure-time convolution), differentiable in P:
    c2_term[_expr]_coefficients forward, c2_term[_expr]_coefficients_rev backward (one launch each; a shared P receives the
    batch sum).  What the reference's jax / pymc term classes give by autodiff.  `with_shift=True`: a seventh tensor, the
    diagonal shift (B,) of a convolution (zeros for any other kernel), differentiable as well."""
    out = _TermCoefficients.apply(program, P, B)
    if not with_shift:
        return tuple(out[:6])
    if len(out) == 7:
        return tuple(out)
    n = out[0].shape[0] if program.Jr else out[2].shape[0]
    return tuple(out) + (torch.zeros(n, dtype=torch.float64, device=P.device),)


class _LogLikKernel(torch.autograd.Function):
    """noise_mean_apply -> term_coefficients -> loglik_terms[_grad] -> term_coefficients_rev / noise_mean_rev as ONE node
    (ops.loglik_kernel_grad; with a TermExpr its chain through the diagonal shift): the gradients come out of the forward
    call (as in _LogLikTerms), backward scales them by the incoming cotangent."""

    @staticmethod
    def forward(ctx, program, is_sigma, P, x, yerr, jitter, mean, y):
        tens = (P, x, yerr, jitter, mean, y)
        Pd, xd, ed, jd, md, yd = [None if v is None else v.detach().contiguous() for v in tens]
        B = y.shape[0]
        if not any(v is not None and v.requires_grad for v in tens):
            if isinstance(program, ops.TermExpr):
                coefs, tflag, shift = ops.term_coefficients(program, Pd, B)
                diag, r = ops.noise_mean_shift_apply(ed, jd, md, shift, yd, yerr_is_sigma=is_sigma)
            else:
                diag, r = ops.noise_mean_apply(ed, jd, md, yd, yerr_is_sigma=is_sigma)
                coefs, tflag = ops.term_coefficients(program, Pd, B)
            ll, flag = ops.loglik_terms(*coefs, xd, diag, r)
            return torch.where(tflag != 0, torch.full_like(ll, -float("inf")), ll)
        ll, (bP, bj, bm, bx, bdiag, by), flag = ops.loglik_kernel_grad(program, Pd, xd, ed, jd, md, yd, yerr_is_sigma=is_sigma)
        ctx.shared_P, ctx.shared_x = P.dim() == 1, x.dim() == 1
        ctx.has = (jitter is not None, mean is not None)
        # byerr = 2 yerr bdiag only when somebody asks for it
        be = bdiag if not is_sigma else (2.0 * ed * bdiag if yerr.requires_grad else None)
        ctx.has_e = be is not None
        ctx.save_for_backward(flag, bP, bj, bm, bx, by, *([be] if be is not None else []))
        return ll

    @staticmethod
    def backward(ctx, g):
        flag, bP, bj, bm, bx, by = ctx.saved_tensors[:6]
        be = ctx.saved_tensors[6] if ctx.has_e else None
        zero = torch.zeros((), dtype=g.dtype, device=g.device)
        dead = (g == 0) | (flag != 0)     # a masked-out or flagged series contributes exactly zero (_LogLikTerms.backward)
        sc1 = lambda v: torch.where(dead, zero, v * g)
        sc2 = lambda v: torch.where(dead[:, None], zero, v * g[:, None])
        gP, gx = sc2(bP), sc2(bx)
        return (None, None, gP.sum(0) if ctx.shared_P else gP, gx.sum(0) if ctx.shared_x else gx,
                sc2(be) if be is not None else None, sc1(bj) if ctx.has[0] else None, sc1(bm) if ctx.has[1] else None, sc2(by))


def _per_series(v, B, like):
    """A float, a 0-d or a (B,) tensor -> (B,) (autograd sums the gradient of a shared value), None stays None."""
    if v is None:
        return None
    if not torch.is_tensor(v):
        return torch.full((B,), float(v), dtype=torch.float64, device=like.device)
    if v.dim() == 0 or tuple(v.shape) == (1,):
        return v.reshape(()).expand(B)
    if tuple(v.shape) != (B,):
        raise ValueError("Invalid shape: jitter / mean (must be a float, 0-d or (B,))")
    return v


def log_likelihood_kernel(kernel, x, y, *, yerr=None, diag=None, jitter=None, mean=None):
    """Batched GP log-likelihood (B,) as a differentiable function of the HYPER-PARAMETERS: every tensor parameter of
    `kernel` (terms.RealTerm / ComplexTerm / SHOTerm / Matern32Term / RotationTerm, their sums, products (TermProduct),
    derivatives (TermDiff) and exposure-time convolution (TermConvolution), with parameters given as float64 device tensors,
    0-d or (B,)), `jitter` (added in quadrature: diag = yerr^2 + jitter^2, or diag + jitter^2) and
    `mean` (floats, 0-d or (B,) tensors), and x (N,) | (B, N), yerr | diag (B, N), y (B, N) when they require grad.
    Everything between the parameters and the gradient runs on the device (csrc/c2_term_params.hip around
    c2_loglik_terms_grad); shared parameters receive the batch-summed gradient.  A series whose factorisation fails, or whose
    Q is on the wrong side of an SHO term's regime, has ll = -inf and contributes zero gradient; the others are untouched."""
    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, N) is required")
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B = y.shape[0]
    if not kernel._has_tensors():
        raise TypeError("log_likelihood_kernel: the kernel has no tensor parameter (give its parameters as device tensors)")
    P = kernel.parameter_matrix(B)
    return _LogLikKernel.apply(kernel.program, yerr is not None, P, x, yerr if diag is None else diag,
                               _per_series(jitter, B, y), _per_series(mean, B, y), y)


def _reduce(g, like):
    """Gradient of an argument that was shared by the batch (one fewer dimension): sum over the batch."""
    return g.sum(0) if like.dim() == g.dim() - 1 else g


class _Factor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, c, a, U, V):
        args = [x.detach().contiguous() for x in (t, c, a, U, V)]
        d, W, S, flag = ops.factor(*args, workspace=True)
        if bool((flag != 0).any()):
            err = LinAlgError("failed to factorize or solve matrix")
            err.flag = flag
            raise err
        ctx.save_for_backward(*args, d, W, S)
        return d, W

    @staticmethod
    def backward(ctx, bd, bW):
        t, c, a, U, V, d, W, S = ctx.saved_tensors
        bt, bc, ba, bU, bV = ops.factor_rev(t, c, a, U, V, d, W, S, bd.contiguous(), bW.contiguous())
        return _reduce(bt, t), _reduce(bc, c), ba, bU, bV


def factor(t, c, a, U, V):
    """(d, W) = LDL^T factors of the batch (forward.hpp:69-135), differentiable (reverse.hpp:10-85)."""
    return _Factor.apply(t, c, a, U, V)


def _sweep(name):
    fwd, rev = getattr(ops, name), getattr(ops, name + "_rev")

    class _Op(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, c, U, W, Y):
            args = [x.detach().contiguous() for x in (t, c, U, W, Y)]
            Z, F = fwd(*args, workspace=True, zero_z=True) if name.startswith("matmul") else fwd(*args, workspace=True)
            ctx.save_for_backward(*args, Z, F)
            return Z

        @staticmethod
        def backward(ctx, bZ):
            t, c, U, W, Y, Z, F = ctx.saved_tensors
            bt, bc, bU, bW, bY = rev(t, c, U, W, Y, Z, F, bZ.contiguous())
            return _reduce(bt, t), _reduce(bc, c), bU, bW, bY

    _Op.__name__ = "_" + name

    def op(t, c, U, W, Y):
        return _Op.apply(t, c, U, W, Y)

    op.__name__ = name
    op.__doc__ = "Batched %s (B,N,nrhs), differentiable w.r.t. (t, c, U, W|V, Y); internal.hpp:105-303." % name
    return op


solve_lower = _sweep("solve_lower")
solve_upper = _sweep("solve_upper")
matmul_lower = _sweep("matmul_lower")
matmul_upper = _sweep("matmul_upper")


class _InverseDiag(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, c, U, W, d, z):
        args = [None if x is None else x.detach().contiguous() for x in (t, c, U, W, d, z)]
        out = ops.inverse_diag(*args, workspace=True)
        q, alpha, (Mws, Fws) = (out[0], None, out[1]) if z is None else out
        ctx.hz = z is not None
        ctx.save_for_backward(*[x for x in (*args, q, alpha, Mws, Fws) if x is not None])
        return q if z is None else (q, alpha)

    @staticmethod
    def backward(ctx, bq, balpha=None):
        if ctx.hz:
            t, c, U, W, d, z, q, alpha, Mws, Fws = ctx.saved_tensors
            balpha = balpha.contiguous()
        else:
            t, c, U, W, d, q, Mws = ctx.saved_tensors
            z = alpha = Fws = balpha = None
        bt, bc, bU, bW, bd, bz = ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, (Mws, Fws), bq.contiguous(), balpha)
        return _reduce(bt, t), _reduce(bc, c), bU, bW, bd, bz


def inverse_diag(t, c, U, W, d, z=None):
    """q (B, N) = diag((K + D)^-1) from the factors (d, W) -- and with z (B, N), solve_lower of a residual, also
    alpha = (K + D)^-1 (y - mean): (q, alpha) -- differentiable in every argument (c2_inverse_diag_fwd forward,
    c2_inverse_diag_rev backward; a shared t / c receives the batch sum).  Composes with `factor` and `solve_lower`.
    The forward call keeps 8 B N J (J + 1) bytes for the backward pass: 2.4 MB per series at N = 4096, J = 8 -- chunk large
    batches.  J <= 32."""
    return _InverseDiag.apply(t, c, U, W, d, z)


def _loo_objective(q, alpha):
    return 0.5 * (torch.log(q) - alpha * alpha / q).sum(dim=1) - 0.5 * q.shape[1] * math.log(2.0 * math.pi)


def loo_log_predictive(t, c, a, U, V, y):
    """Leave-one-out log predictive density (B,), sum_n log N(y_n | y_n - alpha_n / q_n, 1 / q_n) with
    q = diag((K + D)^-1) and alpha = (K + D)^-1 y, differentiable in all six arguments: the chain
    factor -> solve_lower -> inverse_diag of this module (O(N J^2) per series each way).  Raises LinAlgError when a
    factorisation fails (as `factor`).  Workspace: see `inverse_diag`."""
    d, W = factor(t, c, a, U, V)
    z = solve_lower(t, c, U, W, y[..., None])[..., 0]
    q, alpha = inverse_diag(t, c, U, W, d, z)
    return _loo_objective(q, alpha)


class _LooKernel(torch.autograd.Function):
    """term_coefficients -> noise_mean[_shift]_apply -> get_celerite_matrices -> factor -> solve_lower -> inverse_diag ->
    the objective -> inverse_diag_rev -> solve_lower_rev -> factor_rev -> get_celerite_matrices_rev ->
    noise_mean[_shift]_rev / term_coefficients_rev as ONE node: the gradients come out of the forward call (as in
    _LogLikKernel), backward scales them by the incoming cotangent."""

    @staticmethod
    def forward(ctx, program, is_sigma, P, x, yerr, jitter, mean, y):
        tens = (P, x, yerr, jitter, mean, y)
        Pd, xd, ed, jd, md, yd = [None if v is None else v.detach().contiguous() for v in tens]
        B = y.shape[0]
        expr = isinstance(program, ops.TermExpr)
        grad = any(v is not None and v.requires_grad for v in tens)
        if expr:
            coefs, tflag, shift = ops.term_coefficients(program, Pd, B)
            diag, r = ops.noise_mean_shift_apply(ed, jd, md, shift, yd, yerr_is_sigma=is_sigma)
        else:
            diag, r = ops.noise_mean_apply(ed, jd, md, yd, yerr_is_sigma=is_sigma)
            coefs, tflag = ops.term_coefficients(program, Pd, B)
        ar, cr, ac, bc, cc, dc = coefs
        a, U, V = ops.get_celerite_matrices(ar, ac, bc, dc, xd, diag)
        c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1).contiguous()   # (terms.py:171-173)
        r3 = r[..., None]
        neg_inf = torch.full((B,), -math.inf, dtype=torch.float64, device=y.device)
        if not grad:
            d, W, flag = ops.factor(xd, c, a, U, V)
            z = ops.solve_lower(xd, c, U, W, r3)[..., 0]
            q, alpha = ops.inverse_diag(xd, c, U, W, d, z=z, alpha=z)
            return torch.where((flag != 0) | (tflag != 0), neg_inf, _loo_objective(q, alpha))
        d, W, S, flag = ops.factor(xd, c, a, U, V, workspace=True)
        z3, F = ops.solve_lower(xd, c, U, W, r3, workspace=True)
        z = z3[..., 0]
        q, alpha, ws = ops.inverse_diag(xd, c, U, W, d, z=z, workspace=True)
        loo = torch.where(flag != 0, neg_inf, _loo_objective(q, alpha))
        bq = 0.5 / q + 0.5 * alpha * alpha / (q * q)
        balpha = -alpha / q
        bt, bcv, bU, bW, bd, bz = ops.inverse_diag_rev(xd, c, U, W, d, z, q, alpha, ws, bq, balpha)
        bt2, bc2, bU2, bW2, bY = ops.solve_lower_rev(xd, c, U, W, r3, z3, F, bz[..., None])
        bt3, bc3, ba, bU3, bV = ops.factor_rev(xd, c, a, U, V, d, W, S, bd, bW + bW2)
        bar, bcr, bac, bbc, bcc, bdc, bx, bdiag = ops.get_celerite_matrices_rev(
            ac, bc, dc, xd, V, bt + bt2 + bt3, bcv + bc2 + bc3, ba, bU + bU2 + bU3, bV, program.Jr)
        by = bY[..., 0].contiguous()
        cots = [bar, bcr, bac, bbc, bcc, bdc]
        if expr:
            bj, bm, bs = ops.noise_mean_shift_rev(jd, bdiag, by, flag=flag, tflag=tflag)
            bP = ops.term_coefficients_rev(program, Pd, cots, tflag=tflag, lflag=flag, ll=loo, bshift=bs)
        else:
            bP = ops.term_coefficients_rev(program, Pd, cots, tflag=tflag, lflag=flag, ll=loo)
            bj, bm = ops.noise_mean_rev(jd, bdiag, by, flag=flag)
        ctx.shared_P, ctx.shared_x = P.dim() == 1, x.dim() == 1
        ctx.has = (jitter is not None, mean is not None)
        be = bdiag if not is_sigma else (2.0 * ed * bdiag if yerr.requires_grad else None)
        ctx.has_e = be is not None
        ctx.save_for_backward(flag, bP, bj, bm, bx, by, *([be] if be is not None else []))
        return loo

    backward = staticmethod(_LogLikKernel.backward)   # (the same saved tensors: dead series masked, shared P / x summed)


def loo_log_predictive_kernel(kernel, x, y, *, yerr=None, diag=None, jitter=None, mean=None):
    """Leave-one-out log predictive density (B,) as a differentiable function of the HYPER-PARAMETERS: the arguments and
    conventions of `log_likelihood_kernel` (tensor parameters of `kernel`, TermExpr kernels with their diagonal shift,
    `jitter` in quadrature, `mean`, x, yerr | diag, y), the objective of `loo_log_predictive`.  One autograd node; every step
    between the parameters and the gradient is a device kernel, the reverse of the inverse diagonal among them
    (csrc/c2_invdiag_rev.hip).  A series whose factorisation fails, or whose Q is on the wrong side of an SHO term's regime,
    has the value -inf and contributes zero gradient; the others are untouched.  The forward call keeps the workspaces of
    factor, solve_lower and inverse_diag, 8 B N J (2 J + 2) bytes together (inverse_diag's share: 8 B N J (J + 1), 2.4 MB per
    series at N = 4096, J = 8): chunk large batches.  J <= 32."""
    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, N) is required")
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B = y.shape[0]
    if not kernel._has_tensors():
        raise TypeError("loo_log_predictive_kernel: the kernel has no tensor parameter (give its parameters as device tensors)")
    P = kernel.parameter_matrix(B)
    return _LooKernel.apply(kernel.program, yerr is not None, P, x, yerr if diag is None else diag,
                            _per_series(jitter, B, y), _per_series(mean, B, y), y)


def _general(name):
    fwd, rev = getattr(ops, name), getattr(ops, name + "_rev")

    class _Op(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t1, t2, c, U, V, Y):
            args = [x.detach().contiguous() for x in (t1, t2, c, U, V, Y)]
            Z, F = fwd(*args, workspace=True, zero_z=True)
            ctx.save_for_backward(*args, F)
            return Z

        @staticmethod
        def backward(ctx, bZ):
            t1, t2, c, U, V, Y, F = ctx.saved_tensors
            bt1, bt2, bc, bU, bV, bY = rev(t1, t2, c, U, V, Y, F, bZ.contiguous())
            return _reduce(bt1, t1), _reduce(bt2, t2), _reduce(bc, c), bU, bV, bY

    _Op.__name__ = "_" + name

    def op(t1, t2, c, U, V, Y):
        return _Op.apply(t1, t2, c, U, V, Y)

    op.__name__ = name
    op.__doc__ = ("Batched %s (B, N, nrhs): the product that carries Y (B, M, nrhs) from the grid t2 ((M,) | (B, M)) to the grid t1\n"
                  "((N,) | (B, N)) (forward.hpp:285-392), differentiable w.r.t. (t1, t2, c, U, V, Y) -- forward with its workspace\n"
                  "F (B, M, J, nrhs), backward c2_%s_rev (csrc/c2_general_rev.hip).  Shared t1 / t2 / c receive the batch sum.\n"
                  "The result starts from zero (the ops layer accumulates into a caller's Z).  J <= 32." % (name, name))
    return op


general_matmul_lower = _general("general_matmul_lower")
general_matmul_upper = _general("general_matmul_upper")


class _CeleriteMatrices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ar, ac, bc, dc, x, diag):
        args = [v.detach().contiguous() for v in (ar, ac, bc, dc, x, diag)]
        a, U, V = ops.get_celerite_matrices(*args)
        ctx.save_for_backward(*args[:5], V)
        return a, U, V

    @staticmethod
    def backward(ctx, ba, bU, bV):
        ar, ac, bc, dc, x, V = ctx.saved_tensors
        B, N, J = V.shape
        zt, zc = torch.zeros((B, N), dtype=V.dtype, device=V.device), torch.zeros((B, J), dtype=V.dtype, device=V.device)
        bar, _, bac, bbc, _, bdc, bx, bdiag = ops.get_celerite_matrices_rev(
            ac, bc, dc, x, V, zt, zc, ba.contiguous(), bU.contiguous(), bV.contiguous(), ar.shape[-1])
        return _reduce(bar, ar), _reduce(bac, ac), _reduce(bbc, bc), _reduce(bdc, dc), _reduce(bx, x), bdiag


def get_celerite_matrices(ar, ac, bc, dc, x, diag):
    """(a (B, N), U, V (B, N, J)) from the celerite coefficients ar (Jr,) | (B, Jr), ac, bc, dc (Jc,) | (B, Jc), the times
    x (N,) | (B, N) and the diagonal diag (B, N) (ops.get_celerite_matrices), differentiable in all six
    (c2_get_celerite_matrices_rev; shared arguments receive the batch sum).  The decay rates c = (cr, cc, cc) do not pass
    through it: build them in torch.  The glue between `term_coefficients` and `factor` / `general_matmul_*`."""
    return _CeleriteMatrices.apply(ar, ac, bc, dc, x, diag)


def predict_mean(t, c, a, U, V, y, ts, Us, Vs):
    """The conditional mean (B, M) at the sorted times ts ((M,) | (B, M)) of the process with the semiseparable matrix
    (t, c, a, U, V) given y (B, N): K(ts, t) (K + D)^-1 y, as the chain factor -> solve_lower -> / d -> solve_upper ->
    general_matmul_lower + general_matmul_upper of this module, differentiable in all nine arguments.  Us, Vs (B, M, J):
    the kernel's rows at ts.  O((N + M) J^2) per series each way, no N x M array.  Raises LinAlgError when a factorisation
    fails (as `factor`).  J <= 32."""
    d, W = factor(t, c, a, U, V)
    z = solve_lower(t, c, U, W, y[..., None])
    alpha = solve_upper(t, c, U, W, z / d[..., None])
    return (general_matmul_lower(ts, t, c, Us, V, alpha) + general_matmul_upper(ts, t, c, Vs, U, alpha))[..., 0]


def predict_mean_kernel(kernel, x, y, t, *, yerr=None, diag=None, jitter=None, mean=None):
    """The conditional mean (B, M) at the sorted times t ((M,) | (B, M)) given y (B, N) at x, as a differentiable function of
    the HYPER-PARAMETERS: the arguments and conventions of `log_likelihood_kernel` (tensor parameters of `kernel`, TermExpr
    kernels with their diagonal shift, `jitter` in quadrature, `mean` added back), differentiable in the parameters, jitter,
    mean, y, x and t (and yerr | diag).  The composed chain term_coefficients -> get_celerite_matrices (at x and at t) ->
    `predict_mean`; every step with a recurrence is a device kernel with its reverse.  A failed factorisation raises
    LinAlgError.  J <= 32."""
    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, N) is required")
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != y.shape[0]):
        raise ValueError("Invalid shape: t (must be (M,) or (B, M))")
    B = y.shape[0]
    if not kernel._has_tensors():
        raise TypeError("predict_mean_kernel: the kernel has no tensor parameter (give its parameters as device tensors)")
    ar, cr, ac, bc, cc, dc, shift = term_coefficients(kernel.program, kernel.parameter_matrix(B), B, with_shift=True)
    D = (yerr * yerr if diag is None else diag) + shift[:, None]
    jitter, mean = _per_series(jitter, B, y), _per_series(mean, B, y)
    if jitter is not None:
        D = D + (jitter * jitter)[:, None]
    r = y if mean is None else y - mean[:, None]
    c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1)   # (terms.py:171-173)
    a, U, V = get_celerite_matrices(ar, ac, bc, dc, x, D)
    _, Us, Vs = get_celerite_matrices(ar, ac, bc, dc, t, torch.zeros((B, t.shape[-1]), dtype=y.dtype, device=y.device))
    mu = predict_mean(x, c, a, U, V, r, t, Us, Vs)
    return mu if mean is None else mu + mean[:, None]


class _ExplainedVariance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, ts, c, U, W, d, Us, Vs):
        args = [x.detach().contiguous() for x in (t, ts, c, U, W, d, Us, Vs)]
        work = torch.empty_like(args[6])
        r, (Sws, Rws) = ops.explained_variance(*args, work=work, workspace=True)
        ctx.save_for_backward(*args, work, Sws, Rws)
        return r

    @staticmethod
    def backward(ctx, br):
        t, ts, c, U, W, d, Us, Vs, work, Sws, Rws = ctx.saved_tensors
        bt, bts, bc, bU, bW, bd, bUs, bVs = ops.explained_variance_rev(t, ts, c, U, W, d, Us, Vs, work, (Sws, Rws), br.contiguous())
        return _reduce(bt, t), _reduce(bts, ts), _reduce(bc, c), bU, bW, bd, bUs, bVs


def explained_variance(t, ts, c, U, W, d, Us, Vs):
    """r (B, M) = diag(K*^T (K + D)^-1 K*) at the sorted times ts ((M,) | (B, M)) from the factors (d, W) on t, differentiable
    in all eight arguments (c2_explained_variance_fwd forward, c2_explained_variance_rev backward, csrc/c2_predvar_rev.hip;
    shared t / ts / c receive the batch sum).  Composes with `factor`.  The forward call keeps 16 B N J^2 bytes for the
    backward pass: 4.2 MB per series at N = 4096, J = 8 -- chunk large batches.  J <= 32."""
    return _ExplainedVariance.apply(t, ts, c, U, W, d, Us, Vs)


def predict_variance(t, c, a, U, V, ts, Us, Vs, k0):
    """The conditional variance (B, M) at the sorted times ts ((M,) | (B, M)) of the process with the semiseparable matrix
    (t, c, a, U, V): k0 - K(ts, t) (K + D)^-1 K(t, ts) on the diagonal, as the chain factor -> explained_variance of this
    module, differentiable in all nine arguments.  k0 (B,) | float: the kernel at lag 0.  Us, Vs (B, M, J): the kernel's rows at
    ts.  O((N + M) J^2) per series each way, no N x M array.  Raises LinAlgError when a factorisation fails (as `factor`).
    Workspace: see `explained_variance`.  J <= 32."""
    d, W = factor(t, c, a, U, V)
    r = explained_variance(t, ts, c, U, W, d, Us, Vs)
    return (k0[:, None] if torch.is_tensor(k0) and k0.dim() == 1 else k0) - r


def _log_density(ys, mu, var):
    return -0.5 * ((ys - mu) ** 2 / var + torch.log(var)).sum(dim=1) - 0.5 * ys.shape[1] * math.log(2.0 * math.pi)


def predictive_log_density(t, c, a, U, V, y, ts, Us, Vs, k0, ys, vars=None):
    """The held-out log predictive density (B,): sum_m log N(ys_m | mu_m, k0 - r_m + vars_m) with mu = `predict_mean` and
    k0 - r = `predict_variance` at the sorted times ts, ys (B, M) the held-out values and vars (B, M) | None their noise
    variances -- differentiable in every tensor argument.  The objective itself is plain torch on (B, M) arrays.  Raises
    LinAlgError when a factorisation fails.  J <= 32."""
    mu = predict_mean(t, c, a, U, V, y, ts, Us, Vs)
    var = predict_variance(t, c, a, U, V, ts, Us, Vs, k0)
    return _log_density(ys, mu, var if vars is None else var + vars)


def _has_convolution(kernel):
    """Is there a TermConvolution anywhere in the kernel's tree?"""
    from .terms import TermConvolution
    if isinstance(kernel, TermConvolution):
        return True
    kids = list(getattr(kernel, "terms", None) or []) + [getattr(kernel, nm, None) for nm in ("term", "term1", "term2")]
    return any(_has_convolution(k) for k in kids if k is not None)


def _predict_chain(name, kernel, x, y, t, yerr, diag, jitter, mean):
    """predict_mean_kernel's conventions: (c, a, U, V, r, Us, Vs, k0, jitter, mean) of the coefficient-level chain."""
    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, N) is required")
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != y.shape[0]):
        raise ValueError("Invalid shape: t (must be (M,) or (B, M))")
    if _has_convolution(kernel):
        raise ValueError("%s does not take a kernel with a TermConvolution in it (not semiseparable inside the exposure "
                         "window): use predict(y, t, return_var=True)" % name)
    B = y.shape[0]
    if not kernel._has_tensors():
        raise TypeError("%s: the kernel has no tensor parameter (give its parameters as device tensors)" % name)
    ar, cr, ac, bc, cc, dc, shift = term_coefficients(kernel.program, kernel.parameter_matrix(B), B, with_shift=True)
    D = (yerr * yerr if diag is None else diag) + shift[:, None]
    jitter, mean = _per_series(jitter, B, y), _per_series(mean, B, y)
    if jitter is not None:
        D = D + (jitter * jitter)[:, None]
    r = y if mean is None else y - mean[:, None]
    c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1)   # (terms.py:171-173)
    a, U, V = get_celerite_matrices(ar, ac, bc, dc, x, D)
    _, Us, Vs = get_celerite_matrices(ar, ac, bc, dc, t, torch.zeros((B, t.shape[-1]), dtype=y.dtype, device=y.device))
    k0 = ar.sum(dim=-1) + ac.sum(dim=-1)
    return c, a, U, V, r, Us, Vs, k0, jitter, mean


def predict_variance_kernel(kernel, x, y, t, *, yerr=None, diag=None, jitter=None, mean=None):
    """The conditional variance (B, M) of the process at the sorted times t ((M,) | (B, M)) as a differentiable function of
    the HYPER-PARAMETERS, `predict_mean_kernel`'s arguments and chain with `predict_variance` at its end (y and mean only
    give the batch size: the variance does not depend on them)."""
    c, a, U, V, _, Us, Vs, k0, _, _ = _predict_chain("predict_variance_kernel", kernel, x, y, t, yerr, diag, jitter, mean)
    return predict_variance(x, c, a, U, V, t, Us, Vs, k0)


def predictive_log_density_kernel(kernel, x, y, t, ys, *, yerr=None, diag=None, jitter=None, mean=None, yerr_new=None):
    """The held-out log predictive density (B,), sum_m log N(ys_m | mu_m, var_m + yerr_new_m^2 + jitter^2), of the values
    ys (B, M) at the sorted times t ((M,) | (B, M)) given y (B, N) at x, as a differentiable function of the
    HYPER-PARAMETERS: the arguments and conventions of `predict_mean_kernel` (tensor parameters of `kernel`, `jitter` in
    quadrature, `mean`), the queries' own noise yerr_new (B, M) | None with the same jitter added in quadrature (or none).
    Differentiable in the parameters, jitter, mean, y, ys, x and t (and yerr | diag, yerr_new).  The chain
    term_coefficients -> get_celerite_matrices (at x and at t) -> `predict_mean` and `predict_variance` -> the objective in
    torch; every step with a recurrence is a device kernel with its reverse, the reverse of the explained variance among
    them (csrc/c2_predvar_rev.hip).  A failed factorisation raises LinAlgError.  A kernel with a TermConvolution anywhere in
    it is refused: use predict(y, t, return_var=True).  Workspace: see `explained_variance`.  J <= 32."""
    if ys.dim() != 2 or ys.shape[0] != y.shape[0] or ys.shape[1] != t.shape[-1]:
        raise ValueError("Invalid shape: ys (must be (B, M))")
    c, a, U, V, r, Us, Vs, k0, jitter, mean = _predict_chain("predictive_log_density_kernel", kernel, x, y, t, yerr, diag,
                                                               jitter, mean)
    noise = None if yerr_new is None else yerr_new * yerr_new
    if jitter is not None:
        j2 = (jitter * jitter)[:, None]
        noise = j2 if noise is None else noise + j2
    rs = ys if mean is None else ys - mean[:, None]
    return predictive_log_density(x, c, a, U, V, r, t, Us, Vs, k0, rs, noise)


class _WhitenedGram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, c, U, W, d, A, y):
        args = [None if x is None else x.detach().contiguous() for x in (t, c, U, W, d, A, y)]
        S = ops.whitened_gram(*args)
        ctx.hy = y is not None
        ctx.save_for_backward(*[x for x in args if x is not None])
        return S

    @staticmethod
    def backward(ctx, bS):
        t, c, U, W, d, A, *rest = ctx.saved_tensors
        B, N, P = U.shape[0], U.shape[1], A.shape[-1]
        Y = torch.cat([A.expand(B, N, P)] + [y[..., None] for y in rest], dim=-1).contiguous()
        Z, F = ops.solve_lower(t, c, U, W, Y, workspace=True)
        bZ = torch.matmul(Z, bS + bS.transpose(1, 2)) / d[..., None]
        bd = -(torch.matmul(Z, bS) * Z).sum(dim=-1) / (d * d)
        bt, bc, bU, bW, bY = ops.solve_lower_rev(t, c, U, W, Y, Z, F, bZ.contiguous())
        return (_reduce(bt, t), _reduce(bc, c), bU, bW, bd, _reduce(bY[..., :P], A), bY[..., P] if ctx.hy else None)


def whitened_gram(t, c, U, W, d, A, y=None):
    """S (B, Q, Q) = [A | y]^T (K + D)^-1 [A | y] from the factors (d, W) of `factor`, differentiable in every argument.
    A (N, P) shared by the batch | (B, N, P); y (B, N) | None (Q = P + 1 with y, its column last).  The forward call is the
    fused sweep (c2_whitened_gram: S accumulates in registers, L^-1 [A | y] is never written) and keeps only its inputs.
    The backward pass is composed from reverses that exist: it recomputes Z = solve_lower([A | y]) with its workspace, then
    bZ = Z (bS + bS^T) / d, bd_n = -(z_n^T bS z_n) / d_n^2 and solve_lower_rev; a shared t / c / A receives the batch sum.
    J <= 32 and Q <= 32."""
    return _WhitenedGram.apply(t, c, U, W, d, A, y)


LinearFit = collections.namedtuple("LinearFit", "beta cov log_likelihood marginal_log_likelihood")

# A Cholesky pivot of H below this fraction of H's own diagonal entry: the column is a combination of those before it to
# twelve digits, the coefficients keep fewer than four -- H counts as rank-deficient.
_RANK_TOL = 1e-12


def _linear_fit(S, log_det, N, prior_mean=None, prior_precision=None, ok=None):
    """`gls` on the Gram matrix S (B, P + 1, P + 1) of [A | y - A mu0], log_det (B,) = sum log d and the series length N:
    (LinearFit, bad) with bad (B,) marking the series whose H = S_AA + Lambda is not positive definite or is
    rank-deficient (_RANK_TOL).  `ok` (B,) | None: series to take at all (the others count as bad; their S is not read).
    Plain torch on (B, Q, Q) arrays, differentiable; bad series hold NaN / -inf."""
    B, Q = S.shape[0], S.shape[-1]
    P = Q - 1
    eye = torch.eye(P, dtype=S.dtype, device=S.device)
    if ok is not None:
        S = torch.where(ok[:, None, None], S, torch.eye(Q, dtype=S.dtype, device=S.device))
    S_AA, s_Ay, s_yy = S[:, :P, :P], S[:, :P, P], S[:, P, P]
    H = S_AA if prior_precision is None else S_AA + prior_precision
    Lc, info = torch.linalg.cholesky_ex(H)
    bad = info != 0
    bad = bad | ~((torch.diagonal(Lc, dim1=-2, dim2=-1) ** 2 > _RANK_TOL * torch.diagonal(H, dim1=-2, dim2=-1)).all(dim=-1))
    if ok is not None:
        bad = bad | ~ok
    if bool(bad.any()):   # (the solves below stay finite: a bad series is solved against the identity, then overwritten)
        Lc = torch.where(bad[:, None, None], eye, Lc)
    delta = torch.cholesky_solve(s_Ay[..., None], Lc)[..., 0]
    cov = torch.cholesky_solve(eye.expand(B, P, P), Lc)
    beta = delta if prior_mean is None else prior_mean + delta
    ll = -0.5 * (s_yy - (s_Ay * delta).sum(dim=-1)) - 0.5 * log_det - 0.5 * N * math.log(2.0 * math.pi)
    log_det_H = 2.0 * torch.log(torch.diagonal(Lc, dim1=-2, dim2=-1)).sum(dim=-1)
    if prior_precision is None:
        mll = ll - 0.5 * log_det_H + 0.5 * P * math.log(2.0 * math.pi)
    else:
        mll = ll - 0.5 * log_det_H + 0.5 * torch.linalg.slogdet(prior_precision)[1]
    if bool(bad.any()):
        nan = torch.full((), math.nan, dtype=S.dtype, device=S.device)
        ninf = torch.full((), -math.inf, dtype=S.dtype, device=S.device)
        beta, cov = torch.where(bad[:, None], nan, beta), torch.where(bad[:, None, None], nan, cov)
        ll, mll = torch.where(bad, ninf, ll), torch.where(bad, ninf, mll)
    return LinearFit(beta, cov, ll, mll), bad


def _check_design(A, B, N, prior_mean, prior_precision):
    """"Invalid shape: A" and the prior's shapes; returns P."""
    if A.dim() not in (2, 3) or tuple(A.shape[-2:-1]) != (N,) or (A.dim() == 3 and A.shape[0] != B) or A.shape[-1] < 1:
        raise ValueError("Invalid shape: A %s (must be (N, P) or (B, N, P) with (B, N) = %s, P >= 1)" % (tuple(A.shape), (B, N)))
    P = A.shape[-1]
    if prior_mean is not None and tuple(prior_mean.shape) not in ((P,), (B, P)):
        raise ValueError("Invalid shape: prior_mean %s (must be (P,) or (B, P))" % (tuple(prior_mean.shape),))
    if prior_precision is not None and tuple(prior_precision.shape) not in ((P, P), (B, P, P)):
        raise ValueError("Invalid shape: prior_precision %s (must be (P, P) or (B, P, P))" % (tuple(prior_precision.shape),))
    return P


def _prior_residual(y, A, prior_mean):
    """r = y - A mu0 (one matmul), y itself without a prior mean."""
    return y if prior_mean is None else y - torch.matmul(A, prior_mean[..., None])[..., 0]


def gls(t, c, a, U, V, A, y, *, prior_mean=None, prior_precision=None):
    """Generalized least squares of y (B, N) on the design matrix A ((N, P) shared | (B, N, P)) under the covariance
    (t, c, a, U, V): LinearFit(beta (B, P), cov (B, P, P), log_likelihood (B,), marginal_log_likelihood (B,)),
    differentiable in every tensor argument.  The chain `factor` -> `whitened_gram` -> torch on (B, Q, Q): a batched P x P
    Cholesky, outside the hot path.  With S_AA, s_Ay, s_yy the blocks of the Gram matrix of [A | r], r = y - A mu0,
    mu0 = prior_mean ((P,) | (B, P)), Lambda = prior_precision ((P, P) | (B, P, P)) and H = S_AA + Lambda (a flat prior:
    mu0 = 0, Lambda = 0):

        beta = mu0 + H^-1 s_Ay,      cov = H^-1
        log_likelihood          = -(s_yy - s_Ay^T H^-1 s_Ay) / 2 - sum log d / 2 - N log(2 pi) / 2
        marginal_log_likelihood = log_likelihood - logdet H / 2 + logdet Lambda / 2          (Gaussian prior)
                                = log_likelihood - logdet S_AA / 2 + P log(2 pi) / 2         (flat prior)

    `log_likelihood` is the profiled one: log N(y | A beta, K + D) at beta under a flat prior; with a Gaussian prior the
    same expression carries the prior's quadratic term -(beta - mu0)^T Lambda (beta - mu0) / 2 at beta.  The Gaussian-prior
    marginal is log N(y | A mu0, K + D + A Lambda^-1 A^T).  Raises LinAlgError when a factorisation fails (as `factor`) or
    an H is not positive definite to twelve digits (rank-deficient A); `.flag` marks the series.  J <= 32 and P <= 31."""
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B, N = y.shape
    _check_design(A, B, N, prior_mean, prior_precision)
    d, W = factor(t, c, a, U, V)
    S = whitened_gram(t, c, U, W, d, A, _prior_residual(y, A, prior_mean))
    fit, bad = _linear_fit(S, torch.log(d).sum(dim=1), N, prior_mean, prior_precision)
    if bool(bad.any()):
        err = LinAlgError("failed to factorize or solve matrix (rank-deficient design matrix)")
        err.flag = bad.to(torch.int32)
        raise err
    return fit


def marginal_log_likelihood_kernel(kernel, x, y, A, *, yerr=None, diag=None, jitter=None, mean=None, prior_mean=None,
                                   prior_precision=None, profiled=False):
    """The log-likelihood (B,) of y (B, N) at x under `kernel` plus a LINEAR mean model mean + A beta, with the coefficients
    beta marginalised out (`profiled=False`: `gls`'s marginal_log_likelihood, under the Gaussian prior (prior_mean,
    prior_precision) or a flat one) or set to their generalized-least-squares value (`profiled=True`: its log_likelihood) --
    a differentiable function of the HYPER-PARAMETERS alone, with `predict_mean_kernel`'s conventions (tensor parameters of
    `kernel`, TermExpr kernels with their diagonal shift, `jitter` in quadrature, `mean` subtracted).  Differentiable in the
    parameters, jitter, mean, y, A, x (and yerr | diag, the prior).  The chain term_coefficients -> get_celerite_matrices ->
    `gls`.  A TermConvolution is allowed: only the factored matrix is used.  Raises LinAlgError as `gls`.  J <= 32, P <= 31."""
    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, N) is required")
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B, N = y.shape
    _check_design(A, B, N, prior_mean, prior_precision)
    if not kernel._has_tensors():
        raise TypeError("marginal_log_likelihood_kernel: the kernel has no tensor parameter (give its parameters as device tensors)")
    ar, cr, ac, bc, cc, dc, shift = term_coefficients(kernel.program, kernel.parameter_matrix(B), B, with_shift=True)
    D = (yerr * yerr if diag is None else diag) + shift[:, None]
    jitter, mean = _per_series(jitter, B, y), _per_series(mean, B, y)
    if jitter is not None:
        D = D + (jitter * jitter)[:, None]
    r = y if mean is None else y - mean[:, None]
    c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1)   # (terms.py:171-173)
    a, U, V = get_celerite_matrices(ar, ac, bc, dc, x, D)
    fit = gls(x, c, a, U, V, A, r, prior_mean=prior_mean, prior_precision=prior_precision)
    return fit.log_likelihood if profiled else fit.marginal_log_likelihood


# ---- streaming updates (csrc/c2_filter.hip forward, csrc/c2_filter_rev.hip backward) -------------------------------------------
class _FilterAppend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, t, c, a, U, V, y, count):
        args = [x.detach().contiguous() for x in (state, t, c, a, U, V, y)]
        out, d, W, z, flag = ops.filter_append(*args, count=count)   # out of place: the entry state is what backward reads
        ctx.count = count
        ctx.save_for_backward(args[0], args[1], args[2], args[4], W, d, z, flag)
        ctx.mark_non_differentiable(flag)
        return out, d, W, z, flag

    @staticmethod
    def backward(ctx, bstate, bd, bW, bz, _bflag=None):
        state, t, c, U, W, d, z, flag = ctx.saved_tensors
        bsi, bt, bc, ba, bU, bV, by = ops.filter_append_rev(state, t, c, U, W, d, z, flag, bstate.contiguous(), bd.contiguous(),
                                                            bW.contiguous(), bz.contiguous(), count=ctx.count)
        return bsi, _reduce(bt, t), _reduce(bc, c), ba, bU, bV, by, None


def filter_append(state, t, c, a, U, V, y, *, count=None):
    """ops.filter_append out of place, -> (state_out, d, W, z, flag), differentiable in state, t, c, a, U, V, y
    (c2_filter_append_rev; shared t / c receive the batch sum).  The cotangent of a state is carried from one call to the
    previous one, so a loss on a later state -- -(1/2) ([3] + [2] + n log 2 pi) of its words is the log-likelihood of every
    row absorbed -- or on the d and z of any call flows back through as many calls as states were kept; `state.detach()`
    cuts it.  The rows m >= count[b] of d, W, z are uninitialised and receive no gradient.  flag (B,) int32 is not
    differentiable and nothing is raised: a series whose call failed (flag != 0) keeps its state, passes its state
    cotangent through and gives zero row gradients; the others are untouched.  J <= 32."""
    return _FilterAppend.apply(state, t, c, a, U, V, y, count)


def filter_append_kernel(kernel, state, t_new, y_new, *, yerr=None, diag=None, jitter=None, mean=None, count=None):
    """`filter_append` as a differentiable function of the HYPER-PARAMETERS, with `log_likelihood_kernel`'s conventions
    (tensor parameters of `kernel`, TermExpr kernels with their diagonal shift, `jitter` in quadrature, `mean` subtracted):
    the rows t_new (M,) | (B, M), y_new (B, M) with noise yerr | diag (B, M) appended to `state` -> (state_out, d, W, z, flag).
    Differentiable in the parameters, jitter, mean, the state, t_new, y_new and the noise.  The chain term_coefficients ->
    get_celerite_matrices -> `filter_append`, c built in torch.  A kernel with a TermConvolution anywhere in it is refused.
    J <= 32."""
    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, M) is required")
    if y_new.dim() != 2:
        raise ValueError("Invalid shape: y_new (must be (B, M))")
    if t_new.dim() not in (1, 2) or (t_new.dim() == 2 and t_new.shape[0] != y_new.shape[0]):
        raise ValueError("Invalid shape: t_new (must be (M,) or (B, M))")
    if _has_convolution(kernel):
        raise ValueError("filter_append_kernel does not take a kernel with a TermConvolution in it (not semiseparable inside "
                         "the exposure window): use predict(y, t, return_var=True)")
    B = y_new.shape[0]
    if not kernel._has_tensors():
        raise TypeError("filter_append_kernel: the kernel has no tensor parameter (give its parameters as device tensors)")
    ar, cr, ac, bc, cc, dc, shift = term_coefficients(kernel.program, kernel.parameter_matrix(B), B, with_shift=True)
    D = (yerr * yerr if diag is None else diag) + shift[:, None]
    jitter, mean = _per_series(jitter, B, y_new), _per_series(mean, B, y_new)
    if jitter is not None:
        D = D + (jitter * jitter)[:, None]
    r = y_new if mean is None else y_new - mean[:, None]
    c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1)   # (terms.py:171-173)
    a, U, V = get_celerite_matrices(ar, ac, bc, dc, t_new, D)
    return filter_append(state, t_new, c, a, U, V, r, count=count)


def _filter_rows(name, kernel, B, t, like, yerr, diag, jitter, mean, *, noise_required=True):
    """filter_append_kernel's conventions and refusals for the rows at t ((M,) | (B, M)) -> (c, a, U, V, jitter, mean) of the
    coefficient-level chain term_coefficients -> get_celerite_matrices, the diagonal a = k(0) + noise + jitter^2 (without
    noise, where that is allowed: a = k(0), and the jitter is not added)."""
    if noise_required and (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (B, M) is required")
    if yerr is not None and diag is not None:
        raise ValueError("only one of 'diag' and 'yerr' can be provided")
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != B):
        raise ValueError("Invalid shape: t (must be (M,) or (B, M))")
    if _has_convolution(kernel):
        raise ValueError("%s does not take a kernel with a TermConvolution in it (not semiseparable inside the exposure "
                         "window): use predict(y, t, return_var=True)" % name)
    if not kernel._has_tensors():
        raise TypeError("%s: the kernel has no tensor parameter (give its parameters as device tensors)" % name)
    ar, cr, ac, bc, cc, dc, shift = term_coefficients(kernel.program, kernel.parameter_matrix(B), B, with_shift=True)
    jitter, mean = _per_series(jitter, B, like), _per_series(mean, B, like)
    if yerr is None and diag is None:
        D = torch.zeros((B, t.shape[-1]), dtype=like.dtype, device=like.device)
    else:
        D = (yerr * yerr if diag is None else diag) + shift[:, None]
        if jitter is not None:
            D = D + (jitter * jitter)[:, None]
    c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1)   # (terms.py:171-173)
    a, U, V = get_celerite_matrices(ar, ac, bc, dc, t, D)
    return c, a, U, V, jitter, mean


# ---- forecast and absorb (csrc/c2_filter.hip forward, csrc/c2_filter_stream_rev.hip backward) ----------------------------------
class _FilterForecast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, t, c, a, U, count):
        args = [x.detach().contiguous() for x in (state, t, c, a, U)]
        # (rows beyond count are not written by the kernel: zeros there)
        mu, var = (None, None) if count is None else (torch.zeros_like(args[3]), torch.zeros_like(args[3]))
        mu, var = ops.filter_forecast(*args, count=count, mu=mu, var=var)
        ctx.count = count
        ctx.save_for_backward(args[0], args[1], args[2], args[4])
        return mu, var

    @staticmethod
    def backward(ctx, bmu, bvar):
        state, t, c, U = ctx.saved_tensors
        bs, bt, bc, ba, bU = ops.filter_forecast_rev(state, t, c, U, bmu.contiguous(), bvar.contiguous(), count=ctx.count)
        return bs, _reduce(bt, t), _reduce(bc, c), ba, bU, None


def filter_forecast(state, t, c, a, U, *, count=None):
    """ops.filter_forecast -> (mu, var) (B, M), differentiable in state, t, c, a, U (c2_filter_forecast_rev; shared t / c
    receive the batch sum).  The state is read and left: its cotangent adds to that of whatever else the state feeds, so the
    log density of what arrives h nights after a forecast trains everything the state was built from.  Rows m >= count[b]
    are zeros and receive no gradient.  J <= 32."""
    return _FilterForecast.apply(state, t, c, a, U, count)


class _FilterAbsorb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, t, c, W, d, z, count):
        args = [x.detach().contiguous() for x in (state, t, c, W, d, z)]
        out = ops.filter_absorb(*args, count=count)   # out of place: the entry state is what backward reads
        ctx.count = count
        ctx.save_for_backward(*args)
        return out

    @staticmethod
    def backward(ctx, bstate):
        state, t, c, W, d, z = ctx.saved_tensors
        bsi, bt, bc, bW, bd, bz = ops.filter_absorb_rev(state, t, c, W, d, z, bstate.contiguous(), count=ctx.count)
        return bsi, _reduce(bt, t), _reduce(bc, c), bW, bd, bz, None


def filter_absorb(state, t, c, W, d, z, *, count=None):
    """ops.filter_absorb out of place -> state_out, differentiable in state, t, c, W, d, z (c2_filter_absorb_rev; shared
    t / c receive the batch sum): a filter warm-started from a factored archive sends its gradient back into the archive's
    rows.  The state cotangent is carried as in `filter_append`.  Workspace of the backward call: 8 M (J + J^2) bytes per
    series.  J <= 32."""
    return _FilterAbsorb.apply(state, t, c, W, d, z, count)


def filter_forecast_kernel(kernel, state, t, *, yerr=None, diag=None, jitter=None, mean=None, count=None):
    """`filter_forecast` as a differentiable function of the HYPER-PARAMETERS, with `filter_append_kernel`'s conventions and
    refusals: (mu, var) (B, M) at the times t (M,) | (B, M), each row independently from `state`.  Without noise `var` is
    the latent variance and no jitter is added; with yerr | diag (B, M) it is the variance of a would-be observation,
    jitter^2 included.  `mu` includes `mean`.  Differentiable in the parameters, jitter, mean, the state, t and the noise.
    The chain term_coefficients -> get_celerite_matrices -> `filter_forecast`, c built in torch.  J <= 32."""
    if state.dim() != 2:
        raise ValueError("Invalid shape: state (must be (B, SW))")
    B = state.shape[0]
    c, a, U, _, _, mean = _filter_rows("filter_forecast_kernel", kernel, B, t, state, yerr, diag, jitter, mean,
                                       noise_required=False)
    mu, var = filter_forecast(state, t, c, a, U, count=count)
    return (mu if mean is None else mu + mean[:, None]), var


def filter_absorb_kernel(kernel, x, y, *, yerr=None, diag=None, jitter=None, mean=None):
    """The filter state (B, SW) behind the whole series y (B, N) at x (N,) | (B, N) as a differentiable function of the
    HYPER-PARAMETERS, `log_likelihood_kernel`'s arguments and conventions: the chain term_coefficients ->
    get_celerite_matrices -> `factor` -> `solve_lower` -> `filter_absorb` from the empty state, so -(1/2) ([3] + [2] + n log 2 pi)
    of its words is the log-likelihood of the series, and rows appended or forecast behind it send their gradient back
    through it.  A failed factorisation raises LinAlgError.  A kernel with a TermConvolution anywhere in it is refused.
    J <= 32."""
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B = y.shape[0]
    c, a, U, V, _, mean = _filter_rows("filter_absorb_kernel", kernel, B, x, y, yerr, diag, jitter, mean)
    r = y if mean is None else y - mean[:, None]
    d, W = factor(x, c, a, U, V)
    z = solve_lower(x, c, U, W, r[..., None])[..., 0]
    return filter_absorb(ops.filter_init(B, U.shape[-1], y.device), x, c, W, d, z)
