# -*- coding: utf-8 -*-
"""Kernel terms -> celerite matrices (c, a, U, V), on the device.

A minimal mirror of the reference's term algebra (python/celerite2/terms.py): each term exposes
`get_coefficients() -> (ar, cr, ac, bc, cc, dc)`; sums concatenate coefficient lists (terms.py:233-235);
`get_celerite_matrices(x, diag)` fills c with the reference's interleaved layout (terms.py:171-173) and runs
the c2_get_celerite_matrices kernel (driver.cpp:422-477) for (a, U, V).  Parameters may be python floats
(one kernel shared by the batch) or 1-D arrays of length B (one hyper-parameter draw per series).

Parameters may also be float64 torch TENSORS on the device, 0-d (shared) or (B,), with or without requires_grad: the
reference's jax / pymc term classes (python/celerite2/jax/terms.py, pymc/terms.py) on this backend.  A kernel with any
tensor parameter is flattened ONCE into a term program (ops.TermProgram); `coefficients(B)` forms its six coefficient
arrays on the device by one kernel (csrc/c2_term_params.hip), differentiable in every tensor parameter, and nothing is
read back to the host.  With floats / numpy arrays every path below runs as it always did.

Term ALGEBRA (terms.py:238-482): `t1 * t2` / TermProduct, TermDiff and TermConvolution, nested freely with sums (a
convolution only as the outermost term).  With floats / numpy arrays they map coefficient arrays on the host; with tensor
parameters the kernel becomes an expression (ops.TermExpr: the leaf records plus operation records) that
csrc/c2_term_expr.hip evaluates and differentiates on the device.  A kernel without them is a TermProgram as before.
"""
import math

import numpy as np

__all__ = ["Term", "TermSum", "TermProduct", "TermDiff", "TermConvolution", "RealTerm", "ComplexTerm", "SHOTerm", "Matern32Term",
           "RotationTerm"]

_CONV_OUTER = "You cannot perform operations on an TermConvolution, it must be the outer term in the kernel"


def _col(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float64))


def _is_tensor(v):
    return hasattr(v, "requires_grad") and hasattr(v, "device")


class Term:
    """Base class: subclasses implement get_coefficients() returning six arrays of shape (Jr,)|(B,Jr) / (Jc,)|(B,Jc)."""

    def get_coefficients(self):
        raise NotImplementedError

    def __add__(self, other):
        return TermSum(self, other)

    def __mul__(self, other):
        return TermProduct(self, other)

    @property
    def width(self):
        if self._has_tensors():
            return self.program.width
        ar, _, ac, _, _, _ = self.get_coefficients()
        return ar.shape[-1] + 2 * ac.shape[-1]

    # -- tensor parameters: the device path -------------------------------------------------------------------------
    def _records(self, add):
        """The term's records for ops.TermProgram; `add(value)` registers a parameter and returns its column of P."""
        raise NotImplementedError

    def _has_tensors(self):
        return any(_is_tensor(v) or (isinstance(v, tuple) and any(_is_tensor(w) for w in v)) for v in self.__dict__.values())

    def _no_host(self):
        if self._has_tensors():
            raise TypeError("this kernel has tensor parameters: its coefficients live on the device -- use coefficients(B)")

    def _build_program(self):
        cached = self.__dict__.get("_program")
        if cached is None:
            from . import ops

            values = []

            def add(v):
                for k, w in enumerate(values):   # the SAME tensor in two terms reads one column
                    if w is v and _is_tensor(v):
                        return k
                values.append(v)
                return len(values) - 1

            if self._uses_algebra():   # products / derivatives / a convolution: leaf records + operation records
                ctx = _ExprBuilder(add)
                self._emit(ctx)
                program = ops.TermExpr(ctx.records, ctx.operations, len(values))
            else:
                program = ops.TermProgram(self._records(add), len(values))
            cached = self.__dict__["_program"] = (program, values)
        return cached

    def _uses_algebra(self):
        """Does the kernel contain a TermProduct / TermDiff / TermConvolution (then its program is an ops.TermExpr)?"""
        return False

    def _emit(self, ctx):
        """Post-order walk for ops.TermExpr: emits this term's records / operations, returns the operand that names its
        coefficient list (a leaf register range, or the index of the operation that produced it)."""
        return ctx.leaf(self._records(ctx.add))

    @property
    def program(self):
        """The flattened kernel (ops.TermProgram; ops.TermExpr when it uses products, derivatives or a convolution), built once."""
        return self._build_program()[0]

    def parameter_matrix(self, B=None):
        """The parameters as ONE float64 device matrix, columns in program order: (NP,) when every parameter is shared
        (a float or a 0-d tensor), else (B, NP).  Formed by torch on the device, so gradients w.r.t. P reach the tensors.
        (Floats / numpy arrays given next to tensors are uploaded on every call; give tensors to keep the host out of it.)"""
        import torch

        _, values = self._build_program()
        device = next(v.device for v in values if _is_tensor(v))
        cols = []
        for v in values:
            if not _is_tensor(v):
                v = torch.as_tensor(np.asarray(v, dtype=np.float64), device=device)
            if v.dtype != torch.float64 or v.dim() > 1:
                raise ValueError("term parameters must be float64 tensors, 0-d or (B,)")
            cols.append(v.reshape(()) if v.numel() == 1 else v)
        nb = {int(v.shape[0]) for v in cols if v.dim() == 1}
        if len(nb) > 1 or (nb and B is not None and nb != {B}):
            raise ValueError("per-series parameters disagree on the batch size: %s" % sorted(nb | ({B} if B else set())))
        if not nb:
            return torch.stack(cols)
        n = nb.pop()
        return torch.stack([v.expand(n) for v in cols], dim=1)

    def coefficients(self, B):
        """(ar, cr, ac, bc, cc, dc), (B, Jr) / (B, Jc) device tensors by c2_term_coefficients, differentiable.  A series on
        the wrong side of an SHO regime raises nothing here (no read-back): autograd.log_likelihood_kernel gives it -inf."""
        from . import autograd

        return autograd.term_coefficients(self.program, self.parameter_matrix(B), B)

    def _device_coefs(self, B):
        """Detached device coefficients + the interleaved c of terms.py:171-173, for the matrix-level paths."""
        import torch

        co = [v.detach() for v in self.coefficients(B)]
        c = torch.cat([co[1], co[4].repeat_interleave(2, dim=-1)], dim=-1)
        return co, c

    def get_psd(self, omega):
        """Power spectral density at the angular frequencies `omega` (terms.py:81-104).  Floats / numpy parameters: numpy,
        shape of omega (shared coefficients) or (B, M).  Tensor parameters: torch on the device from coefficients(B),
        (B, M) for omega (M,) with B the batch size of the parameters (1 when all are shared)."""
        if self._has_tensors():
            import torch

            P = self.parameter_matrix()
            co = self._device_coefs(P.shape[0] if P.dim() == 2 else 1)[0]
            w2 = torch.as_tensor(omega, dtype=torch.float64, device=P.device).reshape(1, -1) ** 2
            return _psd(co, w2, lambda v, j: v[:, j, None])
        co = self.get_coefficients()
        w2 = np.atleast_1d(np.asarray(omega, dtype=np.float64)) ** 2
        if any(v.ndim == 2 for v in co):
            nb = max(v.shape[0] for v in co if v.ndim == 2)
            co = [np.broadcast_to(v, (nb, v.shape[-1])) for v in co]
            return _psd(co, w2.reshape(1, -1), lambda v, j: v[:, j, None])
        return _psd(co, w2, lambda v, j: float(v[j]))

    def _k0_shift(self, B, device):
        """What k(0) has beyond sum ar + sum ac: nothing, except under a TermConvolution."""
        return 0.0

    def _shifted(self, diag):
        """diag plus the kernel's own diagonal shift (TermConvolution only)."""
        return diag

    def get_value(self, tau):
        """k(tau) (terms.py:58-79), numpy, for dense cross-checks; shared coefficients only."""
        ar, cr, ac, bc, cc, dc = self.get_coefficients()
        tau = np.abs(np.asarray(tau, dtype=np.float64))[..., None]
        k = np.sum(ar * np.exp(-cr * tau), axis=-1)
        return k + np.sum(np.exp(-cc * tau) * (ac * np.cos(dc * tau) + bc * np.sin(dc * tau)), axis=-1)

    def _dev_coefs(self, device, nb=None):
        """The six coefficient arrays (+ the interleaved c of terms.py:171-173 as a seventh) as device tensors, ONE upload,
        cached on the term while the coefficient VALUES stay what they were (parameters are plain attributes a caller may
        change): a pageable host-to-device copy is a synchronisation, and predict() used to make ten of them per call.
        Per-series coefficients keep their (B, .) shape; with any of them per-series the shared ones are broadcast to
        (nb or their own B, .).  Returns (tensors, batched)."""
        import torch

        coefs = [np.asarray(v, dtype=np.float64) for v in self.get_coefficients()]
        batched = any(v.ndim == 2 for v in coefs)
        if batched:
            B = max([v.shape[0] for v in coefs if v.ndim == 2] + [nb or 0])
            coefs = [np.broadcast_to(v, (B, v.shape[-1])) if v.ndim == 1 else v for v in coefs]
        ar, cr, ac, bc, cc, dc = coefs
        Jr, Jc = ar.shape[-1], ac.shape[-1]
        c = np.empty(cr.shape[:-1] + (Jr + 2 * Jc,))
        c[..., :Jr] = cr       # c = [cr, cc0, cc0, cc1, cc1, ...]  (terms.py:171-173)
        c[..., Jr::2] = cc
        c[..., Jr + 1::2] = cc
        host = [np.ascontiguousarray(v) for v in coefs + [c]]
        key = (str(device), batched)
        cache = self.__dict__.get("_dev_cache")
        if cache is not None and cache[0] == key and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(cache[1], host)):
            return cache[2], batched
        flat = torch.from_numpy(np.concatenate([h.ravel() for h in host] + [np.zeros(1)])).to(device)
        out, at = [], 0
        for h in host:
            out.append(flat[at:at + h.size].view(h.shape))
            at += h.size
        self.__dict__["_dev_cache"] = (key, host, out)
        return out, batched

    def get_value_device(self, tau):
        """k(tau) (terms.py:58-79) on the device: `tau` a float64 tensor whose LEADING axis is the batch (B, ...);
        coefficients shared by the batch or one row per series.  What the conditional distribution needs for its
        cross-covariances `KxsT`, `k(0)` and `k(xs - xs')` (core.py:57-66, 134-150)."""
        import torch

        if self._has_tensors():
            batched = True
            ar, cr, ac, bc, cc, dc = self._device_coefs(tau.shape[0])[0]
        else:
            host = self.get_coefficients()
            batched = any(np.ndim(v) == 2 for v in host)
            (ar, cr, ac, bc, cc, dc) = self._dev_coefs(tau.device, tau.shape[0])[0][:6] if batched else host
        tau = tau.abs()
        extra = (1,) * (tau.dim() - 1)

        def co(v, j):   # coefficient j broadcastable against tau: a python float (shared) or a (B, 1, ..) device view
            if not batched:
                return float(v[j])
            return v[:, j].reshape((-1,) + extra)

        k = torch.zeros_like(tau)
        for j in range(ar.shape[-1]):
            k = k + co(ar, j) * torch.exp(-co(cr, j) * tau)
        for j in range(ac.shape[-1]):
            arg = co(dc, j) * tau
            k = k + torch.exp(-co(cc, j) * tau) * (co(ac, j) * torch.cos(arg) + co(bc, j) * torch.sin(arg))
        return k

    def get_value_grid(self, t1, t2, B=None):
        """k(t1[n] - t2[m]) on two grids, (B, N, M), by the c2_kernel_values kernel (ops.kernel_values): what the
        conditional distribution needs for KxsT and for the prior covariance of the prediction grid (core.py:46-54, 142-148)."""
        import torch

        from . import ops

        if self._has_tensors():
            nb = B if B is not None else max(t.shape[0] if t.dim() == 2 else 1 for t in (t1, t2))
            return ops.kernel_values(*self._device_coefs(nb)[0], t1.contiguous(), t2.contiguous(), B=nb)
        dev, _ = self._dev_coefs(t1.device, B)
        return ops.kernel_values(*dev[:6], t1.contiguous(), t2.contiguous(), B=B)

    def get_celerite_matrices(self, x, diag):
        """x (N,)|(B,N), diag (B,N) torch float64 device tensors -> (c, a, U, V) device tensors."""
        import torch

        from . import ops

        if self._has_tensors():
            (ar, cr, ac, bc, cc, dc), c = self._device_coefs(diag.shape[0])
        else:
            (ar, cr, ac, bc, cc, dc, c), _ = self._dev_coefs(diag.device, diag.shape[0])
        a, U, V = ops.get_celerite_matrices(ar, ac, bc, dc, x, self._shifted(diag))
        return c, a, U, V


def _psd(co, w2, cof):
    """terms.py:88-104 on numpy arrays or torch tensors; cof(v, j) = coefficient j, broadcastable against w2."""
    ar, cr, ac, bc, cc, dc = co
    psd = 0.0 * w2
    for j in range(ar.shape[-1]):
        a, c = cof(ar, j), cof(cr, j)
        psd = psd + a * c / (c * c + w2)
    for j in range(ac.shape[-1]):
        a, b, c, d = cof(ac, j), cof(bc, j), cof(cc, j), cof(dc, j)
        w02 = c * c + d * d
        psd = psd + ((a * c + b * d) * w02 + (a * c - b * d) * w2) / (w2 * w2 + 2.0 * (c * c - d * d) * w2 + w02 * w02)
    return math.sqrt(2.0 / math.pi) * psd


class _ExprBuilder:
    """Collects the leaf records and the operation records of an ops.TermExpr while a kernel is walked in post-order."""

    def __init__(self, add):
        self.add, self.records, self.operations, self.jr, self.jc = add, [], [], 0, 0

    def leaf(self, records):
        from . import ops

        r0, c0 = self.jr, self.jc
        for r in records:
            wr, wc = ops.record_widths(r)
            self.jr += wr
            self.jc += wc
        self.records += records
        return (r0, self.jr - r0, c0, self.jc - c0)

    def op(self, name, a, b=None, col=None):
        self.operations.append(dict(op=name, a=a, b=b, col=col))
        return len(self.operations) - 1


def _same_batch(*coefs):
    """Coefficient tuples of several terms, every array broadcast to (nb, J) when any of them is per-series."""
    nb = max(v.shape[0] if v.ndim == 2 else 0 for co in coefs for v in co)
    if not nb:
        return coefs
    return tuple(tuple(np.broadcast_to(v, (nb, v.shape[-1])) if v.ndim == 1 else v for v in co) for co in coefs)


class TermSum(Term):
    def __init__(self, *terms):
        if any(isinstance(t, TermConvolution) for t in terms):
            raise TypeError(_CONV_OUTER)
        self.terms = []
        for t in terms:
            self.terms += t.terms if isinstance(t, TermSum) and t.terms else [t]

    def _has_tensors(self):
        return any(t._has_tensors() for t in self.terms)

    def _records(self, add):
        return [r for t in self.terms for r in t._records(add)]

    def _uses_algebra(self):
        return any(t._uses_algebra() for t in self.terms)

    def _emit(self, ctx):
        if not self._uses_algebra():
            return ctx.leaf(self._records(ctx.add))
        acc, run = [None], []   # runs of plain terms become one leaf list; coefficient order = term order (terms.py:233-235)

        def join(h):
            acc[0] = h if acc[0] is None else ctx.op("sum", acc[0], h)

        for t in self.terms + [None]:
            if t is not None and not t._uses_algebra():
                run.append(t)
                continue
            if run:
                join(ctx.leaf([r for u in run for r in u._records(ctx.add)]))
                run = []
            if t is not None:
                join(t._emit(ctx))
        return acc[0]

    def get_coefficients(self):
        self._no_host()
        parts = [t.get_coefficients() for t in self.terms]
        nb = max(max(v.shape[0] if v.ndim == 2 else 0 for v in p) for p in parts)

        def cat(i):
            arrs = [p[i] for p in parts]
            if nb:
                arrs = [np.broadcast_to(v, (nb, v.shape[-1])) if v.ndim == 1 else v for v in arrs]
            return np.concatenate(arrs, axis=-1)

        return tuple(cat(i) for i in range(6))


class TermProduct(Term):
    """k = k1 k2 (terms.py:238-301): again a celerite kernel, wider.  Coefficients in the reference's order: reals =
    product(reals1, reals2); complex = real1 x complex2, then real2 x complex1, then per complex pair the (dj - dk) term
    followed by the (dj + dk) term."""

    def __init__(self, term1, term2):
        if isinstance(term1, TermConvolution) or isinstance(term2, TermConvolution):
            raise TypeError(_CONV_OUTER)
        self.term1, self.term2 = term1, term2

    def _has_tensors(self):
        return self.term1._has_tensors() or self.term2._has_tensors()

    def _uses_algebra(self):
        return True

    def _emit(self, ctx):
        a = self.term1._emit(ctx)
        b = self.term2._emit(ctx)
        return ctx.op("product", a, b)

    def get_coefficients(self):
        self._no_host()
        c1, c2 = _same_batch(self.term1.get_coefficients(), self.term2.get_coefficients())
        lead = c1[0].shape[:-1]
        R, C = [[], []], [[], [], [], []]
        for j in range(c1[0].shape[-1]):
            for k in range(c2[0].shape[-1]):
                R[0].append(c1[0][..., j] * c2[0][..., k])
                R[1].append(c1[1][..., j] + c2[1][..., k])
        for x, y in ((c1, c2), (c2, c1)):   # real x complex
            for j in range(x[0].shape[-1]):
                for k in range(y[2].shape[-1]):
                    C[0].append(x[0][..., j] * y[2][..., k])
                    C[1].append(x[0][..., j] * y[3][..., k])
                    C[2].append(x[1][..., j] + y[4][..., k])
                    C[3].append(y[5][..., k] + 0.0 * x[0][..., j])
        for j in range(c1[2].shape[-1]):
            aj, bj, cj, dj = (c1[i][..., j] for i in range(2, 6))
            for k in range(c2[2].shape[-1]):
                ak, bk, ck, dk = (c2[i][..., k] for i in range(2, 6))
                C[0] += [0.5 * (aj * ak + bj * bk), 0.5 * (aj * ak - bj * bk)]
                C[1] += [0.5 * (bj * ak - aj * bk), 0.5 * (bj * ak + aj * bk)]
                C[2] += [cj + ck, cj + ck]
                C[3] += [dj - dk, dj + dk]
        st = lambda v: np.stack(v, axis=-1) if v else np.empty(lead + (0,))
        return tuple(st(v) for v in R + C)


class TermDiff(Term):
    """The covariance of the derivative process, -k'' (terms.py:304-330): ar <- -ar cr^2, (a, b) <- (a (d^2 - c^2) + 2 b c d,
    b (d^2 - c^2) - 2 a c d); rates unchanged.  (Not every kernel has a derivative process: TermDiff(RealTerm) is not a
    valid covariance.)"""

    def __init__(self, term):
        if isinstance(term, TermConvolution):
            raise TypeError(_CONV_OUTER)
        self.term = term

    def _has_tensors(self):
        return self.term._has_tensors()

    def _uses_algebra(self):
        return True

    def _emit(self, ctx):
        return ctx.op("diff", self.term._emit(ctx))

    def get_coefficients(self):
        self._no_host()
        ar, cr, a, b, c, d = self.term.get_coefficients()
        q = (d - c) * (d + c)   # d^2 - c^2 without the cancellation of two rounded squares
        return (-ar * cr**2, cr, a * q + 2 * b * c * d, b * q - 2 * a * c * d, c, d)


_CONV_SERIES = 9


def _conv_FG(z):
    """F(z) = 2 (cosh z - 1) / z^2 and G(z) = 2 (z - sinh z) / z^2 at complex z.  The closed forms lose 2 / |z|^2 in
    relative accuracy at small z (an exposure time is short against the kernel's time scales), so below |z| = 1/2 the power
    series are summed -- the same split as the device kernel (csrc/c2_term_expr.hip, conv_fg)."""
    z = np.asarray(z, dtype=np.complex128)
    w = z * z
    f = g = np.zeros_like(z)
    for k in range(_CONV_SERIES - 1, -1, -1):
        f = f * w + 2.0 / math.factorial(2 * k + 2)
        g = g * w - 2.0 / math.factorial(2 * k + 3)
    with np.errstate(all="ignore"):
        F = 2.0 * (np.cosh(z) - 1.0) / w
        G = 2.0 * (z - np.sinh(z)) / w
    small = np.abs(z) ** 2 < 0.25
    return np.where(small, f, F), np.where(small, z * g, G)


def _conv_value(xp, coefs, cof, dt, tau):
    """The boxcar-convolved kernel at lags tau (terms.py:421-482), piecewise in |tau| < dt, on numpy arrays (xp = numpy) or
    torch tensors (xp = torch).  coefs: the INNER term's coefficients; cof(v, j): coefficient j, a float or broadcastable
    against tau; dt likewise."""
    ar, cr, ac, bc, cc, dc = coefs

    def fn(name, v):
        return getattr(math, name)(v) if isinstance(v, float) else getattr(xp, name)(v)

    tau = abs(tau)
    dpt, dmt = dt + tau, dt - tau
    large, small = 0.0 * tau, 0.0 * tau
    for j in range(ar.shape[-1]):
        a, c = cof(ar, j), cof(cr, j)
        crd = c * dt
        norm = 2.0 * a / (crd * crd)
        big = norm * (fn("cosh", crd) - 1.0) * xp.exp(-c * tau)
        x = c * dmt
        large = large + big
        small = small + big + norm * (x - xp.sinh(x))
    for j in range(ac.shape[-1]):
        a, b, c, d = cof(ac, j), cof(bc, j), cof(cc, j), cof(dc, j)
        cd, dd, c2, d2 = c * dt, d * dt, c * c, d * d
        n = c2 + d2
        C1 = a * (c2 - d2) + 2.0 * b * c * d
        C2 = b * (c2 - d2) - 2.0 * a * c * d
        norm = 1.0 / ((dt * n) * (dt * n))
        k0, cdt, sdt = xp.exp(-c * tau), xp.cos(d * tau), xp.sin(d * tau)
        ct = 2.0 * (fn("cosh", cd) * fn("cos", dd) - 1.0)
        st = 2.0 * (fn("sinh", cd) * fn("sin", dd))
        large = large + ((C1 * ct - C2 * st) * cdt + (C2 * ct + C1 * st) * sdt) * (k0 * norm)
        edmt, edpt = xp.exp(-c * dmt), xp.exp(-c * dpt)
        ct = edmt * xp.cos(d * dmt) + edpt * xp.cos(d * dpt) - 2.0 * k0 * cdt
        st = edmt * xp.sin(d * dmt) + edpt * xp.sin(d * dpt) - 2.0 * k0 * sdt
        small = small + 2.0 * (a * c + b * d) * n * dmt * norm + (C1 * ct + C2 * st) * norm
    return xp.where(tau >= dt, large, small)


class TermConvolution(Term):
    """The kernel integrated over a boxcar of width `delta`, e.g. an exposure time (terms.py:333-482): new amplitudes, and a
    diagonal shift `delta_diag` that get_celerite_matrices adds to diag; get_value is piecewise for |tau| < delta.  It must be
    the OUTERMOST term.  `delta` is data, not a hyper-parameter: a float, a numpy (B,) array (one exposure time per series) or
    a tensor that does not require grad.

    The semiseparable form (compute / log_likelihood / the conditional MEAN at new times, core.py:68-113) is exact for lags
    >= delta, as in the reference: observations closer than delta to each other, or predictions closer than delta to an
    observation, see the tail formula instead of the piecewise one.  The conditional variance / covariance use get_value_grid
    and are piecewise-exact."""

    def __init__(self, term, delta):
        if isinstance(term, TermConvolution):
            raise TypeError(_CONV_OUTER)
        if _is_tensor(delta):
            if delta.requires_grad:
                raise TypeError("TermConvolution: delta is data, not a hyper-parameter (it must not require grad)")
        elif np.ndim(delta) == 0:
            delta = float(delta)
        else:
            delta = np.asarray(delta, dtype=np.float64).reshape(-1)
        self.term, self.delta = term, delta

    def _has_tensors(self):
        return self.term._has_tensors() or _is_tensor(self.delta)

    def _uses_algebra(self):
        return True

    def _emit(self, ctx):
        h = self.term._emit(ctx)
        return ctx.op("convolve", h, col=ctx.add(self.delta))

    def _dt_host(self):
        return self.delta if isinstance(self.delta, float) else self.delta[:, None]

    def _convolved(self):
        """(coefficients, delta_diag) on the host: (a - i b) <- (a - i b) F(z) and delta_diag = sum Re (a - i b) G(z) with
        z = (c - i d) delta (d = b = 0 for the real terms) -- the reference's terms.py:350-410 in complex arithmetic."""
        ar, cr, a, b, c, d = self.term.get_coefficients()
        dt = self._dt_host()
        Fr, Gr = _conv_FG(cr * dt + 0j)
        Fc, Gc = _conv_FG((c - 1j * d) * dt)
        w = (a - 1j * b) * Fc
        shift = np.sum(ar * Gr.real, axis=-1, keepdims=True) + np.sum(((a - 1j * b) * Gc).real, axis=-1, keepdims=True)
        one = np.ones_like(w.real)
        return (ar * Fr.real, cr * np.ones_like(Fr.real), w.real, -w.imag, c * one, d * one), shift

    def get_coefficients(self):
        self._no_host()
        return self._convolved()[0]

    def get_delta_diag(self):
        """delta_diag (terms.py:353-378), host parameters: a float, or (B, 1) with per-series coefficients / delta."""
        self._no_host()
        out = self._convolved()[1]
        return float(out[0]) if out.ndim == 1 else out

    def _shift_device(self, B, device):
        """delta_diag as a float (shared host parameters) or a (B, 1) device tensor."""
        import torch

        if self._has_tensors():
            from . import autograd

            return autograd.term_coefficients(self.program, self.parameter_matrix(B), B, with_shift=True)[6].detach()[:, None]
        s = self.get_delta_diag()
        return s if isinstance(s, float) else torch.from_numpy(np.ascontiguousarray(s)).to(device)

    def _k0_shift(self, B, device):
        return self._shift_device(B, device)

    def _shifted(self, diag):
        return (diag + self._shift_device(diag.shape[0], diag.device)).contiguous()

    def get_psd(self, omega):
        """The inner term's spectrum times sinc^2(delta omega / 2) (terms.py:412-419)."""
        psd0 = self.term.get_psd(omega) if not (_is_tensor(self.delta) and not self.term._has_tensors()) else None
        if _is_tensor(psd0) or psd0 is None:
            import torch

            dev = self.delta.device if psd0 is None else psd0.device
            if psd0 is None:
                psd0 = torch.as_tensor(np.atleast_2d(self.term.get_psd(omega)), device=dev)
            w = torch.as_tensor(omega, dtype=torch.float64, device=dev).reshape(1, -1)
            dt = self.delta if _is_tensor(self.delta) else torch.as_tensor(self.delta, dtype=torch.float64, device=dev)
            arg = 0.5 * dt.reshape(-1, 1) * w
            return psd0 * torch.sinc(arg / math.pi) ** 2
        w = np.atleast_1d(np.asarray(omega, dtype=np.float64))
        arg = 0.5 * self._dt_host() * (w if psd0.ndim == 1 else w.reshape(1, -1))
        return psd0 * np.sinc(arg / np.pi) ** 2

    def get_value(self, tau):
        """The piecewise convolved kernel (terms.py:421-482), numpy; shared coefficients and a float delta only."""
        self._no_host()
        co = self.term.get_coefficients()
        if any(v.ndim == 2 for v in co) or not isinstance(self.delta, float):
            raise ValueError("TermConvolution.get_value: shared coefficients only (use get_value_device for a batch)")
        return _conv_value(np, co, lambda v, j: float(v[j]), self.delta, np.atleast_1d(np.asarray(tau, dtype=np.float64)))

    def get_value_device(self, tau):
        """The piecewise convolved kernel on the device (a torch expression on the lag tensor: the O(N M) prediction path)."""
        import torch

        B, extra = tau.shape[0], (1,) * (tau.dim() - 1)
        inner = self.term
        if inner._has_tensors():
            co, batched = inner._device_coefs(B)[0], True
        else:
            co = inner.get_coefficients()
            batched = any(v.ndim == 2 for v in co)
            if batched:
                co = inner._dev_coefs(tau.device, B)[0][:6]
        cof = (lambda v, j: v[:, j].reshape((-1,) + extra)) if batched else (lambda v, j: float(v[j]))
        dt = self.delta
        if not isinstance(dt, float):
            dt = dt.detach().to(tau.device) if _is_tensor(dt) else torch.from_numpy(dt).to(tau.device)
            dt = dt.reshape((-1,) + extra) if dt.numel() > 1 else dt.reshape(())
        return _conv_value(torch, co, cof, dt, tau)

    def get_value_grid(self, t1, t2, B=None):
        """k(t1[n] - t2[m]), (B, N, M), piecewise for |lag| < delta: get_value_device on the lag tensor."""
        nb = B if B is not None else max(t.shape[0] if t.dim() == 2 else 1 for t in (t1, t2))
        a = t1 if t1.dim() == 2 else t1[None].expand(nb, -1)
        b = t2 if t2.dim() == 2 else t2[None].expand(nb, -1)
        return self.get_value_device(a[:, :, None] - b[:, None, :]).contiguous()


def _stack(*cols):
    cols = [_col(v) for v in cols]
    n = max(v.shape[0] for v in cols)
    if n == 1:
        return np.array([float(v[0]) for v in cols])
    return np.stack([np.broadcast_to(v, (n,)) for v in cols], axis=1)


_E = np.empty(0)


def _empty_like(v):
    return np.empty(v.shape[:-1] + (0,))


class RealTerm(Term):
    """k(tau) = a exp(-c tau)  (terms.py:515-521)."""

    def __init__(self, *, a, c):
        self.a, self.c = a, c

    def _records(self, add):
        return [dict(kind="real", cols=(add(self.a), add(self.c)))]

    def get_coefficients(self):
        self._no_host()
        ar, cr = _stack(self.a), _stack(self.c)
        e = _empty_like(ar)
        return ar, cr, e, e, e, e


class ComplexTerm(Term):
    """k(tau) = exp(-c tau) (a cos(d tau) + b sin(d tau))  (terms.py:554-569)."""

    def __init__(self, *, a, b, c, d):
        self.a, self.b, self.c, self.d = a, b, c, d

    def _records(self, add):
        return [dict(kind="complex", cols=(add(self.a), add(self.b), add(self.c), add(self.d)))]

    def get_coefficients(self):
        self._no_host()
        ac, bc, cc, dc = _stack(self.a), _stack(self.b), _stack(self.c), _stack(self.d)
        e = _empty_like(ac)
        return e, e, ac, bc, cc, dc


class SHOTerm(Term):
    """Stochastically driven damped harmonic oscillator (terms.py:641-691).  With floats / numpy arrays Q is ONE number
    (the over/under-damped branch is chosen once on the host); S0 and w0 may be per-series arrays.

    With tensor parameters (any of S0 | sigma, w0 | rho, Q | tau a device tensor) the parameters stay as given -- the
    alternative parameterisations are resolved on the device, forward and reverse -- and `regime` says how the branch is
    taken, so that nothing is read back: "under" / "over": the whole batch is on that side of Q = 1/2 (one complex term /
    two real terms; a series on the wrong side gets ll = -inf and zero gradients from autograd.log_likelihood_kernel);
    "mixed": each series takes the side ITS Q selects, as the reference's jax term does (jax/terms.py:481-548).  Mixed
    costs width 4 instead of 2: the term occupies two real AND one complex slot, the unused side with zero amplitudes.
    `regime` is required when Q (or the w0 | rho and tau it derives from) is a tensor; with a float Q it defaults to the
    side of that Q."""

    def __init__(self, *, S0=None, w0=None, Q=None, sigma=None, rho=None, tau=None, eps=1e-5, regime=None):
        if regime not in (None, "under", "over", "mixed"):
            raise ValueError("SHOTerm: regime must be 'under', 'over' or 'mixed'")
        self.regime = regime
        if any(_is_tensor(v) for v in (S0, w0, Q, sigma, rho, tau)):
            if (S0 is None) == (sigma is None) or (w0 is None) == (rho is None) or (Q is None) == (tau is None):
                raise ValueError("SHOTerm: give exactly one of S0 | sigma, of w0 | rho and of Q | tau")
            self._given = (sigma if S0 is None else S0, rho if w0 is None else w0, tau if Q is None else Q)
            self._par = (1 if S0 is None else 0) | (2 if w0 is None else 0) | (4 if Q is None else 0)
            self.eps = float(eps)
            if regime is None:
                qsrc = (Q,) if tau is None else (tau, self._given[1])
                if any(_is_tensor(v) for v in qsrc) or np.size(qsrc[0]) != 1 or np.size(qsrc[-1]) != 1:
                    raise ValueError("SHOTerm: Q is a tensor (or derives from one): say regime='under', 'over' or 'mixed'")
                w = float(2 * np.pi / rho) if w0 is None else float(w0)
                q = float(Q) if tau is None else 0.5 * w * float(tau)
                self.regime = "over" if q < 0.5 else "under"
            return
        if w0 is None:
            w0 = 2 * np.pi / _col(rho)
        if Q is None:
            Q = 0.5 * np.asarray(w0, dtype=np.float64) * tau
        # One over/under-damped branch serves the whole batch, so Q must be ONE number: a per-series Q (given, or
        # derived from a per-series rho / w0 and tau) would be truncated silently -- refuse it instead.
        Qv = np.unique(np.ravel(np.asarray(Q, dtype=np.float64)))
        if Qv.size != 1:
            raise ValueError("SHOTerm: Q must be a scalar shared by the batch (got %d distinct values); "
                             "pass a scalar Q, or scalar rho/w0 together with tau" % Qv.size)
        Q = float(Qv[0])
        if S0 is None:
            S0 = _col(sigma) ** 2 / (_col(w0) * Q)  # the same Q that is stored and used below
        self.S0, self.w0, self.Q, self.eps = S0, w0, Q, float(eps)

    def _records(self, add):
        if "_given" in self.__dict__:
            return [dict(kind="sho", cols=tuple(add(v) for v in self._given), par=self._par, regime=self.regime, eps=self.eps)]
        # float parameters next to tensor terms in one sum: (S0, w0, Q) as stored, the side of the float Q
        regime = self.regime or ("over" if self.Q < 0.5 else "under")
        return [dict(kind="sho", cols=(add(self.S0), add(self.w0), add(self.Q)), par=0, regime=regime, eps=self.eps)]

    def get_coefficients(self):
        self._no_host()
        S0, w0, Q = _col(self.S0), _col(self.w0), self.Q
        if Q < 0.5:
            f = np.sqrt(max(1.0 - 4.0 * Q**2, self.eps))
            ar = _stack(0.5 * S0 * w0 * Q * (1.0 + 1.0 / f), 0.5 * S0 * w0 * Q * (1.0 - 1.0 / f))
            cr = _stack(0.5 * w0 / Q * (1.0 - f), 0.5 * w0 / Q * (1.0 + f))
            e = _empty_like(ar)
            return ar, cr, e, e, e, e
        f = np.sqrt(max(4.0 * Q**2 - 1.0, self.eps))
        a = S0 * w0 * Q
        c = 0.5 * w0 / Q
        ac, bc, cc, dc = _stack(a), _stack(a / f), _stack(c), _stack(c * f)
        e = _empty_like(ac)
        return e, e, ac, bc, cc, dc


class Matern32Term(Term):
    """Approximate Matern-3/2 (terms.py:729-745)."""

    def __init__(self, *, sigma, rho, eps=0.01):
        self.sigma, self.rho, self.eps = sigma, rho, float(eps)

    def _records(self, add):
        return [dict(kind="matern32", cols=(add(self.sigma), add(self.rho)), eps=self.eps)]

    def get_coefficients(self):
        self._no_host()
        w0 = np.sqrt(3.0) / _col(self.rho)
        S0 = _col(self.sigma) ** 2 / w0
        ac, bc, cc, dc = _stack(w0 * S0), _stack(w0 * w0 * S0 / self.eps), _stack(w0), _stack(np.full_like(w0, self.eps))
        e = _empty_like(ac)
        return e, e, ac, bc, cc, dc


class RotationTerm(TermSum):
    """Mixture of two SHO terms at period and period/2 (terms.py:791-812)."""

    def __init__(self, *, sigma, period, Q0, dQ, f):
        if any(_is_tensor(v) for v in (sigma, period, Q0, dQ, f)):
            # one record of its own kind: the two oscillators share their five parameters (Q0, dQ > 0: both under-damped)
            self._given = (sigma, period, Q0, dQ, f)
            self.terms = []
            return
        amp = float(sigma) ** 2 / (1 + float(f))
        Q1 = 0.5 + Q0 + dQ
        w1 = 4 * np.pi * Q1 / (period * np.sqrt(4 * Q1**2 - 1))
        S1 = amp / (w1 * Q1)
        Q2 = 0.5 + Q0
        w2 = 8 * np.pi * Q2 / (period * np.sqrt(4 * Q2**2 - 1))
        S2 = f * amp / (w2 * Q2)
        super().__init__(SHOTerm(S0=S1, w0=w1, Q=Q1), SHOTerm(S0=S2, w0=w2, Q=Q2))

    def _has_tensors(self):
        return "_given" in self.__dict__ or super()._has_tensors()

    def _records(self, add):
        if "_given" in self.__dict__:
            return [dict(kind="rotation", cols=tuple(add(v) for v in self._given), eps=1e-5)]
        return super()._records(add)
