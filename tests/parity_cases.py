# -*- coding: utf-8 -*-
"""Inputs and float64-oracle expectations shared by test_gpu_switch_parity.py and test_gpu_offset_arrays.py (plain
helpers, no tests): the draws are `problem()` / dense.synthetic_batch ones, the comparison rule is that of
test_gpu_ops.py::close -- 1e-10 relative per element with a floor of 1e-12 of the largest entry."""
from types import SimpleNamespace

import numpy as np

from oracle import dense

SWEEPS = ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper")


def dev(*xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def close(a, b, tol=1e-10, floor=1e-12):
    """|a - b| <= tol |b| + floor max(1, max|b|) per element (the rule of tests/test_gpu_ops.py::close)."""
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    np.testing.assert_allclose(a, b, rtol=tol, atol=floor * max(1.0, float(np.abs(b).max())))


class forced:
    """Dispatch options (process-global) set for a block and put back to automatic, whatever happens inside."""

    def __init__(self, opts):
        self.opts = dict(opts or {})

    def __enter__(self):
        from celerite2_amd import _lib
        try:
            for k, v in self.opts.items():
                _lib.set_option(k, v)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        from celerite2_amd import _lib
        for k in self.opts:
            _lib.set_option(k, None)


def problem(rng, B, N, J):
    """A positive-definite batch of width J (columns dropped from an even-width SHO sum, diagonal lifted): the draw of
    tests/test_gpu_fuzz.py::problem."""
    Je = J if J % 2 == 0 else J + 1
    t, c, a, U, V, y = dense.synthetic_batch(B, max(N, 2), Je)
    t = np.ascontiguousarray(t[:, :N]); a = np.ascontiguousarray(a[:, :N]) + 1.0
    U = np.ascontiguousarray(U[:, :N, :J]); V = np.ascontiguousarray(V[:, :N, :J])
    c = np.ascontiguousarray(c[:, :J]); y = np.ascontiguousarray(y[:, :N])
    return t, c, a, U, V, y


def factor_case(oracle, B, N, J, fail=None):
    """problem() and the oracle's d, W, S, flag; `fail` = (series, row): a diagonal entry that makes that series fail."""
    t, c, a, U, V, y = problem(None, B, N, J)
    if fail is not None:
        a[fail[0], fail[1]] = -5.0
    d = np.empty((B, N)); W = np.empty((B, N, J)); S = np.empty((B, N, J, J)); flag = np.empty(B, dtype=np.int64)
    for b in range(B):
        flag[b] = oracle.factor_flag(t[b], c[b], a[b], U[b], V[b], d[b], W[b], S[b])
    return SimpleNamespace(B=B, N=N, J=J, t=t, c=c, a=a, U=U, V=V, y=y, d=d, W=W, S=S, flag=flag, ok=flag == 0)


def check_factor(case, d, W, S, flag):
    """d, W, S of the series that factor and the flags of all of them against the oracle."""
    assert flag.cpu().tolist() == case.flag.tolist()
    ok = case.ok
    close(d[ok], case.d[ok]); close(W[ok], case.W[ok])
    if S is not None:
        close(S[ok], case.S[ok])


def sweep_case(oracle, seed, B, N, J, nrhs, shared_t=False):
    """Inputs of the four sweeps and, from the oracle, per op: Z and F of the *_fwd form and the five reverse outputs for
    the cotangent bZ.  The solves take (0.3 / J) randn as W where the series is short (N <= 40: the recursion cannot
    grow), the W of the oracle's factor beyond."""
    rng = np.random.default_rng(seed)
    t, c, a, U, V, y = problem(rng, B, N, J)
    if shared_t:
        t = np.repeat(t[:1], B, axis=0)
    if N <= 40:
        W = (0.3 / J) * rng.standard_normal((B, N, J))
    else:
        W = np.empty((B, N, J))
        for b in range(B):
            assert oracle.factor_flag(t[b], c[b], a[b], U[b], V[b], np.empty(N), W[b], np.empty((N, J, J))) == 0
    Y = rng.standard_normal((B, N, nrhs)); bZ = rng.standard_normal((B, N, nrhs)); Z0 = rng.standard_normal((B, N, nrhs))
    want = {}
    for name in SWEEPS:
        sec = W if name.startswith("solve") else V
        Zo = np.empty_like(Y); Fo = np.empty((B, N, J, nrhs))
        rev = [np.empty((B, N)), np.empty((B, J)), np.empty((B, N, J)), np.empty((B, N, J)), np.empty((B, N, nrhs))]
        for b in range(B):
            getattr(oracle, name + "_fwd")(t[b], c[b], U[b], sec[b], Y[b], Zo[b], Fo[b])
            getattr(oracle, name + "_rev")(t[b], c[b], U[b], sec[b], Y[b], Zo[b], Fo[b], bZ[b], *[r[b] for r in rev])
        want[name] = SimpleNamespace(Z=Zo, F=Fo, rev=rev)
    return SimpleNamespace(B=B, N=N, J=J, nrhs=nrhs, shared_t=shared_t, t=t, c=c, U=U, V=V, W=W, Y=Y, bZ=bZ, Z0=Z0,
                           want=want)


def second(case, name):
    return case.W if name.startswith("solve") else case.V


def check_reverse(case, name, res):
    """The five reverse outputs, series by series; over a shared grid bt is summed over the batch by the device and per
    series by the oracle, so it is left out there (as tests/test_gpu_fuzz.py does)."""
    got = [r.cpu().numpy() for r in res]
    want = case.want[name].rev
    first = 1 if case.shared_t else 0
    for b in range(case.B):
        for g, w in zip(got[first:], want[first:]):
            close(g[b], w[b])


def sweep_inputs(case, name):
    """Aligned device tensors of one op: t (shared: (N,)), c, U, the second matrix, Y."""
    return dev(case.t[0] if case.shared_t else case.t, case.c, case.U, second(case, name), case.Y)


def check_forward_modes(ops, case, name, with_F=True):
    """One op of a case through the forms the entry point has: with the F workspace, without it, in place (Z is Y) and --
    the products -- accumulating into a Z that holds other numbers (zero_z=False)."""
    import torch
    matmul = name.startswith("matmul")
    w = case.want[name]
    td, cd, Ud, Sd, Yd = sweep_inputs(case, name)
    op = getattr(ops, name)
    kw = dict(zero_z=True) if matmul else {}
    if with_F:
        Z, F = op(td, cd, Ud, Sd, Yd, workspace=True, **kw)
        close(Z, w.Z); close(F, w.F)
    Zn = torch.full_like(Yd, float("nan"))
    close(op(td, cd, Ud, Sd, Yd, Z=Zn, **kw), w.Z)
    Yc = Yd.clone()
    Zi = op(td, cd, Ud, Sd, Yc, Z=Yc)
    assert Zi.data_ptr() == Yc.data_ptr()
    close(Zi, w.Z + case.Y if matmul else w.Z)
    if matmul:
        (Z0d,) = dev(case.Z0)
        close(op(td, cd, Ud, Sd, Yd, Z=Z0d, zero_z=False), w.Z + case.Z0)
        if with_F:
            (Z0d,) = dev(case.Z0)
            Za, Fa = op(td, cd, Ud, Sd, Yd, Z=Z0d, workspace=True, zero_z=False)
            close(Za, w.Z + case.Z0); close(Fa, w.F)


def run_reverse(ops, case, name):
    td, cd, Ud, Sd, Yd = sweep_inputs(case, name)
    Zd, Fd, bZd = dev(case.want[name].Z, case.want[name].F, case.bZ)
    check_reverse(case, name, getattr(ops, name + "_rev")(td, cd, Ud, Sd, Yd, Zd, Fd, bZd))


def general_case(oracle, seed, B, N, M, J, nrhs):
    """general_matmul_lower/upper: a problem() grid t2 of M rows, N sorted output times that start before it and end
    behind it, accumulation into Z0, F prefilled with 3 (rows the merge never visits stay)."""
    rng = np.random.default_rng(seed)
    t2, c, a, U2, V, y = problem(rng, B, M, J)
    lo, hi = t2[:, :1], t2[:, -1:]
    t1 = np.sort(lo - 0.5 + (hi - lo + 1.0) * rng.random((B, N)), axis=1)
    U = rng.standard_normal((B, N, J)); Y = rng.standard_normal((B, M, nrhs)); Z0 = rng.standard_normal((B, N, nrhs))
    want = {}
    for name in ("general_matmul_lower", "general_matmul_upper"):
        Zo = Z0.copy(); Fo = np.full((B, M, J, nrhs), 3.0)
        for b in range(B):
            getattr(oracle, name)(t1[b], t2[b], c[b], U[b], V[b], Y[b], Zo[b], Fo[b])
        want[name] = SimpleNamespace(Z=Zo, F=Fo)
    return SimpleNamespace(B=B, N=N, M=M, J=J, nrhs=nrhs, t1=t1, t2=t2, c=c, U=U, V=V, Y=Y, Z0=Z0, want=want)


def loglik_case(oracle, B, N, J):
    t, c, a, U, V, y = dense.synthetic_batch(B, N, J)
    ll, grads, flag = oracle.loglik_grad_batched(t, c, a, U, V, y, nthreads=2)
    assert not np.asarray(flag).any()
    return SimpleNamespace(B=B, N=N, J=J, t=t, c=c, a=a, U=U, V=V, y=y, ll=ll, grads=grads)
