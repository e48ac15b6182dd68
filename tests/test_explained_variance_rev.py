# -*- coding: utf-8 -*-
"""The reverse of the explained variance at new times on the CPU: the numpy restatement (tests/explained_variance_rev_ref.py,
what csrc/c2_predvar.hip's workspace form and csrc/c2_predvar_rev.hip implement) against complex-step derivatives of the
forward, against the dense closed form under torch autograd through `factor`, the kernels' event loops against the per-row
form, the margin float64 has against long double, and the C-ABI's argument checks, which need no device."""
import ctypes

import numpy as np
import pytest
import torch

import explained_variance_rev_ref as R
import predict_at_ref as P
from general_rev_ref import close

SHAPES = [(1, 1, 4), (2, 3, 9), (17, 8, 12), (33, 5, 40), (6, 32, 11)]      # (N, J, M)
NAMES = ("bt", "bts", "bc", "bU", "bW", "bd", "bUs", "bVs")


def case(seed, N, J, M, kind):
    """One series: (t, ts, c, U, W, d, Us, Vs) with (d, W) the factors of the draw, the draw's dict, and br."""
    rng = np.random.default_rng(seed + 31)
    t = P.draw(seed, N, J)["t"]
    ts = R.query_grid(kind, t, rng, M)
    D = P.draw_with_queries(seed, N, J, t=t, ts=ts)
    d, W = P.factor(D["t"], D["c"], D["a"], D["U"], D["V"])
    return [D["t"], ts, D["c"], D["U"], W, d, D["Us"], D["Vs"]], D, rng.normal(size=M)


def complex_forward(args):
    """predict_at_ref.explained_variance restated in complex arithmetic (the merge index n(m) from the real parts)."""
    return R.forward_ws(*args)[0]


@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_adjoint_against_complex_step(kind):
    """All eight cotangents against complex-step derivatives of the forward, element by element: 1e-12 of each array's
    largest entry (measured: 1.7e-15).  The grids: predict_at_ref.queries (ties, before the first, after the last, several in
    one gap), every query in front of the data, every query behind it, and ties with repeated queries."""
    h = 1e-30
    worst = 0.0
    for i, (N, J, M) in enumerate(SHAPES):
        args, _, br = case(100 + i, N, J, M, kind)
        r, X, Sws, Rws = R.forward_ws(*args)
        np.testing.assert_allclose(r, P.explained_variance(*args), rtol=1e-13, atol=0)
        got = R.reverse_rows(*args, X, Sws, Rws, br)
        for k, (a, g, nm) in enumerate(zip(args, got, NAMES)):
            num = np.zeros_like(a)
            for idx in np.ndindex(a.shape):
                ac = [x.astype(complex) for x in args]
                ac[k][idx] += 1j * h
                num[idx] = (br @ complex_forward(ac).imag) / h
            scale = float(np.max(np.abs(num)))
            e = float(np.max(np.abs(num - g))) / (scale if scale > 0 else 1.0)
            worst = max(worst, e)
            assert e <= 1e-12, (nm, (N, J, M), kind, e)
        if kind == "front":
            assert not np.any(got[6])                             # bUs: no data row in front of any query
        if kind == "behind":
            assert not np.any(got[7])                             # bVs: no data row above any query
    print("%s: worst complex-step error / largest entry: %.3g" % (kind, worst))


def torch_factor(t, c, a, U, V):
    """inverse_diag_ref.factor in torch (float64, CPU), differentiable: the link between the closed form's (a, V) and the
    sweep's (d, W)."""
    N = U.shape[0]
    S = torch.zeros((U.shape[1],) * 2, dtype=torch.float64)
    d, W = [a[0]], [V[0] / a[0]]
    for n in range(1, N):
        p = torch.exp(-c * (t[n] - t[n - 1]))
        S = torch.outer(p, p) * (S + d[-1] * torch.outer(W[-1], W[-1]))
        tmp = U[n] @ S
        d.append(a[n] - tmp @ U[n])
        W.append((V[n] - tmp) / d[-1])
    return torch.stack(d), torch.stack(W)


@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_chain_against_dense_closed_form(kind):
    """factor -> explained_variance against k0 - diag(K*^T (K + D)^-1 K*) under torch float64 autograd (masks and signed lags:
    explained_variance_rev_ref.dense_variance): the value and the derivative with respect to t, ts, c, a, U, V, Us, Vs at
    the standing criterion, per array.  The sweep's reverse is the restatement; factor's is torch autograd of its recurrence."""
    worst = 0.0
    for i, (N, J, M) in enumerate(SHAPES + [(5, 2, 1)]):
        args, D, bvar = case(200 + i, N, J, M, kind)
        t, ts, c, U, W, d, Us, Vs = args
        r, X, Sws, Rws = R.forward_ws(*args)
        bt, bts, bc, bU, bW, bd, bUs, bVs = R.reverse_rows(*args, X, Sws, Rws, -bvar)      # var = k0 - r
        tt = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (t, c, D["a"], U, D["V"])]
        dT, WT = torch_factor(*tt)
        close(dT.detach().numpy(), d, "d"); close(WT.detach().numpy(), W, "W")
        ft, fc, fa, fU, fV = torch.autograd.grad((dT, WT), tt, (torch.tensor(bd), torch.tensor(bW)), allow_unused=True)
        z = lambda g, like: np.zeros_like(like) if g is None else g.numpy()
        got = (bt + z(ft, t), bts, bc + z(fc, c), z(fa, t), bU + z(fU, U), z(fV, U), bUs, bVs)
        dd = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (t, ts, c, D["a"], U, D["V"], Us, Vs)]
        var = R.dense_variance(*dd, D["k0"])
        want = torch.autograd.grad(var, dd, torch.tensor(bvar))
        worst = max(worst, close(D["k0"] - r, var.detach().numpy(), "var %s" % ((N, J, M),)))
        for nm, g, w in zip(("bt", "bts", "bc", "ba", "bU", "bV", "bUs", "bVs"), got, want):
            worst = max(worst, close(g, w.numpy(), "%s %s %s" % (nm, kind, (N, J, M))))
    print("%s: worst %.3g of the criterion" % (kind, worst))


EVENT_SHAPES = [(1, 1), (2, 9), (7, 8), (8, 7), (9, 33), (33, 9), (150, 40), (5, 1)]      # (N, M): ring 8, pending 4, unroll 4


@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_event_loops_of_the_kernels(kind):
    """The kernels' event loops restated statement by statement (emulate_forward, emulate_reverse: the merge and its tie rule,
    ring slots, requests eight positions ahead arriving four events later, clamping at the end of a grid, the carried bt, the
    record columns, pass B adding to what pass A wrote) against the per-row form; a slot read before its row arrived, and an
    output element never written, hold NaN."""
    idx = 0
    for N, M in EVENT_SHAPES:
        for J in (1, 3, 8):
            idx += 1
            args, _, br = case(300 + idx, N, J, M, kind)
            want_f = R.forward_ws(*args)
            got_f = R.emulate_forward(*args)
            for nm, g, w in zip(("r", "X", "Sws", "Rws"), got_f, want_f):
                close(g, w, "%s %s %s" % (nm, kind, (N, M, J)))
            want = R.reverse_rows(*args, *want_f[1:], br)
            got = R.emulate_reverse(*args, *want_f[1:], br)
            for nm, g, w in zip(NAMES, got, want):
                close(g, w, "%s %s %s" % (nm, kind, (N, M, J)))
            nq = R.last_rows(args[0], args[1])
            assert not np.any(got[6][nq < 0]) and not np.any(got[7][nq == N - 1])      # exact zeros


@pytest.mark.parametrize("J", [1, 3, 8, 32])
def test_float64_against_long_double(J):
    """The same restatement in long double: every float64 cotangent sits inside the standing criterion -- the margin the
    device's other rounding order has against this restatement (where long double is double the comparison is trivial)."""
    worst = 0.0
    for i, (N, M, kind) in enumerate([(17, 15, "mixed"), (33, 16, "ties"), (150, 40, "mixed"), (150, 40, "behind"), (9, 33, "front")]):
        args, _, br = case(400 + 10 * J + i, N, J, M, kind)
        got = R.reverse_rows(*args, *R.forward_ws(*args)[1:], br)
        lo = [x.astype(np.longdouble) for x in args]
        want = R.reverse_rows(*lo, *R.forward_ws(*lo)[1:], br.astype(np.longdouble))
        for nm, g, w in zip(NAMES, got, want):
            e = close(g, w.astype(np.float64), "%s %s" % (nm, (N, M, kind)))
            worst = max(worst, e)
    print("J=%d worst float64 - long double / criterion: %.3g" % (J, worst))


def test_abi_argument_errors():
    """c2_explained_variance_fwd / _rev reject null pointers and non-positive sizes (C2_ERR_INVALID) and widths above
    C2_FAST_WIDTH (C2_ERR_UNSUPPORTED) before anything touches the device."""
    from celerite2_amd import _lib, build

    build.build_all()
    lib = _lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first
    for name, nptr in (("c2_explained_variance_fwd", 12), ("c2_explained_variance_rev", 20)):
        assert name in _lib.HEADERS["main"].symbols
        fn = getattr(lib, name)

        def call(B, N, M, J, ptrs):
            t, ts, c = ptrs[:3]
            return fn(i64(B), i64(N), i64(M), i64(J), t, i64(0), ts, i64(0), c, i64(0), *ptrs[3:], null)

        ok = [one] * nptr
        assert call(1, 4, 3, 2, [null] * nptr) == _lib.C2_ERR_INVALID
        for bad in ((0, 4, 3, 2), (1, 0, 3, 2), (1, 4, 0, 2), (1, 4, 3, 0)):
            assert call(*bad, ok) == _lib.C2_ERR_INVALID, bad
        for i in range(nptr):   # each pointer in turn
            assert call(1, 4, 3, 2, ok[:i] + [null] + ok[i + 1:]) == _lib.C2_ERR_INVALID, (name, i)
        assert call(1, 4, 3, 33, ok) == _lib.C2_ERR_UNSUPPORTED
        assert call(1, 4, 3, 129, [null] * nptr) == _lib.C2_ERR_UNSUPPORTED
        assert call(1, 2 ** 30, 2 ** 30, 2, ok) == _lib.C2_ERR_UNSUPPORTED      # N + M >= 2^31
