# -*- coding: utf-8 -*-
"""CPU checks of the reverse of the inverse-diagonal sweep: the numpy restatement of the adjoint recurrence
(tests/inverse_diag_rev_ref.py, what the GPU tests compare the kernel with) against complex-step derivatives of the
restated forward, the dense closed form of the leave-one-out objective's gradient against the restated chain, and the
argument validation of the new entry points.

Criterion everywhere: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element (inverse_diag_ref.err); an
array whose reference is identically zero (bt, bc of a one-row series) must be identically zero."""
import ctypes

import numpy as np
import pytest

import inverse_diag_ref as R
import inverse_diag_rev_ref as RR


def _err(x, xo):
    xo = np.asarray(xo)
    if not np.any(xo):
        return 0.0 if not np.any(x) else np.inf
    return R.err(x, xo)


def _factored(seed, N, J, gap):
    case = R.draw(seed, N, J, gap=gap)
    case["d"], case["W"] = R.factor(case["t"], case["c"], case["a"], case["U"], case["V"])
    case["z"] = R.solve_lower(case["t"], case["c"], case["U"], case["W"], case["y"])
    return case


def test_forward_states_reproduce_the_restated_sweep():
    for J, N in ((1, 1), (2, 3), (5, 17), (8, 40)):
        k = _factored(100 * J + N, N, J, False)
        q, alpha, Mws, Fws = RR.forward_states(k["t"], k["c"], k["U"], k["W"], k["d"], k["z"])
        q0, alpha0 = R.inverse_diag(k["t"], k["c"], k["U"], k["W"], k["d"], z=k["z"])
        assert R.err(q, q0) <= 1.0 and R.err(alpha, alpha0) <= 1.0
        assert not Mws[N - 1].any() and not Fws[N - 1].any()
        assert np.array_equal(Mws, np.swapaxes(Mws, -1, -2)) or R.err(Mws, np.swapaxes(Mws, -1, -2)) <= 1.0
        q1, a1, M1, F1 = RR.forward_states(k["t"], k["c"], k["U"], k["W"], k["d"])
        assert a1 is None and F1 is None and np.array_equal(q1, q) and np.array_equal(M1, Mws)


@pytest.mark.parametrize("with_z", [True, False])
@pytest.mark.parametrize("gap", [False, True])
@pytest.mark.parametrize("J", [1, 2, 3, 5, 8])
def test_adjoint_vs_complex_step(J, gap, with_z):
    from oracle import exact

    worst = 0.0
    for N in (1, 2, 3, 17, 40):
        k = _factored(1000 * J + N, N, J, gap)
        rng = np.random.default_rng(7 * J + N)
        bq, balpha = rng.normal(size=N), (rng.normal(size=N) if with_z else None)
        args = [k["t"], k["c"], k["U"], k["W"], k["d"]] + ([k["z"]] if with_z else [])

        def f(*a):
            q, alpha, _, _ = RR.forward_states(*a)
            s = np.sum(bq * q, axis=-1)
            return s + np.sum(balpha * alpha, axis=-1) if with_z else s

        ref = exact.cstep_grad(f, args)
        q, alpha, Mws, Fws = RR.forward_states(*args)
        bt, bc, bU, bW, bd, bz = RR.adjoint(k["t"], k["c"], k["U"], k["W"], k["d"], k["z"] if with_z else None, q, alpha, Mws, Fws,
                                            bq, balpha)
        got = [bt, bc, bU, bW, bd] + ([bz] if with_z else [])
        assert with_z or bz is None
        for name, x, xo in zip(("bt", "bc", "bU", "bW", "bd", "bz"), got, ref):
            e = _err(x, xo)
            worst = max(worst, e)
            assert e <= 1.0, (name, N, e)
    print("J = %d, gap %s, z %s: worst adjoint error / criterion %.3g" % (J, gap, with_z, worst))


def _chain_grad(k):
    """loo and (bt, bc, ba, bU, bV, by) through the restated chain: factor and solve_lower as float64 recursions under
    torch's CPU autograd, the inverse diagonal and its reverse from tests/inverse_diag_rev_ref.py."""
    import torch

    class InvDiag(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t, c, U, W, d, z):
            a = [x.detach().numpy() for x in (t, c, U, W, d, z)]
            q, alpha, Mws, Fws = RR.forward_states(*a)
            ctx.stuff = (a, q, alpha, Mws, Fws)
            return torch.from_numpy(q), torch.from_numpy(alpha)

        @staticmethod
        def backward(ctx, bq, balpha):
            a, q, alpha, Mws, Fws = ctx.stuff
            return tuple(torch.from_numpy(g) for g in RR.adjoint(*a, q, alpha, Mws, Fws, bq.numpy(), balpha.numpy()))

    t, c, a, U, V, y = [torch.tensor(k[n], dtype=torch.float64, requires_grad=True) for n in ("t", "c", "a", "U", "V", "y")]
    N, J = U.shape
    S = torch.zeros((J, J), dtype=torch.float64)
    F = torch.zeros(J, dtype=torch.float64)
    d, W, z = [a[0]], [V[0] / a[0]], [y[0]]
    for n in range(1, N):
        p = torch.exp(-c * (t[n] - t[n - 1]))
        S = torch.outer(p, p) * (S + d[-1] * torch.outer(W[-1], W[-1]))
        F = p * (F + W[-1] * z[-1])
        tmp = U[n] @ S
        d.append(a[n] - tmp @ U[n])
        W.append((V[n] - tmp) / d[-1])
        z.append(y[n] - U[n] @ F)
    q, alpha = InvDiag.apply(t, c, U, torch.stack(W), torch.stack(d), torch.stack(z))
    loo = 0.5 * (torch.log(q) - alpha * alpha / q).sum() - 0.5 * N * RR.LOG2PI
    loo.backward()
    return float(loo.detach()), [x.grad.numpy() for x in (t, c, a, U, V, y)]


@pytest.mark.parametrize("gap", [False, True])
@pytest.mark.parametrize("J", [1, 2, 3, 4, 5, 8])
def test_dense_closed_form_vs_restated_chain(J, gap):
    worst = 0.0
    for N in (2, 33, 150):
        k = R.draw(10 * J + N, N, J, gap=gap)
        K = R.dense(k["t"], k["c"], k["a"], k["U"], k["V"])
        assert np.linalg.cond(K) <= 1e6, (N, np.linalg.cond(K))   # a bad draw fails here instead of loosening anything below
        val_o, grads_o = RR.dense_loo_grad(k["t"], k["c"], k["a"], k["U"], k["V"], k["y"])
        val, grads = _chain_grad(k)
        assert abs(val - val_o) <= 1e-10 * abs(val_o) + 1e-12, (N, val, val_o)
        for name, x, xo in zip(("bt", "bc", "ba", "bU", "bV", "by"), grads, grads_o):
            e = _err(x, xo)
            worst = max(worst, e)
            assert e <= 1.0, (name, N, e)
    print("J = %d, gap %s: worst chain error / criterion %.3g" % (J, gap, worst))


def test_objective_is_the_sum_of_leave_one_out_densities():
    k = _factored(5, 33, 4, False)
    q, alpha = R.inverse_diag(k["t"], k["c"], k["U"], k["W"], k["d"], z=k["z"])
    K = R.dense(k["t"], k["c"], k["a"], k["U"], k["V"])
    ref = np.array([R.delete_one(K, k["y"], n) for n in range(33)])
    dens = -0.5 * np.log(2 * np.pi * ref[:, 1]) - 0.5 * (k["y"] - ref[:, 0]) ** 2 / ref[:, 1]
    assert abs(RR.loo_value(q, alpha) - dens.sum()) <= 1e-10 * abs(dens.sum())
    assert abs(RR.dense_loo(K, k["y"])[0] - dens.sum()) <= 1e-10 * abs(dens.sum())


def test_abi_argument_errors():
    """The new entry points reject null pointers / non-positive sizes (C2_ERR_INVALID) and widths above C2_FAST_WIDTH
    (C2_ERR_UNSUPPORTED) before anything touches the device."""
    from celerite2_amd import _lib, build

    build.build_all()
    for name in ("c2_inverse_diag_fwd", "c2_inverse_diag_rev", "c2_get_celerite_matrices_rev"):
        assert name in _lib.HEADERS["main"].symbols
    lib = _lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first

    def fwd(B, N, J, z=null, alpha=null, Mws=one, Fws=null, q=one):
        return lib.c2_inverse_diag_fwd(i64(B), i64(N), i64(J), one, i64(0), one, i64(0), one, one, one, z, q, alpha, Mws, Fws, null)

    assert fwd(0, 4, 2) == fwd(1, 0, 2) == fwd(1, 4, 0) == _lib.C2_ERR_INVALID
    assert fwd(1, 4, 2, Mws=null) == _lib.C2_ERR_INVALID
    assert fwd(1, 4, 2, z=one, alpha=one) == _lib.C2_ERR_INVALID              # z without Fws
    assert fwd(1, 4, 2, Fws=one) == _lib.C2_ERR_INVALID                       # Fws without z
    assert fwd(1, 4, 2, z=one, Fws=one) == _lib.C2_ERR_INVALID                # z without alpha
    assert fwd(1, 4, 2, q=null) == _lib.C2_ERR_INVALID
    assert fwd(1, 4, 33) == fwd(1, 4, 40) == fwd(1, 4, 128) == _lib.C2_ERR_UNSUPPORTED

    def rev(B, N, J, z=null, alpha=null, Fws=null, balpha=null, bz=null, bq=one, bd=one):
        return lib.c2_inverse_diag_rev(i64(B), i64(N), i64(J), one, i64(0), one, i64(0), one, one, one, z, one, alpha, one, Fws, bq,
                                       balpha, one, one, one, one, bd, bz, null)

    assert rev(0, 4, 2) == rev(1, 0, 2) == rev(1, 4, 0) == _lib.C2_ERR_INVALID
    assert rev(1, 4, 2, bq=null) == rev(1, 4, 2, bd=null) == _lib.C2_ERR_INVALID
    assert rev(1, 4, 2, z=one) == rev(1, 4, 2, balpha=one) == rev(1, 4, 2, bz=one) == _lib.C2_ERR_INVALID
    assert rev(1, 4, 2, z=one, alpha=one, Fws=one, balpha=one) == _lib.C2_ERR_INVALID   # no bz
    assert rev(1, 4, 33) == _lib.C2_ERR_UNSUPPORTED

    def mrev(B, N, Jr, Jc, ac=one, bar=one, work=null, nbytes=0):
        return lib.c2_get_celerite_matrices_rev(i64(B), i64(N), i64(Jr), i64(Jc), ac, one, one, ctypes.c_int(0), one, i64(0), one,
                                                one, one, one, one, one, bar, one, one, one, one, one, one, one, work,
                                                ctypes.c_size_t(nbytes), null)

    assert mrev(0, 4, 1, 1) == mrev(1, 0, 1, 1) == mrev(1, 4, 0, 0) == _lib.C2_ERR_INVALID
    assert mrev(1, 4, 1, 1, ac=null) == mrev(1, 4, 1, 1, bar=null) == _lib.C2_ERR_INVALID
    assert mrev(1, 4, 1, 16) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_get_celerite_matrices_rev_workspace_bytes(64, 8192, 1, 1) == 0      # (no split from 64 series)
    assert lib.c2_get_celerite_matrices_rev_workspace_bytes(3, 8191, 1, 1) == 0
    assert lib.c2_get_celerite_matrices_rev_workspace_bytes(3, 8192, 1, 2) == 8 * 3 * 4 * 3 * 4
    assert mrev(3, 8192, 1, 2) == _lib.C2_ERR_INVALID                                # the split needs its workspace
    assert mrev(3, 8192, 1, 2, work=one, nbytes=8) == _lib.C2_ERR_INVALID
