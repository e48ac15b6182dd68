# -*- coding: utf-8 -*-
"""Linear mean models on the CPU: the numpy restatement of the whitened Gram sweep (tests/linear_model_ref.py, what
csrc/c2_gram.hip implements) against dense algebra, the formulas of autograd.gls against dense generalized least squares,
the composed backward rule of autograd.whitened_gram against complex-step derivatives and against torch autograd through
the dense closed form, and the binding of the second public header (include/celerite2_amd_linear.h), which needs no
device.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element."""
import ctypes

import numpy as np
import pytest
import torch

import linear_model_ref as R
from general_rev_ref import close

WIDTHS = [1, 2, 3, 8, 16, 32]
LENGTHS = [1, 2, 9, 33, 150]
COLUMNS = [1, 2, 5, 9, 17, 32]


@pytest.mark.parametrize("J", WIDTHS)
def test_restatement_against_dense(J):
    """Y^T K^-1 Y from the plain recurrence and from the sweep in the kernel's order, on every (N, Q): both triangles at the
    standing criterion against the dense value; y present on every other case (never at Q = 1: the entry point takes P >= 1)."""
    worst = [0.0, 0.0]
    for i, N in enumerate(LENGTHS):
        for k, Q in enumerate(COLUMNS):
            D = R.case(100 * J + 10 * i + k, N, J, Q, with_y=Q > 1 and (i + k) % 2 == 0)
            want = D["Y"].T @ np.linalg.solve(R.dense(D["t"], D["c"], D["a"], D["U"], D["V"]), D["Y"])
            args = [D[x] for x in ("t", "c", "U", "W", "d", "Y")]
            for m, fn in enumerate((R.whitened_gram_rows, R.whitened_gram)):
                got = fn(*args)
                assert got.shape == (Q, Q)
                e = R.err(got, want)
                worst[m] = max(worst[m], e)
                assert e <= 1.0, (J, N, Q, fn.__name__, e)
            assert np.array_equal(got, got.T)      # the kernel's order is symmetric to the bit
    print("J = %d: worst fraction of the criterion: rows %.3g, kernel order %.3g" % (J, *worst))


def gram_of(D, A, r):
    return R.whitened_gram(D["t"], D["c"], D["U"], D["W"], D["d"], np.concatenate([A, r[:, None]], axis=1))


@pytest.mark.parametrize("N,J,P", [(40, 3, 3), (33, 8, 5), (9, 2, 1)])
@pytest.mark.parametrize("prior", ["flat", "gaussian", "gaussian_batched_mean"])
def test_gls_formulas(N, J, P, prior):
    """autograd._linear_fit (the torch part of `gls`) on the restated Gram matrix against linear_model_ref.dense_gls: beta, cov,
    the likelihood at beta, the Gaussian-prior marginal as log N(y | A mu0, K + A Lam^-1 A^T), and the flat-prior marginal two
    ways: at the standing criterion against the density of the data projected on null(A^T), and as the limit Lam = eps I with
    the divergence removed, to the bound dense_gls works out for that limit (its bias and its conditioning)."""
    from celerite2_amd import autograd as ag

    D = R.case(7 * N + J, N, J, P + 1)
    rng = np.random.default_rng(N + P)
    A, y = D["A"], D["y"] + D["A"] @ rng.normal(size=P)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    mu0 = Lam = None
    if prior != "flat":
        M = rng.normal(size=(P, P))
        mu0, Lam = rng.normal(size=P), M @ M.T + 0.5 * np.eye(P)
    r = y if mu0 is None else y - A @ mu0
    S = torch.from_numpy(gram_of(D, A, r))[None]
    tt = lambda v: None if v is None else torch.from_numpy(np.asarray(v))
    pm = tt(mu0) if prior != "gaussian_batched_mean" else tt(mu0)[None]
    fit, bad = ag._linear_fit(S, torch.tensor([np.log(D["d"]).sum()]), N, pm, tt(Lam))
    assert not bool(bad.any())
    eps = 1e-7
    beta, cov, ll, mll = R.dense_gls(K, A, y, mu0, Lam, eps=eps)
    what = (N, J, P, prior)
    close(fit.beta[0].numpy(), beta, "beta %s" % (what,))
    close(fit.cov[0].numpy(), cov, "cov %s" % (what,))
    close(fit.log_likelihood.numpy(), np.array([ll]), "ll %s" % (what,))
    # the likelihood at beta, formed from beta itself
    resid = y - A @ fit.beta[0].numpy()
    pen = 0.0 if Lam is None else 0.5 * (fit.beta[0].numpy() - mu0) @ Lam @ (fit.beta[0].numpy() - mu0)
    close(fit.log_likelihood.numpy(), np.array([R.log_normal(resid, K) - pen]), "ll at beta %s" % (what,))
    got = float(fit.marginal_log_likelihood[0])
    if Lam is None:
        sharp, (limit, bound) = mll
        print("%s: flat marginal %.12g; null-space form %.12g; limit %.12g (bound %.3g)" % (what, got, sharp, limit, bound))
        close(np.array([got]), np.array([sharp]), "mll %s" % (what,))
        assert abs(got - limit) <= bound, (what, got, limit, bound)
    else:
        close(np.array([got]), np.array([mll]), "mll %s" % (what,))


def test_issue_value():
    """N = 40, J = 3, P = 3: the Gaussian-prior marginal both ways (dense and through the Gram matrix) agree to 1e-10."""
    from celerite2_amd import autograd as ag

    D = R.case(3, 40, 3, 4)
    rng = np.random.default_rng(0)
    mu0, Lam = rng.normal(size=3), np.diag(rng.uniform(0.5, 2.0, 3))
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    want = R.log_normal(D["y"] - D["A"] @ mu0, K + D["A"] @ np.linalg.solve(Lam, D["A"].T))
    S = torch.from_numpy(gram_of(D, D["A"], D["y"] - D["A"] @ mu0))[None]
    fit, _ = ag._linear_fit(S, torch.tensor([np.log(D["d"]).sum()]), 40, torch.from_numpy(mu0), torch.from_numpy(Lam))
    assert abs(float(fit.marginal_log_likelihood[0]) - want) <= 1e-10 * abs(want)


def test_rank_deficient_and_failed_series():
    """A repeated column gives a bad series (NaN beta / cov, -inf likelihoods) and leaves its neighbour alone; `ok` does too."""
    from celerite2_amd import autograd as ag

    D = R.case(5, 33, 3, 4)
    A2 = D["A"].copy()
    A2[:, 2] = A2[:, 1]
    S = torch.from_numpy(np.stack([gram_of(D, D["A"], D["y"]), gram_of(D, A2, D["y"]), gram_of(D, D["A"], D["y"])]))
    ld = torch.full((3,), float(np.log(D["d"]).sum()))
    fit, bad = ag._linear_fit(S, ld, 33, None, None, ok=torch.tensor([True, True, False]))
    assert bad.tolist() == [False, True, True]
    assert bool(torch.isfinite(fit.beta[0]).all()) and bool(torch.isfinite(fit.cov[0]).all()) and bool(torch.isfinite(fit.log_likelihood[0]))
    for b in (1, 2):
        assert bool(torch.isnan(fit.beta[b]).all()) and bool(torch.isnan(fit.cov[b]).all())
        assert float(fit.log_likelihood[b]) == -np.inf and float(fit.marginal_log_likelihood[b]) == -np.inf
    one, _ = ag._linear_fit(S[:1], ld[:1], 33)
    assert torch.equal(one.beta[0], fit.beta[0]) and torch.equal(one.marginal_log_likelihood[0], fit.marginal_log_likelihood[0])


SHAPES = [(1, 1, 1), (9, 2, 3), (17, 8, 5), (33, 5, 9), (6, 32, 4)]      # (N, J, Q)
NAMES = ("bt", "bc", "bU", "bW", "bd", "bY")


def test_backward_rule_against_complex_step():
    """bZ, bd feeding the restated reverse of the sweep: all six cotangents against complex-step derivatives of the
    restatement, element by element, at 1e-12 of each array's largest entry."""
    h = 1e-30
    worst = 0.0
    for i, (N, J, Q) in enumerate(SHAPES):
        D = R.case(300 + i, N, J, Q)
        args = [D[x] for x in ("t", "c", "U", "W", "d", "Y")]
        bS = np.random.default_rng(i).normal(size=(Q, Q))      # (not symmetric: both triangles are outputs)
        got = R.whitened_gram_rev(*args, bS)
        for k, (a, g, nm) in enumerate(zip(args, got, NAMES)):
            num = np.zeros_like(a)
            for idx in np.ndindex(a.shape):
                ac = [x.astype(complex) for x in args]
                ac[k][idx] += 1j * h
                num[idx] = (bS * R.whitened_gram_rows(*ac).imag).sum() / h
            scale = float(np.max(np.abs(num)))
            e = float(np.max(np.abs(num - g))) / (scale if scale > 0 else 1.0)
            worst = max(worst, e)
            assert e <= 1e-12, (nm, (N, J, Q), e)
    print("worst complex-step error / largest entry: %.3g" % worst)


def test_backward_rule_against_dense_autograd():
    """factor -> whitened Gram against Y^T K^-1 Y under torch float64 autograd: the value and the derivative with respect to
    t, c, a, U, V, Y at the standing criterion, per array.  The sweep's reverse is the restatement; factor's is torch autograd
    of its recurrence."""
    worst = 0.0
    for i, (N, J, Q) in enumerate(SHAPES + [(40, 3, 4)]):
        D = R.case(400 + i, N, J, Q)
        bS = np.random.default_rng(i).normal(size=(Q, Q))
        bt, bc, bU, bW, bd, bY = R.whitened_gram_rev(*[D[x] for x in ("t", "c", "U", "W", "d", "Y")], bS)
        tt = [torch.tensor(D[x], dtype=torch.float64, requires_grad=True) for x in ("t", "c", "a", "U", "V")]
        dT, WT = R.torch_factor(*tt)
        ft, fc, fa, fU, fV = torch.autograd.grad((dT, WT), tt, (torch.tensor(bd), torch.tensor(bW)), allow_unused=True)
        z = lambda g, like: np.zeros_like(like) if g is None else g.numpy()
        got = (bt + z(ft, bt), bc + z(fc, bc), z(fa, bt), bU + z(fU, bU), z(fV, bU), bY)
        dd = [torch.tensor(D[x], dtype=torch.float64, requires_grad=True) for x in ("t", "c", "a", "U", "V", "Y")]
        S = dd[5].T @ torch.linalg.solve(R.torch_dense(*dd[:5]), dd[5])
        want = torch.autograd.grad(S, dd, torch.tensor(bS), allow_unused=True)
        for nm, g, w in zip(("bt", "bc", "ba", "bU", "bV", "bY"), got, want):
            worst = max(worst, close(g, z(w, g), "%s %s" % (nm, (N, J, Q))))
    print("worst %.3g of the criterion" % worst)


# ---- the binding of the second header ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def gram_args(B=1, N=4, J=2, P=1, p=None, y=None, S=None):
    return [B, N, J, P, p, 0, p, 0, p, p, p, p, 0, y, S, None]


def test_linear_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib

    fn = lib.c2_whitened_gram
    assert len(fn.argtypes) == 16 and fn.restype is ctypes.c_int
    assert fn.argtypes[:4] == (ctypes.c_int64,) * 4 and fn.argtypes[4] is _lib.Pointer and fn.argtypes[12] is ctypes.c_int64


def test_bad_gram_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_whitened_gram(*gram_args()[:-1])
    with pytest.raises(refused):
        lib.c2_whitened_gram(*gram_args(), None)
    with pytest.raises(refused):
        lib.c2_whitened_gram(*gram_args(B=1.0))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_whitened_gram(*gram_args(p=text))


def test_gram_argument_errors(lib):
    """Sizes and null pointers are refused before anything is launched: no device is needed."""
    from celerite2_amd import _lib

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    assert lib.c2_whitened_gram(*gram_args(P=0, p=p, y=None, S=p)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_gram(*gram_args(p=p, y=p, S=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_gram(*gram_args(J=33, p=p, y=p, S=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_gram(*gram_args(P=32, p=p, y=p, S=p)) == _lib.C2_ERR_UNSUPPORTED      # Q = 33
    assert lib.c2_whitened_gram(*gram_args(P=33, p=p, y=None, S=p)) == _lib.C2_ERR_UNSUPPORTED
    for bad in (dict(B=0), dict(N=0), dict(J=0), dict(P=-1)):
        assert lib.c2_whitened_gram(*gram_args(p=p, y=p, S=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_whitened_gram(*gram_args(p=None, y=p, S=p)) == _lib.C2_ERR_INVALID


def test_ops_shape_errors_name_the_argument():
    """ops.whitened_gram and the design-matrix check refuse shapes before a pointer reaches a kernel (CPU tensors: the dtype /
    device check comes first, so the helpers are called directly)."""
    from celerite2_amd import autograd as ag, ops

    dims = dict(B=2, N=5, J=2, P=3, Q=4)
    ops._shapes(dims, [("A", torch.zeros(5, 3), "NP|BNP"), ("A", torch.zeros(2, 5, 3), "NP|BNP"), ("S", torch.zeros(2, 4, 4), "BQQ")])
    with pytest.raises(ValueError, match=r"^Invalid shape: A "):
        ops._shapes(dims, [("A", torch.zeros(2, 3, 5), "NP|BNP")])
    with pytest.raises(ValueError, match=r"^Invalid shape: S "):
        ops._shapes(dims, [("S", torch.zeros(2, 3, 3), "BQQ")])
    for bad in (torch.zeros(5), torch.zeros(4, 3), torch.zeros(3, 5, 3), torch.zeros(2, 5, 3, 1), torch.zeros(5, 0)):
        with pytest.raises(ValueError, match=r"^Invalid shape: A "):
            ag._check_design(bad, 2, 5, None, None)
    assert ag._check_design(torch.zeros(5, 3), 2, 5, torch.zeros(3), torch.zeros(2, 3, 3)) == 3
    with pytest.raises(ValueError, match=r"^Invalid shape: prior_mean "):
        ag._check_design(torch.zeros(5, 3), 2, 5, torch.zeros(4), None)
    with pytest.raises(ValueError, match=r"^Invalid shape: prior_precision "):
        ag._check_design(torch.zeros(5, 3), 2, 5, None, torch.zeros(3, 4))
