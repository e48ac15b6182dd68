# -*- coding: utf-8 -*-
"""Exact references for the gradients (oracle/exact.py), and the CPU restatement's reverse passes held to them.

The closed forms (G = (alpha alpha^T - K^-1) / 2 contracted with dK) are first shown equal to complex-step derivatives of
analytic forwards at small N -- that is what makes them trustworthy at N = 1000, where complex step is too slow -- then
the restatement (oracle/c2_oracle.cpp: loglik_grad, factor_rev, the four sweep reverses) and the numpy chain rules of
oracle/dense.py are pinned to them at 1e-12 .. 1e-13 of each array's largest entry, where the forward-difference checks
of tests/test_oracle.py reach about 3e-4.  The reference's own dense K (tests/golden/ref_golden.npz) anchors them."""
import numpy as np
import pytest

from oracle import dense
from oracle import exact as ex

MAT = ("bt", "bc", "ba", "bU", "bV", "by")
COEF = ("bar", "bcr", "bac", "bbc", "bcc", "bdc", "bx", "bdiag", "by")
SWEEPS = ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper")
CPP_KERNELS = ["real", "complex", "sho1", "sho2", "sum1", "sum2", "sum3", "sum4"]


def agree(got, want, tol, names):
    for nm, g, w in zip(names, got, want):
        e = ex.relerr(g, w)
        assert e <= tol, (nm, e)


def series(N, J, seed=5, ties=False):
    """One well-conditioned series of width J: J // 2 underdamped SHO terms (+ one real term in front for odd J)."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, max(N, 2) / 10.0, N))
    if ties and N > 4:
        t[N // 2] = t[N // 2 - 1]
        t[1] = t[0]
    diag = rng.uniform(0.1, 0.3, N)
    co = dense.sho_sum_coeffs(J - J % 2, rng.uniform(-1, 1)) if J >= 2 else None
    if J % 2:
        r = dense.real_term(1.3, 0.4)
        co = r if co is None else r + co
    c, a, U, V = dense.celerite_matrices(co, t, diag)
    y = np.sin(t) + 0.1 * rng.standard_normal(N)
    return t, c, a + 1.0, U, V, y


def coeffs(Jr, Jc, rng):
    ar = rng.uniform(0.5, 1.5, Jr); cr = rng.uniform(0.05, 0.5, Jr)
    ac = rng.uniform(0.5, 2.0, Jc); cc = rng.uniform(0.02, 0.3, Jc); dc = rng.uniform(0.2, 3.0, Jc)
    bc = ac * cc / dc * rng.uniform(0.0, 0.9, Jc)
    return ar, cr, ac, bc, cc, dc


# ---- the closed forms against complex step ----------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("N,ties", [(2, False), (9, False), (24, False), (24, True)])
def test_matrix_level_closed_form_equals_complex_step(N, J, ties):
    t, c, a, U, V, y = series(N, J, seed=N + J, ties=ties)
    ll, g = ex.loglik_grad(t, c, a, U, V, y)
    assert abs(ll - float(ex.dense_loglik_fwd(t, c, a, U, V, y))) <= 1e-13 * abs(ll)
    agree(g, ex.cstep_grad(ex.dense_loglik_fwd, [t, c, a, U, V, y]), 1e-13, MAT)
    # and the O(N) recursion (factor + forward solve) differentiated the same way
    agree(g, ex.cstep_grad(ex.recursive_loglik_fwd, [t, c, a, U, V, y]), 1e-13, MAT)


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (0, 1), (2, 0), (0, 2), (1, 1), (2, 3), (3, 1), (0, 4)])
@pytest.mark.parametrize("N", [1, 5, 30])
def test_coefficient_level_closed_form_equals_complex_step(N, Jr, Jc):
    rng = np.random.default_rng(100 * N + 10 * Jr + Jc)
    co = coeffs(Jr, Jc, rng)
    x = np.sort(rng.uniform(0, N / 10.0, N))
    if N > 4:
        x[3] = x[2]                        # a tie: the later row's derivative, as the semiseparable form takes it
    diag = rng.uniform(0.1, 0.3, N)
    y = np.sin(x) + 0.1 * rng.standard_normal(N)
    ll, g = ex.terms_grad(*co, x, diag, y)
    assert abs(ll - float(ex.terms_loglik_fwd(*co, x, diag, y))) <= 1e-13 * abs(ll)
    agree(g, ex.cstep_grad(ex.terms_loglik_fwd, [*co, x, diag, y]), 1e-13, COEF)


@pytest.mark.parametrize("N,M,J", [(6, 3, 2), (10, 2, 3), (5, 4, 4), (7, 1, 2)])
def test_kron_closed_form_equals_complex_step(N, M, J):
    t, c, a, U, V, alpha, diag, y, _ = dense.kron_synthetic(1, N, M, J)
    t, c, a, U, V, alpha, diag, y = (x[0] for x in (t, c, a, U, V, alpha, diag, y))

    def fwd(t_, c_, a_, U_, V_, al_, dg_, y_):
        low = np.tril(np.ones((N, N), bool), -1)
        dtl = np.where(low, t_[..., :, None] - t_[..., None, :], 0.0)
        Tl = np.einsum("...nj,...mj,...nmj->...nm", U_, V_, np.exp(-c_[..., None, None, :] * dtl[..., None])) * low
        T = Tl + np.swapaxes(Tl, -1, -2) + a_[..., :, None] * np.eye(N)
        aa = al_[..., :, None] * al_[..., None, :]
        K = np.einsum("...nk,...ml->...nmkl", T, aa)
        K = K.reshape(K.shape[:-4] + (N * M, N * M))
        K = K + dg_.reshape(dg_.shape[:-2] + (N * M,))[..., :, None] * np.eye(N * M)
        return ex._dense_ll(K, y_.reshape(y_.shape[:-2] + (N * M,)))

    ll, g = ex.kron_grad(t, c, a, U, V, alpha, diag, y)
    assert abs(ll - float(fwd(t, c, a, U, V, alpha, diag, y))) <= 1e-13 * abs(ll)
    agree(g, ex.cstep_grad(fwd, [t, c, a, U, V, alpha, diag, y]), 1e-13,
          ("bt", "bc", "ba", "bU", "bV", "balpha", "bdiag", "by"))


@pytest.mark.parametrize("name", SWEEPS)
@pytest.mark.parametrize("J,nrhs", [(1, 1), (2, 3), (3, 2), (4, 1)])
def test_sweep_vjp_closed_form_equals_complex_step(name, J, nrhs):
    N = 14
    t, c, a, U, V, y = series(N, J, seed=7 * J + nrhs, ties=True)
    W = ex.factor_fwd(t, c, a, U, V)[1] if name.startswith("solve") else V
    rng = np.random.default_rng(J + nrhs)
    Y = rng.standard_normal((N, nrhs)); bZ = rng.standard_normal((N, nrhs))
    Z, g = ex.sweep_vjp(name, t, c, U, W, Y, bZ)
    assert ex.relerr(ex.sweep_fwd(name, t, c, U, W, Y), Z) <= 1e-14
    f = lambda t_, c_, U_, W_, Y_: np.sum(bZ * ex.sweep_fwd(name, t_, c_, U_, W_, Y_), axis=(-1, -2))
    agree(g, ex.cstep_grad(f, [t, c, U, W, Y]), 1e-13, ("bt", "bc", "bU", "bW", "bY"))


# ---- the reference's own dense K -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", ["cpp_%s_" % k for k in CPP_KERNELS] + ["py_"])
def test_gradient_on_the_reference_dense_matrix(oracle, golden, p):
    """G from the reference's K = term.to_dense() == the closed form from (t, c, a, U, V) == the restatement; for py_ the
    committed py_grad_* (the restatement's own output when the fixture was made) are thereby checked, not circular."""
    x, c, a, U, V, Y = (np.ascontiguousarray(golden[p + k]) for k in ("x", "c", "a", "U", "V", "Y"))
    y = np.ascontiguousarray(Y[:, 0])
    llK, gK = ex.loglik_grad_from_K(golden[p + "K"], y, x, c, U, V)
    ll, g = ex.loglik_grad(x, c, a, U, V, y)
    assert abs(llK - ll) <= 1e-13 * abs(ll)
    agree(g, gK, 2e-12, MAT)
    llo, go, flag = oracle.loglik_grad(x, c, a, U, V, y)
    assert flag == 0 and abs(llo - llK) <= 1e-12 * abs(llK)
    agree(go, gK, 2e-12, MAT)
    if p == "py_":
        agree([golden["py_grad_" + nm] for nm in MAT], gK, 2e-12, MAT)


@pytest.mark.parametrize("case", ["gp8a", "gp8b", "gprot"])
def test_gradient_on_the_reference_coefficients(oracle, golden, case):
    """K built from the reference term classes' stored coefficients: its G pushed to (t, c, a, U, V, y) == the closed form
    from the stored matrices == the restatement; the coefficient-level gradients == the oracle chain; the log-likelihood
    == the reference GaussianProcess's."""
    g = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "_")}
    co = [np.atleast_1d(g["coef_" + n]) for n in ("ar", "cr", "ac", "bc", "cc", "dc")]
    x, c, a, U, V = (np.ascontiguousarray(g[k]) for k in ("x", "c", "a", "U", "V"))
    y = np.ascontiguousarray(g["y"] - g["mean"])
    K = ex.terms_dense(*co, x, g["diag"])
    llK, gK = ex.loglik_grad_from_K(K, y, x, c, U, V)
    assert abs(llK - float(g["loglik"])) <= 1e-12 * abs(llK)
    agree(ex.loglik_grad(x, c, a, U, V, y)[1], gK, 2e-12, MAT)
    _, go, flag = oracle.loglik_grad(x, c, a, U, V, y)
    assert flag == 0
    agree(go, gK, 2e-12, MAT)
    llt, gt = ex.terms_grad(*co, x, g["diag"], y)
    assert abs(llt - llK) <= 1e-13 * abs(llK)
    _, gch, flag = dense.coefficient_chain(oracle, *co, x, g["diag"], y)
    agree(gch, gt, 2e-12, COEF)


# ---- the restatement against the exact forms --------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("N", [2, 17, 300, 1000])
def test_oracle_loglik_grad_vs_closed_form(oracle, N, J):
    t, c, a, U, V, y = series(N, J, seed=3 * N + J)
    ll, g = ex.loglik_grad(t, c, a, U, V, y)
    llo, go, flag = oracle.loglik_grad(t, c, a, U, V, y)
    assert flag == 0 and abs(llo - ll) <= 1e-12 * abs(ll)
    agree(go, g, 2e-12, MAT)


def _factor_phi(bd, bW):
    def f(t, c, a, U, V):
        d, W = ex.factor_fwd(t, c, a, U, V)
        return np.sum(bd * d, axis=-1) + np.sum(bW * W, axis=(-1, -2))
    return f


def _cotangents(rng, shapes, onehot):
    if onehot is None:
        return [rng.standard_normal(s) for s in shapes]
    k, i = onehot
    out = [np.zeros(s) for s in shapes]
    out[k].flat[i % out[k].size] = 1.0
    return out


@pytest.mark.parametrize("cot", ["random", "onehot_first", "onehot_mid", "onehot_last"])
@pytest.mark.parametrize("kernel,N", [("real", 10), ("sum2", 10), ("sum3", 10), ("sum4", 97)])
def test_oracle_factor_rev_vs_complex_step(oracle, kernel, N, cot):
    x, diag, _ = dense.cpp_test_data(N, 1)
    c, a, U, V = dense.celerite_matrices(dense.cpp_test_kernels()[kernel], x, diag)
    J = len(c)
    rng = np.random.default_rng(N + J)
    oh = {"random": None, "onehot_first": (0, 0), "onehot_mid": (1, (N // 2) * J + J // 2), "onehot_last": (0, N - 1)}[cot]
    bd, bW = _cotangents(rng, [(N,), (N, J)], oh)
    d = np.empty(N); W = np.empty((N, J)); S = np.empty((N, J, J))
    oracle.factor(x, c, a, U, V, d, W, S)
    outs = [np.zeros(N), np.zeros(J), np.zeros(N), np.zeros((N, J)), np.zeros((N, J))]
    oracle.factor_rev(x, c, a, U, V, d, W, S, bd, bW, *outs)
    want = ex.cstep_grad(_factor_phi(bd, bW), [x, c, a, U, V])
    agree(outs, want, 1e-13, ("bt", "bc", "ba", "bU", "bV"))


@pytest.mark.parametrize("cot", ["random", "onehot_first", "onehot_last"])
@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("kernel,N", [("complex", 10), ("sum3", 10), ("sum2", 101)])
@pytest.mark.parametrize("op", SWEEPS)
def test_oracle_sweep_rev_vs_complex_step(oracle, op, kernel, N, nrhs, cot):
    x, diag, Y = dense.cpp_test_data(N, nrhs)
    c, a, U, V = dense.celerite_matrices(dense.cpp_test_kernels()[kernel], x, diag)
    J = len(c)
    if op.startswith("solve"):
        d = np.empty_like(a); W = np.empty_like(V)
        oracle.factor(x, c, a, U, V, d, W)
    else:
        W = V
    rng = np.random.default_rng(N + nrhs)
    oh = {"random": None, "onehot_first": (0, 0), "onehot_last": (0, N * nrhs - 1)}[cot]
    (bZ,) = _cotangents(rng, [(N, nrhs)], oh)
    Z = np.empty_like(Y); F = np.empty((N, J, nrhs))
    getattr(oracle, op + "_fwd")(x, c, U, W, Y, Z, F)
    outs = [np.zeros(N), np.zeros(J), np.zeros((N, J)), np.zeros((N, J)), np.zeros((N, nrhs))]
    getattr(oracle, op + "_rev")(x, c, U, W, Y, Z, F, bZ, *outs)
    f = lambda t_, c_, U_, W_, Y_: np.sum(bZ * ex.sweep_fwd(op, t_, c_, U_, W_, Y_), axis=(-1, -2))
    agree(outs, ex.cstep_grad(f, [x, c, U, W, Y]), 1e-13, ("bt", "bc", "bU", "bW", "bY"))
    # ... and the dense VJP gives the same
    agree(outs, ex.sweep_vjp(op, x, c, U, W, Y, bZ)[1], 1e-13, ("bt", "bc", "bU", "bW", "bY"))


# ---- the numpy chain rules of oracle/dense.py ------------------------------------------------------------------
@pytest.mark.parametrize("Jr,Jc,N", [(1, 0, 40), (0, 1, 40), (2, 3, 120), (0, 4, 300), (3, 1, 77)])
def test_coefficient_chain_vs_exact(oracle, Jr, Jc, N):
    rng = np.random.default_rng(10 * Jr + Jc + N)
    co = coeffs(Jr, Jc, rng)
    x = np.sort(rng.uniform(0, N / 10.0, N))
    diag = rng.uniform(0.1, 0.3, N)
    y = np.sin(x) + 0.1 * rng.standard_normal(N)
    ll, g = ex.terms_grad(*co, x, diag, y)
    llo, go, flag = dense.coefficient_chain(oracle, *co, x, diag, y)
    assert flag == 0 and abs(llo - ll) <= 1e-12 * abs(ll)
    agree(go, g, 2e-12, COEF)


@pytest.mark.parametrize("N,M,J", [(16, 3, 2), (40, 4, 4), (64, 2, 6), (7, 1, 2), (30, 5, 3)])
def test_kron_fold_gradients_vs_exact(oracle, N, M, J):
    """The oracle on the interleaved series, folded back by dense.kron_fold_gradients: the interleaved parametrisation
    carries same-epoch cross-band terms through U_n . V_n, so (bU, bV) are compared as the totals bU + ba V, bV + ba U."""
    t, c, a, U, V, alpha, diag, y, _ = dense.kron_synthetic(1, N, M, J)
    t, c, a, U, V, alpha, diag, y = (x[0] for x in (t, c, a, U, V, alpha, diag, y))
    ll, g = ex.kron_grad(t, c, a, U, V, alpha, diag, y)
    t2, c2, a2, U2, V2 = dense.kron_interleaved(c, a, U, V, t, alpha, diag)
    llo, g2, flag = oracle.loglik_grad(t2, c2, a2, U2, V2, np.ascontiguousarray(y.ravel()))
    assert flag == 0 and abs(llo - ll) <= 1e-12 * abs(ll)
    fo = dense.kron_fold_gradients(g2, a, U, V, alpha)
    tot = lambda h: (h[0], h[1], h[3] + h[2][:, None] * V, h[4] + h[2][:, None] * U, h[5], h[6], h[7])
    agree(tot(fo), tot(g), 2e-12, ("bt", "bc", "bU+baV", "bV+baU", "balpha", "bdiag", "by"))
