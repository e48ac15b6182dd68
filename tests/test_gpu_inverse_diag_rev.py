# -*- coding: utf-8 -*-
"""GPU checks of the leave-one-out objective and of what it is built on: ops.inverse_diag(..., workspace=True)
(c2_inverse_diag_fwd), ops.inverse_diag_rev (c2_inverse_diag_rev, csrc/c2_invdiag_rev.hip), autograd.inverse_diag /
loo_log_predictive / loo_log_predictive_kernel and GaussianProcess.loo_log_predictive[_kernel].

References: the numpy restatement of the sweep with its states and of its adjoint (tests/inverse_diag_rev_ref.py, pinned to
complex-step derivatives and to the dense closed form by tests/test_inverse_diag_rev.py), fed with the device's own inputs
and workspace, and the dense closed form of the objective's gradient.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; a reference that is identically zero must be met exactly.  Every
dense input has a condition number <= 1e6, asserted per draw."""
import math

import numpy as np
import pytest

import inverse_diag_ref as R
import inverse_diag_rev_ref as RR
import term_params_ref as TP

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
ROWS = [1, 2, 15, 16, 17, 33, 150]   # no decay row, one, the 16-row block boundary from both sides, several blocks
WORST = {}


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


def dev(*xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(x):
    return None if x is None else x.detach().cpu().numpy()


def err(x, xo):
    x = host(x) if hasattr(x, "cpu") else np.asarray(x)
    xo = np.asarray(xo)
    if not np.any(xo):
        return 0.0 if not np.any(x) else np.inf
    return R.err(x, xo)


def check(key, x, xo, what=None):
    e = err(x, xo)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert e <= 1.0, (what, key, e)


def batch(seed, B, N, J, *, per_series, gap=False, distinct=3):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct); per_series: every series on its own grid
    with its own rates, else all on the first draw's t and c (shared (N,) and (J,) arrays)."""
    draws = [R.draw(1000 * seed, N, J, gap=gap)]
    for k in range(1, min(B, distinct)):
        draws.append(R.draw(1000 * seed + k, N, J, gap=gap, t=None if per_series else draws[0]["t"]))
    idx = [b % len(draws) for b in range(B)]
    stack = lambda key: np.stack([draws[i][key] for i in idx])
    return dict(draws=draws, idx=idx, t=stack("t") if per_series else draws[0]["t"],
                c=stack("c") if per_series else draws[0]["c"], a=stack("a"), U=stack("U"), V=stack("V"), y=stack("y"))


def factored(ops, bt):
    t, c, a, U, V, y = dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    z = ops.solve_lower(t, c, U, W, y[..., None].contiguous())[..., 0].contiguous()
    return t, c, U, W, d, z


def series(x, b, per):
    x = host(x)
    return x[b] if x.ndim == per + 1 else x


def cotangents(seed, B, N):
    """Series b: random (b mod 4 == 0), one-hot in row 0, in row N - 1, in the row at the block boundary (16, or N - 1)."""
    rng = np.random.default_rng(seed)
    bq, ba = rng.standard_normal((B, N)), rng.standard_normal((B, N))
    for b in range(B):
        if b % 4:
            row = (0, N - 1, min(16, N - 1))[b % 4 - 1]
            s, r = bq[b, row], ba[b, row]
            bq[b], ba[b] = 0.0, 0.0
            bq[b, row], ba[b, row] = s, r
    return bq, ba


def grid(J):
    for i, N in enumerate(ROWS):
        for B in (3, 70):   # 70: a padded last wavefront and a partial group
            yield N, B, bool((i + (B == 70)) % 2), (N == 150 and B == 3)


@pytest.mark.parametrize("J", WIDTHS)
def test_forward_with_workspace(ops, J):
    """q and alpha have the bits of the plain call; Mws, Fws against the restatement fed with the device's d, W, z."""
    import torch

    for N, B, per, gap in grid(J):
        bt = batch(10 * J + N, B, N, J, per_series=per, gap=gap)
        t, c, U, W, d, z = factored(ops, bt)
        what = (J, N, B, per)
        q0 = ops.inverse_diag(t, c, U, W, d)
        q1, a1 = ops.inverse_diag(t, c, U, W, d, z=z)
        q2, (M2, F2) = ops.inverse_diag(t, c, U, W, d, workspace=True)
        q3, a3, (M3, F3) = ops.inverse_diag(t, c, U, W, d, z=z, workspace=True)
        torch.cuda.synchronize()
        assert F2 is None and tuple(M3.shape) == (B, N, J, J) and tuple(F3.shape) == (B, N, J), what
        assert torch.equal(q0, q2) and torch.equal(q1, q3) and torch.equal(a1, a3) and torch.equal(M2, M3), what
        assert not bool(M3[:, N - 1].any()) and not bool(F3[:, N - 1].any()), what
        for b in sorted(set(range(min(B, 3))) | {B - 1}):
            args = [series(t, b, 1), series(c, b, 1), host(U)[b], host(W)[b], host(d)[b], host(z)[b]]
            qr, ar, Mr, Fr = RR.forward_states(*args)
            check("q", q3[b], qr, what); check("alpha", a3[b], ar, what)
            check("Mws", M3[b], Mr, what); check("Fws", F3[b], Fr, what)
        if B == 70:   # a repeat of a draw: identical inputs give identical bits
            assert torch.equal(M3[69], M3[0]) and torch.equal(F3[69], F3[0]), what


def test_forward_with_workspace_rejects_wide_models(ops):
    bt = batch(3, 2, 5, 40, per_series=True)
    t, c, U, W, d, z = factored(ops, bt)
    with pytest.raises(ValueError, match="width not supported"):
        ops.inverse_diag(t, c, U, W, d, workspace=True)
    with pytest.raises(ValueError, match="width not supported"):
        ops.inverse_diag_rev(t, c, U, W, d, None, d.clone(), None, (W.new_zeros((2, 5, 40, 40)), None), d.clone(), None)


def rev_case(ops, bt, seed, what, every=False):
    import torch

    B, N, J = bt["U"].shape
    t, c, U, W, d, z = factored(ops, bt)
    bq, ba = dev(*cotangents(seed, B, N))
    q, alpha, ws = ops.inverse_diag(t, c, U, W, d, z=z, workspace=True)
    got = ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba)
    got0 = ops.inverse_diag_rev(t, c, U, W, d, None, q, None, (ws[0], None), bq, None)
    torch.cuda.synchronize()
    assert got0[5] is None and [tuple(g.shape) for g in got] == [(B, N), (B, J), (B, N, J), (B, N, J), (B, N), (B, N)], what
    names = ("bt", "bc", "bU", "bW", "bd", "bz")
    for b in (range(B) if every else sorted(set(range(min(B, 8))) | {B - 1})):
        args = [series(t, b, 1), series(c, b, 1), host(U)[b], host(W)[b], host(d)[b]]
        qb, ab, Mb, Fb = host(q)[b], host(alpha)[b], host(ws[0])[b], host(ws[1])[b]
        ref = RR.adjoint(*args, host(z)[b], qb, ab, Mb, Fb, host(bq)[b], host(ba)[b])
        for nm, g, r in zip(names, got, ref):
            check(nm, g[b], r, (what, b, "with z"))
        ref0 = RR.adjoint(*args, None, qb, None, Mb, None, host(bq)[b], None)
        for nm, g, r in zip(names[:5], got0, ref0):
            check(nm, g[b], r, (what, b, "without z"))


@pytest.mark.parametrize("J", WIDTHS)
def test_reverse_vs_restatement(ops, J):
    """All six outputs, with and without z, random and one-hot cotangents (row 0, row N - 1, a block-boundary row), against
    the numpy adjoint fed with the device's own inputs and workspace."""
    for N, B, per, gap in grid(J):
        rev_case(ops, batch(20 * J + N, B, N, J, per_series=per, gap=gap), J + N, (J, N, B, per))


@pytest.mark.parametrize("J", [8, 32])
def test_reverse_long_series(ops, J):
    """N = 4097: 256 full blocks of 16 rows and a last block of one."""
    rev_case(ops, batch(55 + J, 2, 4097, J, per_series=True, distinct=2), J, (J, 4097), every=True)


def dense_batch(bt, B):
    out = []
    for b in range(B):
        dr = bt["draws"][bt["idx"][b]]
        tb = bt["t"][b] if bt["t"].ndim == 2 else bt["t"]
        cb = bt["c"][b] if bt["c"].ndim == 2 else bt["c"]
        K = R.dense(tb, cb, dr["a"], dr["U"], dr["V"])
        assert np.linalg.cond(K) <= 1e6, (b, np.linalg.cond(K))
        out.append(RR.dense_loo_grad(tb, cb, dr["a"], dr["U"], dr["V"], dr["y"]))
    return out


@pytest.mark.parametrize("per", [True, False])
@pytest.mark.parametrize("J", [1, 2, 5, 8, 16, 32])
def test_loo_log_predictive_vs_dense_closed_form(ops, J, per):
    """Value and all six gradients; a shared t and c receive the batch sum."""
    import torch
    from celerite2_amd import autograd as ag

    B = 5
    for N in (2, 33, 150):
        bt = batch(30 * J + N, B, N, J, per_series=per, distinct=B)
        want = dense_batch(bt, B)
        leaves = [x.requires_grad_() for x in dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])]
        loo = ag.loo_log_predictive(*leaves)
        loo.sum().backward()
        what = (J, N, per)
        check("loo", loo, np.array([w[0] for w in want]), what)
        for k, nm in enumerate(("bt", "bc", "ba", "bU", "bV", "by")):
            ref = np.stack([w[1][k] for w in want])
            if k < 2 and not per:
                ref = ref.sum(0)
            assert tuple(leaves[k].grad.shape) == ref.shape, (what, nm)
            check("grad " + nm, leaves[k].grad, ref, (what, nm))


def test_autograd_inverse_diag_without_z(ops):
    """q alone, composed with autograd.factor: sum_n w_n q_n against d/dK of sum_n w_n [K^-1]_nn."""
    import torch
    from celerite2_amd import autograd as ag
    from oracle import exact

    B, N, J = 3, 33, 4
    bt = batch(77, B, N, J, per_series=True, distinct=B)
    wts = np.random.default_rng(7).standard_normal((B, N))
    leaves = [x.requires_grad_() for x in dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"])]
    d, W = ag.factor(*leaves)
    q = ag.inverse_diag(leaves[0], leaves[1], leaves[3], W, d)
    (q * dev(wts)[0]).sum().backward()
    for b in range(B):
        dr = bt["draws"][b]
        Ki = np.linalg.inv(R.dense(dr["t"], dr["c"], dr["a"], dr["U"], dr["V"]))
        A = -(Ki * wts[b][None, :]) @ Ki
        A = 0.5 * (A + A.T)
        ref = exact.contract_lower(2.0 * A, dr["t"], dr["c"], dr["U"], dr["V"])
        for k, r in zip((0, 1, 3, 4), ref):
            check("q-only grad", leaves[k].grad[b], r, (b, k))
        check("q-only grad", leaves[2].grad[b], np.diag(A), (b, "ba"))


# ---- hyper-parameters -------------------------------------------------------------------------------------------------
RECS = [TP.rec("sho", (0, 1, 2), regime="under"), TP.rec("real", (3, 4)), TP.rec("matern32", (5, 6))]
SHARED_COLS = (4, 5)   # RealTerm.c and Matern32Term.sigma are 0-d tensors; the other parameters (B,) columns


def kernel_case(seed, B, N):
    rng = np.random.default_rng(seed)
    P = np.concatenate([TP.draw("sho", rng, B, regime="under")[1], TP.draw("real", rng, B)[1], TP.draw("matern32", rng, B)[1]], 1)
    P[:, SHARED_COLS] = P[0, SHARED_COLS]
    x = np.sort(rng.uniform(0, max(N, 2) / 10.0, (B, N)), axis=1)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    return P, x, ye, y, rng.uniform(0.05, 0.4, B), float(rng.uniform(-0.3, 0.3))


def exact_series(Pb, xb, yeb, jb, m, yb):
    """loo, bP, bjitter, bmean, bx, byerr, by of ONE series from the dense kernel matrix of the restated coefficients."""
    from oracle import exact

    coefs = [v[0] for v in TP.coefficients(RECS, Pb[None])]
    K = exact.terms_dense(*coefs, xb, yeb ** 2 + jb ** 2)
    assert np.linalg.cond(K) <= 1e6
    val, A, by = RR.dense_loo(K, yb - m)
    out = RR.terms_contract(A, *coefs, xb)
    bP = TP.coefficients_rev(RECS, Pb[None], [v[None] for v in out[:6]])[0]
    bdiag = out[7]
    return val, bP, 2.0 * jb * bdiag.sum(), -by.sum(), out[6], 2.0 * yeb * bdiag, by


def build_kernel(Pt, sc, ss):
    from celerite2_amd import terms as T
    return (T.SHOTerm(S0=Pt[:, 0], w0=Pt[:, 1], Q=Pt[:, 2], regime="under") + T.RealTerm(a=Pt[:, 3], c=sc)
            + T.Matern32Term(sigma=ss, rho=Pt[:, 6]))


@pytest.mark.parametrize("N", [2, 33, 150])
def test_loo_log_predictive_kernel_vs_exact_dense(ops, N):
    """SHO (under) + Real + Matern32, (B,) and 0-d parameters mixed, a (B,) jitter, a 0-d mean, yerr as sigma: the value and
    the gradient of every tensor, x, yerr and y included."""
    import torch
    from celerite2_amd import autograd as ag

    B = 6
    P, x, ye, y, jit, mean = kernel_case(40 + N, B, N)
    Pt, xd, yed, yd, jt = [v.requires_grad_() for v in dev(P, x, ye, y, jit)]
    sc, ss, mt = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in (P[0, 4], P[0, 5], mean)]
    loo = ag.loo_log_predictive_kernel(build_kernel(Pt, sc, ss), xd, yd, yerr=yed, jitter=jt, mean=mt)
    loo.sum().backward()
    want = [exact_series(P[b], x[b], ye[b], jit[b], mean, y[b]) for b in range(B)]
    bP = np.stack([w[1] for w in want])
    check("kernel loo", loo, np.array([w[0] for w in want]), N)
    per = [k for k in range(7) if k not in SHARED_COLS]
    check("kernel bP", Pt.grad[:, per], bP[:, per], N)
    assert not bool(Pt.grad[:, list(SHARED_COLS)].any())
    check("kernel bP shared", sc.grad, bP[:, 4].sum(), N)
    check("kernel bP shared", ss.grad, bP[:, 5].sum(), N)
    check("kernel bjitter", jt.grad, np.array([w[2] for w in want]), N)
    check("kernel bmean", mt.grad, np.sum([w[3] for w in want]), N)
    check("kernel bx", xd.grad, np.stack([w[4] for w in want]), N)
    check("kernel byerr", yed.grad, np.stack([w[5] for w in want]), N)
    check("kernel by", yd.grad, np.stack([w[6] for w in want]), N)
    # without a tensor that requires grad: the same value from the plain sweeps
    with torch.no_grad():
        plain = ag.loo_log_predictive_kernel(build_kernel(Pt.detach(), sc.detach(), ss.detach()), xd.detach(), yd.detach(),
                                             yerr=yed.detach(), jitter=jt.detach(), mean=mt.detach())
    check("kernel loo", plain, host(loo), N)


def _gp_inputs(seed, B, N):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 0.05 * N + 5, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.4, (B, N))
    y = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3
    return x, diag, y


def _dense_of_gp(gp, b):
    t = host(gp._t)
    return R.dense(t[b] if t.ndim == 2 else t, host(gp._c)[b] if gp._c.dim() == 2 else host(gp._c), host(gp._a)[b],
                   host(gp._U)[b], host(gp._V)[b])


@pytest.mark.parametrize("kind", ["product", "convolution"])
def test_term_algebra_kernels_vs_the_factored_matrix(ops, kind):
    """A TermProduct and a TermConvolution (a TermExpr program with its diagonal shift): value, bdiag, by and bmean against
    the dense inverse of the matrix rebuilt from the GP's own celerite matrices."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N = 4, 150
    x, diag, y = _gp_inputs(5, B, N)
    xd, dd, yd = dev(x, diag, y)
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True)
    pars = [tn(1.2), tn(0.9), tn(2.5), tn(0.7)]
    base = T.SHOTerm(S0=pars[0], w0=pars[1], Q=pars[2], regime="under")
    real = T.RealTerm(a=pars[3], c=0.3)
    kernel = T.TermProduct(base, real) if kind == "product" else T.TermConvolution(base + real, 0.05)
    mean = tn(0.3)
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=mean)
    dd.requires_grad_(); yd.requires_grad_()
    loo = gp.loo_log_predictive_kernel(yd)
    assert torch.equal(loo, ag.loo_log_predictive_kernel(kernel, gp._t, yd, diag=gp._diag, mean=mean))
    loo.sum().backward()
    bm = 0.0
    for b in range(B):
        K = _dense_of_gp(gp, b)
        assert np.linalg.cond(K) <= 1e6
        val, A, by = RR.dense_loo(K, y[b] - 0.3)
        check(kind + " loo", loo[b], val, b)
        check(kind + " bdiag", dd.grad[b], np.diag(A), b)
        check(kind + " by", yd.grad[b], by, b)
        bm -= by.sum()
    check(kind + " bmean", mean.grad, bm, kind)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs()) > 0 for p in pars)


def test_gp_loo_log_predictive(ops):
    """gp.loo_log_predictive(y) is the sum over n of the log density of gp.leave_one_out(y), and the autograd value;
    gp.loo_log_predictive_kernel is the autograd function on the GP's own t, diag, mean."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N = 6, 150
    x, diag, y = _gp_inputs(6, B, N)
    xd, dd, yd = dev(x, diag, y)
    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kernel = T.SHOTerm(S0=t(1.2), w0=t(0.9), Q=t(2.5), regime="under") + T.RealTerm(a=t(0.7), c=0.3)
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=t(0.3))
    loo = gp.loo_log_predictive(yd)
    mu, var = gp.leave_one_out(yd)
    dens = -0.5 * np.log(2 * np.pi * host(var)) - 0.5 * (y - host(mu)) ** 2 / host(var)
    assert tuple(loo.shape) == (B,)
    check("gp loo", loo, dens.sum(1))
    check("gp loo", loo, host(ag.loo_log_predictive(gp._t, gp._c, gp._a, gp._U, gp._V, yd - 0.3)))
    lk = gp.loo_log_predictive_kernel(yd, jitter=t(0.2))
    assert torch.equal(lk, ag.loo_log_predictive_kernel(kernel, gp._t, yd, diag=gp._diag, jitter=t(0.2), mean=gp.mean))
    check("gp loo", gp.loo_log_predictive_kernel(yd), host(loo))
    for b in (0, B - 1):
        val = RR.dense_loo(_dense_of_gp(gp, b), y[b] - 0.3)[0]
        check("gp loo", loo[b], val, b)


def test_failed_series_gets_minus_inf_and_zero_gradient(ops):
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N = 9, 100
    x, diag, y = _gp_inputs(9, B, N)
    bad = diag.copy()
    bad[4, 37] = -50.0   # not positive definite from row 37 on
    xd, bd, yd = dev(x, bad, y)
    ok = [b for b in range(B) if b != 4]

    def run(g):
        pars = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in (1.2, 0.9, 2.5, 0.7, 0.3, 0.2, 0.3)]
        kernel = T.SHOTerm(S0=pars[0], w0=pars[1], Q=pars[2], regime="under") + T.RealTerm(a=pars[3], c=pars[4])
        loo = ag.loo_log_predictive_kernel(kernel, xd, yd, diag=bd, jitter=pars[5], mean=pars[6])
        loo.backward(gradient=g)
        return loo, [p.grad for p in pars]

    ones = torch.ones(B, dtype=torch.float64, device="cuda")
    masked = ones.clone()
    masked[4] = 0.0
    loo1, g1 = run(ones)
    loo2, g2 = run(masked)
    assert float(loo1[4].detach()) == -math.inf and bool(torch.isfinite(loo1[ok]).all()) and torch.equal(loo1, loo2)
    for a, b in zip(g1, g2):
        assert bool(torch.isfinite(a).all()) and float(a.abs()) > 0 and torch.equal(a, b)
    gp = G.GaussianProcess(T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3), mean=0.3).compute(xd, diag=bd, quiet=True)
    v = gp.loo_log_predictive(yd)
    assert float(v[4]) == -math.inf and bool(torch.isfinite(v[ok]).all())


@pytest.mark.parametrize("J", [2, 8, 32])
def test_two_calls_give_identical_bits(ops, J):
    import torch

    B, N = 130, 200
    bt = batch(21, B, N, J, per_series=True, distinct=6)
    t, c, U, W, d, z = factored(ops, bt)
    bq, ba = dev(*cotangents(J, B, N))
    q, alpha, ws = ops.inverse_diag(t, c, U, W, d, z=z, workspace=True)
    g1 = ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba)
    g2 = ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_graph_capture_of_the_forward_and_reverse_sweeps(ops):
    """One torch.cuda.graph capture of solve_lower -> inverse_diag(workspace) -> inverse_diag_rev on caller-owned buffers
    replays correctly on new data."""
    import torch

    B, N, J = 12, 257, 8
    bt = batch(31, B, N, J, per_series=True, distinct=12)
    t, c, a, U, V, y = dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
    d, W, flag = ops.factor(t, c, a, U, V)
    Y = y[..., None].contiguous()
    Z, q, alpha = torch.empty_like(Y), torch.empty_like(d), torch.empty_like(d)
    f64 = dict(dtype=torch.float64, device="cuda")
    ws = (torch.empty((B, N, J, J), **f64), torch.empty((B, N, J), **f64))
    out = (torch.empty((B, N), **f64), torch.empty((B, J), **f64), torch.empty((B, N, J), **f64), torch.empty((B, N, J), **f64),
           torch.empty((B, N), **f64), torch.empty((B, N), **f64))
    bq, ba = dev(*cotangents(5, B, N))

    def chain():
        ops.solve_lower(t, c, U, W, Y, Z=Z)
        ops.inverse_diag(t, c, U, W, d, z=Z[..., 0], q=q, alpha=alpha, ws=ws)
        ops.inverse_diag_rev(t, c, U, W, d, Z[..., 0], q, alpha, ws, bq, ba, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    y2 = torch.from_numpy(np.random.default_rng(32).standard_normal(tuple(y.shape))).cuda()
    Y.copy_(y2[..., None])
    for o in (q, alpha) + out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    z_e = ops.solve_lower(t, c, U, W, y2[..., None].contiguous())[..., 0].contiguous()
    q_e, alpha_e, ws_e = ops.inverse_diag(t, c, U, W, d, z=z_e, workspace=True)
    out_e = ops.inverse_diag_rev(t, c, U, W, d, z_e, q_e, alpha_e, ws_e, bq, ba)
    assert torch.equal(q, q_e) and torch.equal(alpha, alpha_e)
    assert all(torch.equal(a, b) for a, b in zip(out, out_e))
    ref = RR.adjoint(host(t)[0], host(c)[0], host(U)[0], host(W)[0], host(d)[0], host(z_e)[0], host(q)[0], host(alpha)[0],
                     host(ws[0])[0], host(ws[1])[0], host(bq)[0], host(ba)[0])
    for g, r in zip(out, ref):
        check("graph", g[0], r)


def test_seventy_thousand_series(ops):
    """B = 70 000 x N = 16 x J = 4: runs, and the first and last series equal the same series alone."""
    import torch

    B, N, J = 70000, 16, 4
    rng = np.random.default_rng(8)
    base = R.draw(8, N, J)
    scale = rng.uniform(0.5, 2.0, B)
    a = base["k0"] * scale[:, None] + base["diag"][None] * rng.uniform(0.5, 2.0, (B, 1))
    U = base["U"][None] * scale[:, None, None]
    V = np.broadcast_to(base["V"][None], (B, N, J))
    t, c, ad, Ud, Vd, yd, bq, ba = dev(base["t"], base["c"], a, U, V, rng.standard_normal((B, N)), rng.standard_normal((B, N)),
                                       rng.standard_normal((B, N)))
    d, W, flag = ops.factor(t, c, ad, Ud, Vd)
    z = ops.solve_lower(t, c, Ud, W, yd[..., None].contiguous())[..., 0].contiguous()
    q, alpha, ws = ops.inverse_diag(t, c, Ud, W, d, z=z, workspace=True)
    got = ops.inverse_diag_rev(t, c, Ud, W, d, z, q, alpha, ws, bq, ba)
    torch.cuda.synchronize()
    assert int(flag.abs().sum()) == 0 and all(bool(torch.isfinite(g).all()) for g in got)
    for b in (0, B - 1):
        s = slice(b, b + 1)
        one = [x[s].contiguous() for x in (Ud, W, d, z, bq, ba)]
        q1, a1, ws1 = ops.inverse_diag(t, c, one[0], one[1], one[2], z=one[3], workspace=True)
        assert torch.equal(q1[0], q[b]) and torch.equal(a1[0], alpha[b]) and torch.equal(ws1[0][0], ws[0][b])
        alone = ops.inverse_diag_rev(t, c, one[0], one[1], one[2], one[3], q1, a1, ws1, one[4], one[5])
        for g, g1 in zip(got, alone):
            assert torch.equal(g[b], g1[0]), b


def test_shape_and_aliasing_errors(ops):
    import torch

    bt = batch(41, 2, 10, 3, per_series=False)
    t, c, U, W, d, z = factored(ops, bt)
    q, alpha, ws = ops.inverse_diag(t, c, U, W, d, z=z, workspace=True)
    bq, ba = torch.ones_like(d), torch.ones_like(d)
    with pytest.raises(ValueError, match="Invalid shape: bq"):
        ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq[:, :-1].contiguous(), ba)
    with pytest.raises(ValueError, match="Invalid shape: balpha"):
        ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba[:1].contiguous())
    with pytest.raises(ValueError, match="Invalid shape: Mws"):
        ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, (ws[1], ws[1]), bq, ba)
    with pytest.raises(ValueError, match="Invalid shape: balpha"):
        ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, None)
    with pytest.raises(ValueError, match="Invalid shape: Fws"):
        ops.inverse_diag(t, c, U, W, d, ws=ws)
    with pytest.raises(ValueError, match="alpha must not alias z"):
        ops.inverse_diag(t, c, U, W, d, z=z, alpha=z, workspace=True)
    with pytest.raises(ValueError, match="q must not alias d"):
        ops.inverse_diag(t, c, U, W, d, q=d, workspace=True)
    good = ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba)
    for k, (nm, other) in enumerate((("bt", bq), ("bc", c), ("bU", U), ("bW", W), ("bd", d), ("bz", z))):
        out = list(good)
        out[k] = other if other.shape == good[k].shape else None
        if out[k] is None:   # (c is shared here: (J,) cannot stand in for (B, J))
            continue
        with pytest.raises(ValueError, match="%s must not alias" % nm):
            ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba, out=tuple(out))
    out = list(good)
    out[4] = out[0]
    with pytest.raises(ValueError, match="bd must not alias bt"):
        ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, ba, out=tuple(out))


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
