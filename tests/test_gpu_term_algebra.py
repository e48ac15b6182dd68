# -*- coding: utf-8 -*-
"""Term algebra on the device (csrc/c2_term_expr.hip, ops.TermExpr, ops.term_coefficients[_rev] on an expression,
ops.noise_mean_shift_*, ops.loglik_kernel_grad, autograd.log_likelihood_kernel, TermProduct / TermDiff / TermConvolution
with tensor parameters, GaussianProcess) against

  * what the REFERENCE's term classes and GaussianProcess produced (tests/golden/algebra_golden.npz) and the numpy
    restatement of tests/term_algebra_ref.py (pinned to them by tests/test_term_algebra.py): 1e-13 of each series' largest
    entry per array, the standing figure of tests/test_gpu_term_params.py -- times max(1, kappa) under a convolution when the
    comparison is with the REFERENCE (kappa = 2 / |z|^2: the loss of its closed forms, tests/test_term_algebra.py);
  * the exact complex-step Jacobian of that restatement, and end to end oracle.exact.cstep_grad of the DENSE log-likelihood
    of restatement(P), yerr^2 + jitter^2 + shift, y - mean: the standing 1e-10 |exact| + 1e-12 max |exact|.

Reads only the .npz, never the reference."""
import os

import numpy as np
import pytest

import term_algebra_ref as A
import term_params_ref as R
from oracle import exact

pytestmark = pytest.mark.gpu
CN = ("ar", "cr", "ac", "bc", "cc", "dc")
HERE = os.path.dirname(os.path.abspath(__file__))
WORST = {"rev": 0.0, "e2e": 0.0}


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def fixtures():
    with np.load(os.path.join(HERE, "golden", "algebra_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def dev(*xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(x):
    return x.detach().cpu().numpy()


def close(a, b, tol=1e-10, floor=1e-12, what=None, key=None):
    a = host(a) if hasattr(a, "cpu") else np.asarray(a)
    b = np.asarray(b)
    if key is not None and b.size:
        WORST[key] = max(WORST[key], float(np.max(np.abs(a - b) / (tol * np.abs(b) + floor * max(1.0, float(np.abs(b).max()))))))
    np.testing.assert_allclose(a, b, rtol=tol, atol=floor * max(1.0, float(np.abs(b).max())), err_msg=str(what))


def force(monkeypatch, which):
    """The lane mappings of c2_loglik_terms[_grad], as tests/test_gpu_term_params.py forces them."""
    if which == "default":
        return
    monkeypatch.setenv("C2_TERMS_FUSED", "1" if which == "one" else "0")
    monkeypatch.setenv("C2_TERMS_TWO_LANES", "1" if which == "two" else "0")
    monkeypatch.setenv("C2_TERMS_EIGHT_LANES", "1" if which == "eight" else "0")
    monkeypatch.setenv("C2_TERMS_FOUR_LANES", "1" if which == "four" else "0")


def expr_of(ops, expr, NP):
    records, operations = expr
    e = ops.TermExpr([dict(r, cols=tuple(r["cols"])) for r in records],
                     [dict(op=o["op"], a=o["a"], b=o["b"], col=o["col"]) for o in operations], NP)
    assert e.operations == operations
    return e


def tensor_kernel(name, requires_grad=False):
    import torch
    from celerite2_amd import terms as T

    cases = dict(A.build_cases(T, lambda x: torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=requires_grad)))
    return cases[name]()


# ---- 5. coefficients and their reverse -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.CASES)
def test_coefficients_vs_reference(ops, fixtures, name):
    k = tensor_kernel(name)
    prog = k.program
    assert isinstance(prog, ops.TermExpr)
    P = k.parameter_matrix()
    assert P.dim() == 1
    kap = float(A.kappa((prog.records, prog.operations), host(P)))
    for Pin, B in ((P, 3), (P[None].repeat(3, 1).contiguous(), None)):   # shared (NP,) and per-series (B, NP)
        co, flag, shift = ops.term_coefficients(prog, Pin, B)
        assert int(flag.abs().sum()) == 0
        for cn, g in zip(CN, co):
            want = fixtures["%s_%s" % (name, cn)]
            assert tuple(g.shape) == (3,) + want.shape
            if want.size:
                err = np.max(np.abs(host(g) - want[None])) / np.max(np.abs(want))
                print("%s %s: err %.2e (band %.2e)" % (name, cn, err, 1e-13 * kap))
                assert err <= 1e-13 * kap, (name, cn, err)
        a = fixtures["diag"][None] + host(co[0].sum(1) + co[2].sum(1) + shift)[:, None]
        assert np.max(np.abs(a - fixtures[name + "_a"][None])) <= 1e-13 * kap * np.max(fixtures[name + "_a"])
        assert (float(shift.abs().max()) > 0) == name.startswith("conv")
    # the differentiable front: coefficients(B) are the same numbers
    for u, v in zip(k.coefficients(3), co):
        assert np.array_equal(host(u), host(v))


def check_shift(expr, P, shift):
    """delta_diag on the scale of the terms it sums, |(a - i b) G(z)| each (|a| |z| / 3 at small z): for an SHO / Matern-3/2
    term they cancel to O(delta^3) (a c = b d: the process is differentiable), and what is left has the absolute rounding of
    its terms, in the restatement as on the device."""
    records, operations = expr
    want = A.coefficients(expr, P)[6]
    if not operations or operations[-1]["op"] != "convolve":
        assert np.all(host(shift) == 0.0) and np.all(want == 0.0)
        return
    inner = A.coefficients((records, operations[:-1]), P)
    dt = P[:, operations[-1]["col"]]
    dt = dt[:, None]
    scale = (np.sum(np.abs(inner[0] * A._conv_fg(inner[1] * dt)[1]), axis=1)
             + np.sum(np.abs((inner[2] - 1j * inner[3]) * A._conv_fg((inner[4] - 1j * inner[5]) * dt)[1]), axis=1))
    err = float(np.max(np.abs(host(shift) - want) / scale))
    print("shift: worst err / sum |(a - i b) G(z)| = %.3g" % err)
    assert err <= 1e-13, err


def check_draws(ops, expr, P, rng):
    """Device coefficients vs the restatement (1e-13 of each series' largest entry per array: both sum the same series /
    closed forms, so no kappa) and the shift (check_shift); then the reverse vs the restatement's exact Jacobian (random
    cotangents, the shift's included) at 1e-10 |exact| + 1e-12 max |exact| per series, and vs the numpy reverse it restates."""
    prog = expr_of(ops, expr, P.shape[1])
    (Pd,) = dev(P)
    co, flag, shift = ops.term_coefficients(prog, Pd)
    assert int(flag.abs().sum()) == 0
    want = A.coefficients(expr, P)
    for cn, g, w in zip(CN, co, want[:6]):
        if w.size:
            top = np.max(np.abs(w), axis=1, keepdims=True)      # (a mixed term's inactive amplitudes: an all-zero row, exact)
            err = float(np.max(np.abs(host(g) - w) / np.where(top == 0.0, 1.0, top)))
            assert err <= 1e-13, (cn, err)
    check_shift(expr, P, shift)
    cots = A.zero_inactive_rate_cotangents(expr, P, [rng.standard_normal(w.shape) for w in want[:6]])
    bshift = rng.standard_normal(P.shape[0])
    bP = ops.term_coefficients_rev(prog, Pd, dev(*cots), bshift=dev(bshift)[0])
    exactJ = A.exact_jacobian(expr, P, cots, bshift, h=exact.H)
    got = host(bP)
    last = expr[1][-1]
    if last["op"] == "convolve":        # delta is data: its gradient is not built
        assert np.all(got[:, last["col"]] == 0.0)
        exactJ[:, last["col"]] = 0.0
    tol = 1e-10 * np.abs(exactJ) + 1e-12 * np.maximum(1.0, np.max(np.abs(exactJ), axis=1, keepdims=True))
    ratio = float(np.max(np.abs(got - exactJ) / tol))
    WORST["rev"] = max(WORST["rev"], ratio)
    print("term_coefficients_rev: worst |err| / allowed = %.3g" % ratio)
    assert ratio <= 1.0, ratio
    close(bP, A.coefficients_rev(expr, P, cots, bshift), tol=1e-10, floor=1e-12)


@pytest.mark.parametrize("x,y", A.PRODUCTS)
def test_product_coefficients_and_reverse_vs_restatement(ops, x, y):
    rng = np.random.default_rng(4096 + 7 * len(x) + len(y))
    check_draws(ops, *A.draw_operation("product", x, y, rng, 4096), rng)


@pytest.mark.parametrize("x", ["real", "complex", "under", "over", "matern32", "rotation"])
def test_diff_coefficients_and_reverse_vs_restatement(ops, x):
    rng = np.random.default_rng(5000 + 11 * len(x))
    check_draws(ops, *A.draw_operation("diff", x, None, rng, 4096), rng)


@pytest.mark.parametrize("x", ["real", "complex", "under", "over", "matern32", "rotation"])
def test_convolve_coefficients_and_reverse_vs_restatement(ops, x):
    rng = np.random.default_rng(6000 + 11 * len(x))
    check_draws(ops, *A.draw_operation("convolve", x, None, rng, 4096), rng)


def test_nested_and_mixed_expressions_vs_restatement(ops):
    rng = np.random.default_rng(4141)
    check_draws(ops, *A.nested_expr(rng, 4096), rng)
    # a mixed SHO (half the series on each side) times (real + matern32), convolved
    n = 4096
    records, P = A.join(A.draw_leaf("mixed", rng, n), A.draw_leaf("real", rng, n), A.draw_leaf("matern32", rng, n))
    P = np.concatenate([P, A.draw_delta(rng, n)], axis=1)
    ops_ = [dict(op="sum", a=A.leaf_range(records, 1), b=A.leaf_range(records, 2)), dict(op="product", a=A.leaf_range(records, 0), b=0),
            dict(op="convolve", a=1, col=P.shape[1] - 1)]
    check_draws(ops, (records, A.resolve(records, ops_)), P, rng)
    # two leaves on different sides of a product read the same columns
    a, c, d = rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.5, n), rng.uniform(0.2, 3.0, n)
    records = [R.rec("real", (0, 1)), R.rec("complex", (0, 2, 1, 3))]
    expr = (records, A.resolve(records, [dict(op="product", a=(0, 1, 0, 0), b=(0, 0, 0, 1))]))
    check_draws(ops, expr, np.stack([a, c, 0.3 * a, d], axis=1), rng)


def test_wrong_side_leaf_is_reported_through_the_algebra(ops):
    rng = np.random.default_rng(9)
    expr, P = A.draw_operation("product", "under", "real", rng, 70)
    P[17, 2] = 0.3                      # over-damped under regime="under"
    prog = expr_of(ops, expr, P.shape[1])
    (Pd,) = dev(P)
    co, flag, shift = ops.term_coefficients(prog, Pd)
    assert int(flag[17]) == 1 and int(flag.abs().sum()) == 1
    import torch
    ll = torch.zeros(70, dtype=torch.float64, device="cuda")
    lflag = torch.zeros(70, dtype=torch.int32, device="cuda")
    bP = ops.term_coefficients_rev(prog, Pd, [torch.ones_like(c) for c in co], tflag=flag, lflag=lflag, ll=ll)
    assert float(bP[17].abs().sum()) == 0.0 and float(ll[17]) == -np.inf and int(lflag[17]) == -2 and int(lflag.abs().sum()) == 2
    assert float(bP[16].abs().sum()) > 0.0


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def leaf_kernel(name, B, rng, device_shared=False):
    """The fixture kernel `name` with every parameter its OWN leaf tensor: (B,) draws within 10 % of the fixture's values, or
    0-d (the first draw) when `device_shared`.  Returns (kernel, leaves)."""
    import torch
    from celerite2_amd import terms as T

    leaves = []

    def v(x):
        val = x * rng.uniform(0.9, 1.1, B)
        t = torch.tensor(val[0] if device_shared else val, dtype=torch.float64, device="cuda", requires_grad=True)
        leaves.append(t)
        return t

    return A.build_cases(T, v)[name](), leaves


def gaps_x(rng, B, N):
    return np.cumsum(rng.uniform(A.DELTA_BIG, 0.3, (B, N)), axis=1)      # every gap >= the largest delta


def exact_series(expr, Pb, xb, yeb, jb, mb, yb):
    """(ll, bP, bjitter, bmean) of ONE series: complex step of the dense log-likelihood of the restatement, diag + shift."""
    def f(P, j, m):
        co = A.coefficients(expr, P)
        return exact.terms_loglik_fwd(*co[:6], xb[None], yeb[None] ** 2 + j[:, None] ** 2 + co[6][:, None], yb[None] - m[:, None])

    ll = float(np.real(f(Pb[None].astype(complex), np.array([jb + 0j]), np.array([mb + 0j])))[0])
    g = exact.cstep_grad(f, [Pb, jb, mb])
    return ll, g[0], float(g[1]), float(g[2])


def run_e2e(ops, name, N, lanes, monkeypatch, B, seed):
    import torch
    from celerite2_amd import autograd as ag

    rng = np.random.default_rng(seed)
    x = gaps_x(rng, B, N)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    jit = rng.uniform(0.05, 0.4, B)
    mean = rng.uniform(-0.3, 0.3, B)
    force(monkeypatch, lanes)
    xd, yed, yd = dev(x, ye, y)
    for shared in (False, True):
        kernel, leaves = leaf_kernel(name, B, rng, device_shared=shared)
        jt, mt = [t.requires_grad_() for t in (dev(jit[0], mean[0]) if shared else dev(jit, mean))]
        ll = ag.log_likelihood_kernel(kernel, xd[0].contiguous() if shared else xd, yd, yerr=yed, jitter=jt, mean=mt)
        ll.sum().backward()
        prog, values = kernel._build_program()
        assert isinstance(prog, ops.TermExpr)
        expr = (prog.records, prog.operations)
        P = host(kernel.parameter_matrix(B).detach())
        P = np.broadcast_to(P, (B, P.shape[-1]))
        want = [exact_series(expr, P[b], x[0] if shared else x[b], ye[b], jit[0] if shared else jit[b],
                             mean[0] if shared else mean[b], y[b]) for b in range(B)]
        tag = (name, "shared" if shared else "per series")
        close(ll, np.array([w[0] for w in want]), what=tag + ("ll",))
        bP = np.stack([w[1] for w in want])
        seen = 0
        for k, v in enumerate(values):
            if torch.is_tensor(v) and v.requires_grad:      # (delta is a float: its column has no gradient)
                assert any(v is t for t in leaves)
                close(v.grad, bP[:, k].sum() if shared else bP[:, k], what=tag + ("bP", k), key="e2e")
                seen += 1
        assert seen == len(leaves)
        bj, bm = np.array([w[2] for w in want]), np.array([w[3] for w in want])
        close(jt.grad, bj.sum() if shared else bj, what=tag + ("bjitter",), key="e2e")
        close(mt.grad, bm.sum() if shared else bm, what=tag + ("bmean",), key="e2e")


WIDTH = {"prod_sho_real": 2, "prod_sho_sho": 4, "prod_over_mat": 4, "prod_of_sums": 9, "prod_rot_real": 4, "nested": 5,
         "diff_sho": 2, "diff_mat": 2, "diff_rot_plus": 5, "conv_sho": 2, "conv_over": 2, "conv_sum": 3, "conv_prod": 4,
         "conv_big": 3}
E2E = [(name, lanes) for name in A.CASES
       for lanes in (("composed", "one", "eight") if WIDTH[name] in (2, 4) else ("default",))]


@pytest.mark.parametrize("N", [1, 2, 33, 150])
@pytest.mark.parametrize("name,lanes", E2E)
def test_end_to_end_exact(ops, monkeypatch, name, lanes, N):
    run_e2e(ops, name, N, lanes, monkeypatch, B=70 if N == 150 else 5, seed=N + len(name))


@pytest.mark.parametrize("N", [1, 2, 33, 150])
@pytest.mark.parametrize("lanes", ["composed", "one", "two", "four", "eight"])
def test_end_to_end_exact_width_eight(ops, monkeypatch, lanes, N):
    """(sho + sho2) * sho: two complex terms times one = four complex terms, width 8 -- every lane mapping."""
    run_e2e(ops, "w8", N, lanes, monkeypatch, B=70 if N == 150 else 5, seed=800 + N)


@pytest.mark.parametrize("name", A.CASES)
def test_loglik_vs_reference(ops, fixtures, name):
    """The reference's own number: its GaussianProcess log-likelihood of every fixture kernel."""
    from celerite2_amd import autograd as ag

    kernel = tensor_kernel(name)
    x, diag, y = dev(fixtures["x"], fixtures["diag"][None], fixtures["y"][None])
    ll = ag.log_likelihood_kernel(kernel, x, y, diag=diag)
    want = float(fixtures[name + "_loglik"])
    print("%s: ll %.12f  reference %.12f  rel %.2e" % (name, float(ll[0]), want, abs(float(ll[0]) - want) / abs(want)))
    assert abs(float(ll[0]) - want) <= 1e-10 * abs(want), (float(ll[0]), want)


# ---- 7. the shift variants of the noise / mean kernels --------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(70000, 1), (70000, 2), (3, 4097), (5, 1024), (257, 33)])
def test_noise_mean_shift_kernels(ops, B, N):
    import torch

    rng = np.random.default_rng(B + N)
    ye, y, bd, by = (rng.standard_normal((B, N)) for _ in range(4))
    jit, mean, sh = rng.uniform(0.1, 1, B), rng.standard_normal(B), -rng.uniform(0.0, 0.05, B)
    yed, yd, bdd, byd, jd, md, sd = dev(ye, y, bd, by, jit, mean, sh)
    diag, r = ops.noise_mean_shift_apply(yed, jd, md, sd, yd)
    # the bound of test_noise_mean_kernels (4 * 2^-53 of yerr^2 + jitter^2) plus the one rounding of adding the shift, in
    # numpy and on the device: 6 * 2^-53 of yerr^2 + jitter^2 (the shift is negative: the sum is the smaller number)
    base = ye**2 + jit[:, None] ** 2
    want = base + sh[:, None]
    assert np.max(np.abs(host(diag) - want) / base) <= 6 * 2.0**-53 and np.array_equal(host(r), y - mean[:, None])
    # shift = 0 (and no shift at all): the old kernel's output bit for bit
    old = ops.noise_mean_apply(yed, jd, md, yd)
    for s0 in (torch.zeros_like(sd), None):
        new = ops.noise_mean_shift_apply(yed, jd, md, s0, yd)
        assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    d2, _ = ops.noise_mean_shift_apply(yed, None, None, sd, yd, yerr_is_sigma=False)
    assert np.array_equal(host(d2), ye + sh[:, None])
    bj, bm, bs = ops.noise_mean_shift_rev(jd, bdd, byd)
    bj2, bm2, bs2 = ops.noise_mean_shift_rev(jd, bdd, byd)
    assert torch.equal(bj, bj2) and torch.equal(bm, bm2) and torch.equal(bs, bs2)      # a fixed summation order
    oj, om = ops.noise_mean_rev(jd, bdd, byd)
    assert torch.equal(bj, oj) and torch.equal(bm, om)                                 # the old outputs, bit for bit
    assert np.max(np.abs(host(bs) - bd.sum(1)) / np.abs(bd).sum(1)) <= 1e-14
    assert np.array_equal(host(bj), 2 * jit * host(bs))                                # the row sum bjitter is formed from
    flag = torch.zeros(B, dtype=torch.int32, device="cuda"); flag[1] = 7
    tflag = torch.zeros(B, dtype=torch.int32, device="cuda"); tflag[2] = 1
    bj3, bm3, bs3 = ops.noise_mean_shift_rev(jd, bdd, byd, flag=flag, tflag=tflag)
    assert float(bs3[1]) == 0.0 and float(bj3[1]) == 0.0 and float(bm3[2]) == 0.0 and float(bs3[2]) == 0.0
    assert torch.equal(bs3[3:], bs[3:]) and float(bs3[0]) == float(bs[0])
    with pytest.raises(ValueError, match="Invalid shape: shift"):
        ops.noise_mean_shift_apply(yed, jd, md, sd[:2].contiguous(), yd)


# ---- 8. no host traffic: the whole chain in one captured graph -------------------------------------------------------------
@pytest.mark.parametrize("name", ["prod_sho_sho", "conv_prod"])
def test_loglik_kernel_grad_with_an_expression_is_graph_capturable(ops, name):
    import torch

    rng = np.random.default_rng(93)
    B, N = 70, 150
    kernel, leaves = leaf_kernel(name, B, rng)
    prog = kernel.program
    expr = (prog.records, prog.operations)
    P = host(kernel.parameter_matrix(B).detach())
    x = gaps_x(rng, B, N)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    jit = rng.uniform(0.05, 0.4, B); mean = rng.uniform(-0.3, 0.3, B)
    Pd, xd, yed, jd, md, yd = dev(P, x, ye, jit, mean, y)
    work = ops.loglik_kernel_workspace(prog, B, N, Pd.device)
    assert {"shift", "bshift", "expr"} <= set(work)
    ll, out, flag = ops.loglik_kernel_grad(prog, Pd, xd, yed, jd, md, yd, work=work)     # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                            # one capture: a plain linear chain
        ll_g, out_g, flag_g = ops.loglik_kernel_grad(prog, Pd, xd, yed, jd, md, yd, work=work, out=out)
    for variant in range(3):
        y2 = y + 0.01 * variant
        P2 = P.copy()
        P2[:, :-1 if prog.has_shift else None] *= 1.0 + 0.02 * variant                   # (delta stays what it is)
        j2 = jit * (1.0 + 0.1 * variant)
        yd.copy_(torch.from_numpy(y2)); Pd.copy_(torch.from_numpy(P2)); jd.copy_(torch.from_numpy(j2))
        g.replay()
        torch.cuda.synchronize()
        got = [ll_g.clone(), flag_g.clone()] + [o.clone() for o in out_g]
        ll_e, out_e, flag_e = ops.loglik_kernel_grad(prog, Pd, xd, yed, jd, md, yd)      # eager, fresh buffers, same inputs
        assert int(flag_e.abs().sum()) == 0
        for a, b in zip(got, [ll_e, flag_e] + list(out_e)):
            assert torch.equal(a, b)
        for b in (0, 63, 64, 69):     # ... and the right answer
            want = exact_series(expr, P2[b], x[b], ye[b], j2[b], mean[b], y2[b])
            close(got[0][b:b + 1], np.array([want[0]]))
            keep = np.arange(P.shape[1]) != (prog.operations[-1]["col"] if prog.has_shift else -1)
            close(got[2][b][torch.from_numpy(keep).cuda()], want[1][keep], key="e2e")
            close(got[3][b:b + 1], np.array([want[2]]), key="e2e")
            close(got[4][b:b + 1], np.array([want[3]]), key="e2e")


# ---- 9. the frontend -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["prod_sho_real", "conv_sum"])
def test_gaussian_process_tensor_kernel_float_kernel_and_reference_predictions(ops, fixtures, name):
    import torch
    from celerite2_amd import gp as G, terms as T

    x, xs = fixtures["x"], fixtures["xs"]
    B = 3
    diag = np.repeat(fixtures["diag"][None], B, 0); y = np.repeat(fixtures["y"][None], B, 0)
    xd, xsd, dd, yd = dev(x, xs, diag, y)
    kf = A.build_cases(T, float)[name]()
    kt = tensor_kernel(name)
    gf = G.GaussianProcess(kf, xd, diag=dd)
    gt = G.GaussianProcess(kt, xd, diag=dd)
    same = lambda a, b, tol=1e-13: float((a - b).abs().max()) <= tol * float(b.abs().max())
    for u, v, nm in ((gt._a, gf._a, "a"), (gt._U, gf._U, "U"), (gt._V, gf._V, "V"), (gt._c, gf._c, "c")):
        assert same(u, v), nm
    kap = 1.0 if name == "prod_sho_real" else 2.0 / (0.4 * A.DELTA) ** 2
    for got, nm in ((gf._a, "a"), (gf._U, "U"), (gf._V, "V")):               # ... and both are the reference's matrices
        want = fixtures["%s_%s" % (name, nm)]
        assert np.max(np.abs(host(got)[0] - want)) <= 1e-13 * kap * np.max(np.abs(want)), nm
    want_ll = float(fixtures[name + "_loglik"])
    for gp_ in (gf, gt):
        assert abs(float(gp_.log_likelihood(yd)[0]) - want_ll) <= 1e-10 * abs(want_ll)
        mu, var = gp_.predict(yd, t=xsd, return_var=True)
        for got, want, nm in ((mu, fixtures[name + "_mu"], "mu"), (var, fixtures[name + "_var"], "var")):
            err = np.max(np.abs(host(got) - want[None])) / np.max(np.abs(want))
            print("%s %s: err %.2e" % (name, nm, err))
            assert err <= 1e-10, (nm, err)
    ll = gt.log_likelihood_kernel(yd)
    assert abs(float(ll[0]) - want_ll) <= 1e-10 * abs(want_ll)
    # the piecewise kernel on the device: k(0) and lags inside the boxcar, as the reference's get_value has them
    lags = dev(np.repeat(fixtures[name + "_lags"][None], B, 0))[0]
    for k in (kf, kt):
        got = host(k.get_value_device(lags))[0]
        want = fixtures[name + "_value"]
        assert np.max(np.abs(got - want)) <= 1e-13 * kap * np.max(np.abs(want))
        Kg = host(k.get_value_grid(xd, xd, B=B))[0] + np.diag(fixtures["diag"])
        assert np.max(np.abs(Kg - fixtures[name + "_K"])) <= 1e-13 * kap * np.max(np.abs(fixtures[name + "_K"]))
    psd = host(kt.get_psd(fixtures["omega"]))
    assert np.max(np.abs(psd[0] - fixtures[name + "_psd"])) <= 1e-13 * kap * np.max(fixtures[name + "_psd"])


def test_done_when_example(ops):
    """The two sentences of the feature: parameters -> ll and all gradients without a host round trip, for a quasi-periodic
    product and for an exposure-time convolution (whose diagonal shift is differentiated)."""
    import torch
    from celerite2_amd import autograd as ag, terms as T

    rng = np.random.default_rng(5)
    B, N = 6, 120
    x = gaps_x(rng, 1, N)[0]
    y = np.sin(x)[None] + 0.1 * rng.standard_normal((B, N))
    xd, yd = dev(x, y)
    yerr = torch.full((B, N), 0.3, dtype=torch.float64, device="cuda")
    p = lambda lo, hi: torch.tensor(rng.uniform(lo, hi, B), device="cuda", requires_grad=True)
    s, r, q, c = p(0.8, 1.5), p(2.0, 4.0), p(1.0, 4.0), p(0.05, 0.3)
    kernel = T.SHOTerm(sigma=s, rho=r, Q=q, regime="under") * T.RealTerm(a=1.0, c=c)
    for k in (kernel, T.TermConvolution(kernel, 0.05)):
        for t in (s, r, q, c):
            t.grad = None
        ll = ag.log_likelihood_kernel(k, xd, yd, yerr=yerr)
        ll.sum().backward()
        assert bool(torch.isfinite(ll).all()) and all(bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().min()) > 0 for t in (s, r, q, c))


def test_worst_case_report():
    """Not a check: prints the worst |error| / allowed over this module's gradient comparisons (1.0 = at the criterion)."""
    print("worst |err| / (1e-10 |exact| + 1e-12 max|exact|): term_coefficients_rev %.3g, end to end %.3g" % (WORST["rev"], WORST["e2e"]))
