# -*- coding: utf-8 -*-
"""Term hyper-parameters on the device (csrc/c2_term_params.hip, ops.term_coefficients[_rev], ops.noise_mean_*,
ops.loglik_kernel_grad, autograd.log_likelihood_kernel, tensor parameters in terms.py) against

  * the coefficients the REFERENCE's term classes produced (tests/golden/ref_golden.npz) and the numpy restatement of
    tests/term_params_ref.py (pinned to them by tests/test_term_params.py): 1e-13 of each series' largest entry per array;
  * the exact complex-step Jacobian of that restatement, and end to end oracle.exact.cstep_grad of the DENSE log-likelihood
    of restatement(P), yerr^2 + jitter^2, y - mean w.r.t. P, jitter, mean: the standing criterion for device gradients,
    1e-10 relative + a floor of 1e-12 of the largest entry (tests/test_gpu_exact_gradients.py).

Lengths N = 1, 2, 33, 150 all run (ops.loglik_terms_grad takes every one of them)."""
import numpy as np
import pytest

import term_params_ref as R
from oracle import exact

pytestmark = pytest.mark.gpu
GOLDEN_CASES = R.GOLDEN_CASES
CN = ("ar", "cr", "ac", "bc", "cc", "dc")
S, RH, TA = R.SIGMA, R.RHO, R.TAU
WORST = {"rev": 0.0, "e2e": 0.0}


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
    return x.detach().cpu().numpy()


def close(a, b, tol=1e-10, floor=1e-12, what=None, key=None):
    a = host(a) if hasattr(a, "cpu") else np.asarray(a)
    b = np.asarray(b)
    if key is not None and b.size:
        WORST[key] = max(WORST[key], float(np.max(np.abs(a - b) / (tol * np.abs(b) + floor * max(1.0, float(np.abs(b).max()))))))
    np.testing.assert_allclose(a, b, rtol=tol, atol=floor * max(1.0, float(np.abs(b).max())), err_msg=str(what))


def force(monkeypatch, which):
    """The lane mappings of c2_loglik_terms[_grad], as tests/test_gpu_terms.py forces them; "default": the dispatch's own."""
    if which == "default":
        return
    monkeypatch.setenv("C2_TERMS_FUSED", "1" if which == "one" else "0")
    monkeypatch.setenv("C2_TERMS_TWO_LANES", "1" if which == "two" else "0")
    monkeypatch.setenv("C2_TERMS_EIGHT_LANES", "1" if which == "eight" else "0")
    monkeypatch.setenv("C2_TERMS_FOUR_LANES", "1" if which == "four" else "0")


def program_of(ops, records, NP):
    return ops.TermProgram([dict(r, cols=tuple(r["cols"])) for r in records], NP)


# ---- cases: (records, P) and the same model as a terms.py kernel over the columns of a leaf tensor -----------------------
SHO_NAMES = {0: ("S0", "w0", "Q"), S | RH | TA: ("sigma", "rho", "tau"), S | RH: ("sigma", "rho", "Q")}


def make_case(name, rng, B):
    """name -> (records, P (B, NP), build(cols) -> terms kernel)."""
    from celerite2_amd import terms as T

    if name.startswith("sho/"):
        _, par, regime = name.split("/")
        par = int(par)
        recs, P = R.draw("sho", rng, B, par=par, regime=regime)
        return recs, P, lambda c: T.SHOTerm(**dict(zip(SHO_NAMES[par], c)), regime=regime)
    if name == "matern32":
        recs, P = R.draw("matern32", rng, B)
        return recs, P, lambda c: T.Matern32Term(sigma=c[0], rho=c[1])
    if name == "rotation":
        recs, P = R.draw("rotation", rng, B)
        return recs, P, lambda c: T.RotationTerm(sigma=c[0], period=c[1], Q0=c[2], dQ=c[3], f=c[4])
    if name == "sum":   # SHO + Real + Matern32: width 5
        _, Ps = R.draw("sho", rng, B, regime="under")
        _, Pr = R.draw("real", rng, B)
        _, Pm = R.draw("matern32", rng, B)
        recs = [R.rec("sho", (0, 1, 2), regime="under"), R.rec("real", (3, 4)), R.rec("matern32", (5, 6))]
        return recs, np.concatenate([Ps, Pr, Pm], 1), lambda c: (T.SHOTerm(S0=c[0], w0=c[1], Q=c[2], regime="under")
                                                                   + T.RealTerm(a=c[3], c=c[4]) + T.Matern32Term(sigma=c[5], rho=c[6]))
    assert name == "sho4"   # four under-damped oscillators: width 8, every lane mapping
    parts = [R.draw("sho", rng, B, regime="under")[1] for _ in range(4)]
    recs = [R.rec("sho", (3 * k, 3 * k + 1, 3 * k + 2), regime="under") for k in range(4)]

    def build(c):
        k = T.SHOTerm(S0=c[0], w0=c[1], Q=c[2], regime="under")
        for i in range(1, 4):
            k = k + T.SHOTerm(S0=c[3 * i], w0=c[3 * i + 1], Q=c[3 * i + 2], regime="under")
        return k
    return recs, np.concatenate(parts, 1), build


KIND_DRAWS = ([("real", 0, None), ("complex", 0, None), ("matern32", 0, None), ("rotation", 0, None)]
              + [("sho", par, regime) for par in (0, S, RH, TA, S | RH, S | TA, RH | TA, S | RH | TA)
                 for regime in ("under", "over", "mixed")])


# ---- coefficients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_coefficients_vs_reference_sets(ops, golden, name):
    recs, P = GOLDEN_CASES[name]
    prog = program_of(ops, recs, len(P))
    (Pd,) = dev(np.array(P))
    for Pin, B in ((Pd, 3), (Pd[None].repeat(3, 1).contiguous(), None)):   # shared (NP,) and per-series (B, NP)
        co, flag = ops.term_coefficients(prog, Pin, B)
        assert int(flag.abs().sum()) == 0
        for cn, g in zip(CN, co):
            want = golden["coef_%s_%s" % (name, cn)]
            assert tuple(g.shape) == (3,) + want.shape
            if want.size:
                assert np.max(np.abs(host(g) - want[None])) <= 1e-13 * np.max(np.abs(want)), (name, cn)


@pytest.mark.parametrize("kind,par,regime", KIND_DRAWS)
def test_coefficients_and_reverse_vs_restatement(ops, kind, par, regime):
    """4096 seeded per-series draws per kind and parameterisation: coefficients to 1e-13 of each series' largest entry per
    array, flag == 0; the reverse against the complex-step Jacobian of the restatement (random cotangents)."""
    rng = np.random.default_rng(4096 + 31 * par + len(kind) + len(regime or ""))
    B = 4096
    recs, P = R.draw(kind, rng, B, par=par, regime=regime)
    prog = program_of(ops, recs, P.shape[1])
    (Pd,) = dev(P)
    co, flag = ops.term_coefficients(prog, Pd)
    assert int(flag.abs().sum()) == 0
    want = R.coefficients(recs, P)
    for cn, g, w in zip(CN, co, want):
        if w.size:
            top = np.max(np.abs(w), axis=1, keepdims=True)      # (a mixed term's inactive amplitudes: an all-zero row, exact)
            err = np.max(np.abs(host(g) - w) / np.where(top == 0.0, 1.0, top))
            assert err <= 1e-13, (cn, err)
    cots = R.zero_inactive_rate_cotangents(recs, P, [rng.standard_normal(w.shape) for w in want])
    bP = ops.term_coefficients_rev(prog, Pd, dev(*cots))
    exactJ = np.empty_like(P)
    for k in range(P.shape[1]):
        d = np.zeros(P.shape[1]); d[k] = 1.0
        exactJ[:, k] = np.imag(sum(np.sum(g * c, axis=-1) for g, c in zip(cots, R.coefficients(recs, P + 1j * exact.H * d)))) / exact.H
    got = host(bP)
    # per series: 1e-10 relative + 1e-12 of the series' largest entry
    tol = 1e-10 * np.abs(exactJ) + 1e-12 * np.maximum(1.0, np.max(np.abs(exactJ), axis=1, keepdims=True))
    ratio = float(np.max(np.abs(got - exactJ) / tol))
    WORST["rev"] = max(WORST["rev"], ratio)
    print("term_coefficients_rev %s par=%d %s: worst |err| / allowed = %.3g" % (kind, par, regime, ratio))
    assert ratio <= 1.0, ratio
    # and against the numpy reverse it restates
    close(bP, R.coefficients_rev(recs, P, cots), tol=1e-10, floor=1e-12)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def exact_series(recs, Pb, xb, yeb, jb, mb, yb):
    """(ll, bP, bjitter, bmean) of ONE series: complex step of the dense log-likelihood of the restatement."""
    def f(P, j, m):
        return exact.terms_loglik_fwd(*R.coefficients(recs, P), xb[None], yeb[None] ** 2 + j[:, None] ** 2, yb[None] - m[:, None])

    ll = float(np.real(f(Pb[None].astype(complex), np.array([jb + 0j]), np.array([mb + 0j])))[0])
    g = exact.cstep_grad(f, [Pb, jb, mb])
    return ll, g[0], float(g[1]), float(g[2])


def run_e2e(ops, name, N, lanes, monkeypatch, B, seed):
    import torch
    from celerite2_amd import autograd as ag

    rng = np.random.default_rng(seed)
    recs, P, build = make_case(name, rng, B)
    x = np.sort(rng.uniform(0, max(N, 2) / 10.0, (B, N)), axis=1)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    jit = rng.uniform(0.05, 0.4, B)
    mean = rng.uniform(-0.3, 0.3, B)
    force(monkeypatch, lanes)
    xd, yed, yd = dev(x, ye, y)
    # per-series P, x, jitter, mean
    Pt, jt, mt = [t.requires_grad_() for t in dev(P, jit, mean)]
    kernel = build([Pt[:, k] for k in range(P.shape[1])])
    ll = ag.log_likelihood_kernel(kernel, xd, yd, yerr=yed, jitter=jt, mean=mt)
    ll.sum().backward()
    want = [exact_series(recs, P[b], x[b], ye[b], jit[b], mean[b], y[b]) for b in range(B)]
    close(ll, np.array([w[0] for w in want]), what=(name, "ll"))
    close(Pt.grad, np.stack([w[1] for w in want]), what=(name, "bP"), key="e2e")
    close(jt.grad, np.array([w[2] for w in want]), what=(name, "bjitter"), key="e2e")
    close(mt.grad, np.array([w[3] for w in want]), what=(name, "bmean"), key="e2e")
    # shared P (0-d parameters), shared x, shared jitter and mean: the batch sums
    Ps, js, ms = [t.requires_grad_() for t in dev(P[0], jit[0], mean[0])]
    kernel = build([Ps[k] for k in range(P.shape[1])])
    ll = ag.log_likelihood_kernel(kernel, xd[0].contiguous(), yd, yerr=yed, jitter=js, mean=ms)
    ll.sum().backward()
    want = [exact_series(recs, P[0], x[0], ye[b], jit[0], mean[0], y[b]) for b in range(B)]
    close(ll, np.array([w[0] for w in want]), what=(name, "ll shared"))
    close(Ps.grad, np.sum([w[1] for w in want], axis=0), what=(name, "bP shared"), key="e2e")
    close(js.grad, np.sum([w[2] for w in want]), what=(name, "bjitter shared"), key="e2e")
    close(ms.grad, np.sum([w[3] for w in want]), what=(name, "bmean shared"), key="e2e")


NARROW = ["sho/%d/%s" % (par, regime) for par in sorted(SHO_NAMES) for regime in ("under", "over", "mixed")] + ["matern32", "rotation"]


@pytest.mark.parametrize("N", [1, 2, 33, 150])
@pytest.mark.parametrize("lanes", ["composed", "one", "eight"])
@pytest.mark.parametrize("name", NARROW)
def test_end_to_end_exact_widths_two_and_four(ops, monkeypatch, name, lanes, N):
    run_e2e(ops, name, N, lanes, monkeypatch, B=70 if N == 150 else 5, seed=N + len(name))


@pytest.mark.parametrize("N", [1, 2, 33, 150])
@pytest.mark.parametrize("lanes", ["composed", "one", "two", "four", "eight"])
def test_end_to_end_exact_width_eight(ops, monkeypatch, lanes, N):
    run_e2e(ops, "sho4", N, lanes, monkeypatch, B=70 if N == 150 else 5, seed=800 + N)


@pytest.mark.parametrize("N", [1, 2, 33, 150])
def test_end_to_end_exact_sum_width_five(ops, monkeypatch, N):
    run_e2e(ops, "sum", N, "default", monkeypatch, B=70 if N == 150 else 5, seed=500 + N)


def test_rotation_loglik_vs_reference(ops, golden):
    """The reference's own number: its GaussianProcess log-likelihood of RotationTerm(1.5, 3.45, 1.3, 1.05, 0.5)."""
    import torch
    from celerite2_amd import autograd as ag, terms as T

    p = [torch.tensor(v, dtype=torch.float64, device="cuda") for v in (1.5, 3.45, 1.3, 1.05, 0.5)]
    kernel = T.RotationTerm(sigma=p[0], period=p[1], Q0=p[2], dQ=p[3], f=p[4])
    x, diag, y = dev(golden["gprot_x"], golden["gprot_diag"][None], golden["gprot_y"][None])
    ll = ag.log_likelihood_kernel(kernel, x, y, diag=diag, mean=float(golden["gprot_mean"]))
    want = float(golden["gprot_loglik"])
    assert abs(float(ll[0]) - want) <= 1e-10 * abs(want), (float(ll[0]), want)


# ---- the mixed regime ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("par", sorted(SHO_NAMES))
def test_mixed_agrees_with_under_and_over_on_its_halves(ops, par):
    import torch
    from celerite2_amd import autograd as ag, terms as T

    rng = np.random.default_rng(60 + par)
    B, N = 64, 120
    recs, P = R.draw("sho", rng, B, par=par, regime="mixed")
    Q = R._sho_params(par, P[:, 0], P[:, 1], P[:, 2])[2]
    assert np.sum(Q < 0.5) == B // 2 and np.min(np.abs(Q - 0.5)) > 0.01
    x = np.sort(rng.uniform(0, N / 10.0, (B, N)), axis=1)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))

    def run(idx, regime):
        Pt = dev(P[idx])[0].requires_grad_()
        k = T.SHOTerm(**dict(zip(SHO_NAMES[par], [Pt[:, i] for i in range(3)])), regime=regime)
        ll = ag.log_likelihood_kernel(k, *dev(x[idx], y[idx]), yerr=dev(ye[idx])[0])
        ll.sum().backward()
        return host(ll), host(Pt.grad)

    ll_m, g_m = run(np.arange(B), "mixed")
    for idx, regime in ((np.where(Q >= 0.5)[0], "under"), (np.where(Q < 0.5)[0], "over")):
        ll_h, g_h = run(idx, regime)
        for b, l, g in zip(idx, ll_h, g_h):   # series by series
            close(ll_m[b:b + 1], np.array([l]), what=("ll", b))
            close(g_m[b], g, what=("bP", b))
    want = [exact_series(recs, P[b], x[b], ye[b], 0.0, 0.0, y[b]) for b in range(B)]
    close(ll_m, np.array([w[0] for w in want]))
    close(g_m, np.stack([w[1] for w in want]), key="e2e")
    # the inactive slots' amplitude cotangents may be anything finite: they contribute exactly nothing to bP
    prog = program_of(ops, recs, 3)
    (Pd,) = dev(P)
    co = R.coefficients(recs, P)
    cots = R.zero_inactive_rate_cotangents(recs, P, [rng.standard_normal(c.shape) for c in co])
    a = ops.term_coefficients_rev(prog, Pd, dev(*cots))
    over = Q < 0.5
    cots2 = [c.copy() for c in cots]
    cots2[0][~over] = 1e30 * rng.standard_normal((int(np.sum(~over)), 2))
    cots2[2][over] = -1e30; cots2[3][over] = 1e30
    b2 = ops.term_coefficients_rev(prog, Pd, dev(*cots2))
    assert torch.equal(a, b2)


def test_wrong_side_series_is_flagged_on_the_device(ops):
    import torch
    from celerite2_amd import autograd as ag, terms as T

    rng = np.random.default_rng(8)
    B, N, bad = 70, 100, 17
    recs, P = R.draw("sho", rng, B, regime="under")
    x = np.sort(rng.uniform(0, N / 10.0, (B, N)), axis=1)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    jit = rng.uniform(0.05, 0.4, B)
    xd, yed, yd = dev(x, ye, y)

    def run(Pn):
        Pt, jt = [t.requires_grad_() for t in dev(Pn, jit)]
        k = T.SHOTerm(S0=Pt[:, 0], w0=Pt[:, 1], Q=Pt[:, 2], regime="under")
        ll = ag.log_likelihood_kernel(k, xd, yd, yerr=yed, jitter=jt)
        ll.sum().backward()
        return ll.detach(), Pt.grad, jt.grad

    good = run(P)
    P2 = P.copy(); P2[bad, 2] = 0.3     # over-damped under regime="under"
    ll, gP, gj = run(P2)
    assert float(ll[bad]) == -np.inf and float(gP[bad].abs().sum()) == 0.0 and float(gj[bad]) == 0.0
    keep = np.arange(B) != bad
    for a, b in zip((ll, gP, gj), good):     # every other series: bit-identical to the run where that series is on the right side
        assert torch.equal(a[keep], b[keep])
    prog = program_of(ops, recs, 3)
    _, flag = ops.term_coefficients(prog, dev(P2)[0])
    assert int(flag[bad]) != 0 and int(flag.abs().sum()) == abs(int(flag[bad]))
    out = ops.loglik_kernel_grad(prog, dev(P2)[0], xd, yed, dev(jit)[0], None, yd)
    assert int(out[2][bad]) == -2 and float(out[0][bad]) == -np.inf and int(out[2].abs().sum()) == 2


# ---- no host traffic: the whole chain in one captured graph ----------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["composed", "one", "two", "four", "eight"])
def test_loglik_kernel_grad_is_graph_capturable(ops, monkeypatch, lanes):
    import torch

    rng = np.random.default_rng(91)
    B, N = 70, 150
    recs, P, _ = make_case("sho4", rng, B)
    prog = program_of(ops, recs, P.shape[1])
    x = np.sort(rng.uniform(0, N * 0.02, (B, N)), axis=1)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    jit = rng.uniform(0.05, 0.4, B); mean = rng.uniform(-0.3, 0.3, B)
    force(monkeypatch, lanes)
    Pd, xd, yed, jd, md, yd = dev(P, x, ye, jit, mean, y)
    work = ops.loglik_kernel_workspace(prog, B, N, Pd.device)
    ll, out, flag = ops.loglik_kernel_grad(prog, Pd, xd, yed, jd, md, yd, work=work)     # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ll_g, out_g, flag_g = ops.loglik_kernel_grad(prog, Pd, xd, yed, jd, md, yd, work=work, out=out)
    for variant in range(3):
        y2 = y + 0.01 * variant
        P2 = P * (1.0 + 0.02 * variant)
        j2 = jit * (1.0 + 0.1 * variant)
        x2 = x.copy()
        if variant == 2:
            x2[:64, N // 2:] += 500.0      # beyond the backward guard for the first group: the composed chain answers there
        yd.copy_(torch.from_numpy(y2)); Pd.copy_(torch.from_numpy(P2)); jd.copy_(torch.from_numpy(j2)); xd.copy_(torch.from_numpy(x2))
        g.replay()
        torch.cuda.synchronize()
        got = [ll_g.clone(), flag_g.clone()] + [o.clone() for o in out_g]
        ll_e, out_e, flag_e = ops.loglik_kernel_grad(prog, Pd, xd, yed, jd, md, yd)      # eager, fresh buffers, same inputs
        assert int(flag_e.abs().sum()) == 0
        for a, b in zip(got, [ll_e, flag_e] + list(out_e)):
            assert torch.equal(a, b)
        for b in (0, 63, 64, 69):     # ... and the right answer
            want = exact_series(recs, P2[b], x2[b], ye[b], j2[b], mean[b], y2[b])
            close(got[0][b:b + 1], np.array([want[0]]))
            close(got[2][b], want[1], key="e2e")
            close(got[3][b:b + 1], np.array([want[2]]), key="e2e")
            close(got[4][b:b + 1], np.array([want[3]]), key="e2e")


# ---- jitter and mean ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(70000, 1), (70000, 2), (3, 4097), (5, 1024), (257, 33)])
def test_noise_mean_kernels(ops, B, N):
    import torch

    rng = np.random.default_rng(B + N)
    ye, y, bd, by = (rng.standard_normal((B, N)) for _ in range(4))
    jit, mean = rng.uniform(0.1, 1, B), rng.standard_normal(B)
    yed, yd, bdd, byd, jd, md = dev(ye, y, bd, by, jit, mean)
    diag, r = ops.noise_mean_apply(yed, jd, md, yd)
    # r is ONE rounded subtraction: the same bits as numpy.  diag is two squares and a sum of positive numbers, each rounded
    # once in numpy (<= 3 * 2^-53 relative), fewer roundings where the device contracts them into a fused multiply-add: the
    # two differ by at most 4 * 2^-53 relative
    want = ye**2 + jit[:, None] ** 2
    assert np.max(np.abs(host(diag) - want) / want) <= 4 * 2.0**-53 and np.array_equal(host(r), y - mean[:, None])
    diag, r = ops.noise_mean_apply(yed, None, None, yd, yerr_is_sigma=False)
    assert np.array_equal(host(diag), ye) and np.array_equal(host(r), y)
    bj, bm = ops.noise_mean_rev(jd, bdd, byd)
    bj2, bm2 = ops.noise_mean_rev(jd, bdd, byd)
    assert torch.equal(bj, bj2) and torch.equal(bm, bm2)      # a fixed summation order: identical bits
    scale = np.abs(bd).sum(1)
    assert np.max(np.abs(host(bj) - 2 * jit * bd.sum(1)) / (2 * jit * scale)) <= 1e-14
    assert np.max(np.abs(host(bm) + by.sum(1)) / np.abs(by).sum(1)) <= 1e-14
    flag = torch.zeros(B, dtype=torch.int32, device="cuda"); flag[1] = 7
    bj3, bm3 = ops.noise_mean_rev(jd, bdd, byd, flag=flag)
    assert float(bj3[1]) == 0.0 and float(bm3[1]) == 0.0 and torch.equal(bj3[2:], bj[2:]) and float(bj3[0]) == float(bj[0])
    with pytest.raises(ValueError, match="Invalid shape: yerr"):
        ops.noise_mean_apply(yed[:, : N - 1].contiguous() if N > 1 else yed[:1], jd, md, yd)
    with pytest.raises(ValueError, match="Invalid shape: jitter"):
        ops.noise_mean_rev(jd[:2].contiguous(), bdd, byd)


# ---- the frontend ------------------------------------------------------------------------------------------------------------
def test_gaussian_process_with_tensor_kernel_equals_float_kernel(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    rng = np.random.default_rng(12)
    B, N, M = 3, 80, 50
    x = np.sort(rng.uniform(0, 10, N)); ts = np.sort(rng.uniform(-1, 12, M))
    diag = rng.uniform(0.1, 0.3, (B, N)); y = np.sin(x)[None] + 0.1 * rng.standard_normal((B, N))
    xd, tsd, dd, yd = dev(x, ts, diag, y)
    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kf = T.SHOTerm(S0=5.0, w0=0.1, Q=3.45) + T.RealTerm(a=1.0, c=0.1) + T.Matern32Term(sigma=0.5, rho=2.0) + T.SHOTerm(sigma=0.7, rho=1.1, Q=0.3)
    kt = (T.SHOTerm(S0=t(5.0), w0=t(0.1), Q=t(3.45), regime="under") + T.RealTerm(a=t(1.0), c=0.1)
          + T.Matern32Term(sigma=t(0.5), rho=t(2.0)) + T.SHOTerm(sigma=t(0.7), rho=t(1.1), Q=0.3))
    assert kt.width == kf.width == 7
    gf = G.GaussianProcess(kf, xd, diag=dd, mean=0.3)
    gt = G.GaussianProcess(kt, xd, diag=dd, mean=0.3)
    assert "_dev_cache" in kf.__dict__ and "_dev_cache" not in kt.__dict__     # floats: _dev_coefs is still the path taken
    same = lambda a, b: float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    assert same(gt.log_likelihood(yd), gf.log_likelihood(yd))
    for kw in (dict(), dict(t=tsd, return_var=True), dict(t=tsd, return_cov=True)):
        a, b = gt.predict(yd, **kw), gf.predict(yd, **kw)
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert same(u, v), kw
    # ... and its differentiable log-likelihood is the fused one
    ll = gt.log_likelihood_kernel(yd)
    assert float((ll - gf.log_likelihood(yd)).abs().max()) <= 1e-10 * float(ll.abs().max())
    with pytest.raises(TypeError, match="tensor parameters"):
        kt.get_coefficients()
    with pytest.raises(ValueError, match="regime"):
        T.SHOTerm(S0=1.0, w0=1.0, Q=t(1.0))


def test_worst_case_report():
    """Not a check: prints the worst |error| / allowed over this module's gradient comparisons (1.0 = at the criterion)."""
    print("worst |err| / (1e-10 |exact| + 1e-12 max|exact|): term_coefficients_rev %.3g, end to end %.3g" % (WORST["rev"], WORST["e2e"]))
