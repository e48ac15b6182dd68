# -*- coding: utf-8 -*-
"""GPU checks of the variance at new times in linear time: ops.explained_variance (c2_explained_variance,
csrc/c2_predvar.hip) at every width up to 32, and GaussianProcess.predict_at on top of it.

References: the numpy restatement of the two-state recurrence (tests/predict_at_ref.py, pinned to dense algebra by
tests/test_predict_at.py) fed the device's own d, W; up to 150 rows dense algebra itself; the reference's own
predictive variances (tests/golden/ref_golden.npz); and the existing predict(y, t, return_var=True).  Criterion: the
standing one on the variance, |x - x_o| <= 1e-10 |x_o| + 1e-12 k(0).  Every dense input has a condition number <= 1e6,
asserted per draw."""
import numpy as np
import pytest

import predict_at_ref as P

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
SIZES_N = [1, 2, 16, 17, 33, 150]      # one row, the 16-row stream block of the sibling sweeps and its neighbours
SIZES_M = [1, 15, 16, 17, 150]
KINDS = ["mixed", "before", "after", "equal", "dups", "cluster"]


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


def make_queries(kind, t, M, rng):
    """M sorted query times relative to the data grid t."""
    N = len(t)
    if kind == "before":
        return np.sort(t[0] - rng.uniform(1e-3, 3.0, M))
    if kind == "after":
        return np.sort(t[-1] + rng.uniform(1e-3, 3.0, M))
    if kind == "equal":     # data times only (repeats as soon as M > N)
        return np.sort(t[rng.integers(0, N, M)])
    if kind == "cluster":   # every query in ONE gap: all the other gaps are empty
        if N == 1:
            return np.sort(t[0] + rng.uniform(0.0, 0.5, M))
        k = N // 2 - 1 if N > 1 else 0
        return np.sort(t[k] + (t[k + 1] - t[k]) * rng.uniform(0.0, 1.0, M))
    ts = P.queries(t, rng, M)
    if kind == "dups":
        ts[1::2] = ts[:-1:2][:len(ts[1::2])]
    return np.sort(ts)


def batch(seed, B, N, M, J, *, per_t, per_ts, kind="mixed", gap=False, distinct=5):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct); data and query grids each either the
    first draw's, shared by the batch, or every draw's own."""
    rng = np.random.default_rng(seed)
    draws = []
    for k in range(min(B, distinct)):
        t = None if (per_t or k == 0) else draws[0]["t"]
        if t is None:
            t = P.draw(1000 * seed + k, N, J, gap=gap)["t"]
        ts = make_queries(kind, t, M, rng) if (per_ts or k == 0) else draws[0]["ts"]
        draws.append(P.draw_with_queries(1000 * seed + k, N, J, t=t, ts=ts))
    idx = [b % len(draws) for b in range(B)]
    stack = lambda key: np.stack([draws[i][key] for i in idx])
    return dict(draws=draws, idx=idx, t=stack("t") if per_t else draws[0]["t"], ts=stack("ts") if per_ts else draws[0]["ts"],
                c=stack("c"), a=stack("a"), U=stack("U"), V=stack("V"), Us=stack("Us"), Vs=stack("Vs"))


def run_case(ops, bt, *, dense, what):
    """ops.explained_variance against the restatement fed the SAME d, W (the device's factorisation) and, if `dense`,
    against dense algebra for every distinct draw; repeats of a draw give identical bits."""
    import torch

    B = bt["a"].shape[0]
    t, ts, c, a, U, V, Us, Vs = dev(bt["t"], bt["ts"], bt["c"], bt["a"], bt["U"], bt["V"], bt["Us"], bt["Vs"])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0, what
    r = ops.explained_variance(t, ts, c, U, W, d, Us, Vs)
    torch.cuda.synchronize()
    assert tuple(r.shape) == (B, bt["Us"].shape[1])
    dh, Wh, rh = host(d), host(W), host(r)
    seen = set()
    for b in range(B):
        k = bt["idx"][b]
        if k in seen:   # a repeat of a draw already compared: identical inputs give identical bits
            assert torch.equal(r[b], r[bt["idx"].index(k)]), (what, b)
            continue
        seen.add(k)
        dr = bt["draws"][k]
        k0 = dr["k0"]
        ro = P.explained_variance(dr["t"], dr["ts"], dr["c"], dr["U"], Wh[b], dh[b], dr["Us"], dr["Vs"])
        e = P.err(k0 - rh[b], k0 - ro, floor=k0)
        assert e <= 1.0, (what, b, "restatement", e)
        if dense:
            cond = np.linalg.cond(P.dense(dr["t"], dr["c"], dr["a"], dr["U"], dr["V"]))
            assert cond <= 1e6, (what, b, cond)
            rd = P.dense_explained(dr["t"], dr["ts"], dr["c"], dr["a"], dr["U"], dr["V"], dr["Us"], dr["Vs"])
            e = P.err(k0 - rh[b], k0 - rd, floor=k0)
            assert e <= 1.0, (what, b, "dense", e)


@pytest.mark.parametrize("J", WIDTHS)
def test_explained_variance_vs_restatement_and_dense(ops, J):
    """Every width; every pair of N in {1, 2, 16, 17, 33, 150} and M in {1, 15, 16, 17, 150}; B = 3 and 70 (a padded last
    wavefront); the four combinations of shared and per-series t and ts, and the six kinds of query set (mixed with the
    exact data times t_0, t_{N/2}, t_{N-1}; all before t_0; all after t_{N-1}; data times only; duplicates; all in one gap)
    cycling over the pairs; one draw with the 50-unit gap."""
    n = 0
    for i, N in enumerate(SIZES_N):
        for k, M in enumerate(SIZES_M):
            B = (3, 70)[(i + k) % 2]
            per_t, per_ts = bool(n & 1), bool(n & 2)
            kind = KINDS[(n + J) % len(KINDS)]
            bt = batch(100 * J + n, B, N, M, J, per_t=per_t, per_ts=per_ts, kind=kind)
            run_case(ops, bt, dense=True, what=(J, N, M, B, per_t, per_ts, kind))
            n += 1
    bt = batch(100 * J + 99, 3, 150, 150, J, per_t=True, per_ts=True, gap=True)
    run_case(ops, bt, dense=True, what=(J, "gap"))


@pytest.mark.parametrize("J", [8, 32])
def test_explained_variance_long_series(ops, J):
    """N = 4096 with M = 4097, and N = 4097 with M = 256, against the restatement."""
    for N, M, per in ((4096, 4097, True), (4097, 256, False)):
        bt = batch(77 + J, 2, N, M, J, per_t=per, per_ts=not per, distinct=2)
        run_case(ops, bt, dense=False, what=(J, N, M))


def _close(a, b, tol, floor):   # the comparison of tests/test_reference_fixtures.py
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    np.testing.assert_allclose(a, b, rtol=tol, atol=floor * max(1.0, float(np.abs(b).max())))


def test_predict_at_vs_reference_numbers(ops, golden):
    """predict_at against what the REFERENCE's ConditionalDistribution returned (tests/golden/ref_golden.npz): the batch of
    three series gp0_/gp1_/gp2_ (per-series S0, J = 5) and the RotationTerm series gprot_ (J = 4, N = 120, M = 300); kernels
    and tolerances as tests/test_reference_fixtures.py (variance 1e-9, 1e-11; mean 1e-10, 1e-11)."""
    from celerite2_amd import gp as gpmod, terms

    B = 3
    g = [{k[4:]: v for k, v in golden.items() if k.startswith("gp%d_" % b)} for b in range(B)]
    st = lambda k: np.stack([g[b][k] for b in range(B)])
    kernel = (terms.SHOTerm(S0=np.array([5.0, 4.0, 3.0]), w0=0.1, Q=3.45) + terms.RealTerm(a=1.0, c=0.1)
              + terms.Matern32Term(sigma=0.5, rho=2.0))
    xd, dd, yd, tsd = dev(st("x"), st("diag"), st("y"), st("ts"))
    gp = gpmod.GaussianProcess(kernel, mean=0.3)
    gp.compute(xd, diag=dd)
    mu, var = gp.predict_at(yd, tsd, return_var=True)
    _close(var, st("var_star"), 1e-9, 1e-11)
    _close(mu, st("mu_star"), 1e-10, 1e-11)
    _close(gp.predict_at(yd, tsd, include_mean=False), st("mu_star_nomean"), 1e-10, 1e-11)

    g = {k[6:]: v for k, v in golden.items() if k.startswith("gprot_")}
    kernel = terms.RotationTerm(sigma=1.5, period=3.45, Q0=1.3, dQ=1.05, f=0.5)
    xd, dd, yd, tsd = dev(g["x"][None], g["diag"][None], g["y"][None], g["ts"][None])
    gp = gpmod.GaussianProcess(kernel, mean=0.0)
    gp.compute(xd, diag=dd)
    mu, var = gp.predict_at(yd, tsd, return_var=True)
    _close(var[0], g["var_star"], 1e-9, 1e-11)
    _close(mu[0], g["mu_star"], 1e-10, 1e-11)
    mu1, var1 = gp.predict_at(yd, tsd[0], return_var=True)   # the same grid given as (M,)
    _close(var1[0], g["var_star"], 1e-9, 1e-11)
    _close(mu1[0], g["mu_star"], 1e-10, 1e-11)


def _gp_inputs(seed, B, N):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 0.05 * N + 5, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.4, (B, N))
    y = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3
    return x, diag, y


def test_predict_at_equals_predict(ops):
    """8 x 512 with M = 700 (per-series query grids, some outside the data), host-float and tensor hyper-parameters, a tensor
    mean, include_mean both ways: mean and variance against the existing predict(y, t, return_var=True)."""
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N, M = 8, 512, 700
    x, diag, y = _gp_inputs(4, B, N)
    xs = np.sort(np.random.default_rng(5).uniform(x.min() - 1.0, x.max() + 1.0, (B, M)), axis=1)
    xd, dd, yd, xsd = dev(x, diag, y, xs)
    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kf = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3) + T.Matern32Term(sigma=0.5, rho=2.0)
    kt = (T.SHOTerm(S0=t(1.2), w0=t(0.9), Q=t(2.5), regime="under") + T.RealTerm(a=t(0.7), c=0.3)
          + T.Matern32Term(sigma=t(0.5), rho=t(2.0)))
    for kernel in (kf, kt):
        gp = G.GaussianProcess(kernel, xd, diag=dd, mean=t(0.3))
        k0 = gp.condition(yd, xsd)._k0()
        k0max = float(k0.max()) if torch.is_tensor(k0) else float(k0)
        for include_mean in (True, False):
            mu_o, var_o = gp.predict(yd, xsd, return_var=True, include_mean=include_mean)
            mu, var = gp.predict_at(yd, xsd, return_var=True, include_mean=include_mean)
            assert tuple(mu.shape) == tuple(var.shape) == (B, M)
            e = P.err(host(mu), host(mu_o))
            assert e <= 1.0, ("mean", include_mean, e)
            e = P.err(host(var), host(var_o), floor=k0max)
            assert e <= 1.0, ("variance", include_mean, e)
            assert bool((var > 0).all()) and bool((var <= k0).all())
            assert torch.equal(gp.predict_at(yd, xsd, include_mean=include_mean), mu)


def test_seventy_thousand_series(ops):
    """B = 70 000 x N = 16 x M = 8 x J = 4: runs, the results are finite, and the first and last series agree with the same
    series computed alone."""
    import torch

    B, N, M, J = 70000, 16, 8, 4
    rng = np.random.default_rng(8)
    base = P.draw_with_queries(8, N, J, M)
    scale = rng.uniform(0.5, 2.0, B)
    a = base["k0"] * scale[:, None] + base["diag"][None] * rng.uniform(0.5, 2.0, (B, 1))
    U, Us = base["U"][None] * scale[:, None, None], base["Us"][None] * scale[:, None, None]
    V, Vs = np.broadcast_to(base["V"][None], (B, N, J)), np.broadcast_to(base["Vs"][None], (B, M, J))
    t, ts, c, ad, Ud, Vd, Usd, Vsd = dev(base["t"], base["ts"], base["c"], a, U, V, Us, Vs)
    d, W, flag = ops.factor(t, c, ad, Ud, Vd)
    r = ops.explained_variance(t, ts, c, Ud, W, d, Usd, Vsd)
    torch.cuda.synchronize()
    assert int(flag.abs().sum()) == 0 and bool(torch.isfinite(r).all())
    for b in (0, B - 1):
        s = slice(b, b + 1)
        r1 = ops.explained_variance(t, ts, c, Ud[s].contiguous(), W[s].contiguous(), d[s].contiguous(), Usd[s].contiguous(),
                                    Vsd[s].contiguous())
        k0 = base["k0"] * scale[b]
        assert P.err(k0 - host(r[b]), k0 - host(r1[0]), floor=k0) <= 1.0, b
        rd = P.dense_explained(base["t"], base["ts"], base["c"], a[b], U[b], V[b], Us[b], Vs[b])
        assert P.err(k0 - host(r[b]), k0 - rd, floor=k0) <= 1.0, (b, "dense")


def test_failed_series_gives_nan_and_leaves_its_neighbours_alone(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N, M = 9, 100, 64
    x, diag, y = _gp_inputs(9, B, N)
    bad = diag.copy()
    bad[4, 37] = -50.0   # not positive definite from row 37 on
    xs = np.sort(np.random.default_rng(10).uniform(x.min() - 1.0, x.max() + 1.0, M))
    kernel = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3)
    xd, dd, bd, yd, xsd = dev(x, diag, bad, y, xs)
    good = G.GaussianProcess(kernel, xd, diag=dd, mean=0.3)
    gp = G.GaussianProcess(kernel, mean=0.3).compute(xd, diag=bd, quiet=True)
    assert host(gp._flag).tolist() == [0, 0, 0, 0, 37, 0, 0, 0, 0]
    ok = [b for b in range(B) if b != 4]
    for got, want in zip(gp.predict_at(yd, xsd, return_var=True), good.predict_at(yd, xsd, return_var=True)):
        assert bool(torch.isnan(got[4]).all())
        assert torch.equal(got[ok], want[ok])   # bit-identical to the same batch without the failure
        assert bool(torch.isfinite(want).all())
    assert bool(torch.isnan(gp.predict_at(yd, xsd)[4]).all())


@pytest.mark.parametrize("J", [2, 8, 32])
def test_two_calls_give_identical_bits(ops, J):
    import torch

    bt = batch(21, 130, 200, 170, J, per_t=True, per_ts=True, distinct=130 if J <= 8 else 6)
    t, ts, c, a, U, V, Us, Vs = dev(bt["t"], bt["ts"], bt["c"], bt["a"], bt["U"], bt["V"], bt["Us"], bt["Vs"])
    d, W, flag = ops.factor(t, c, a, U, V)
    r1 = ops.explained_variance(t, ts, c, U, W, d, Us, Vs)
    r2 = ops.explained_variance(t, ts, c, U, W, d, Us, Vs)
    assert bool(torch.isfinite(r1).all()) and torch.equal(r1, r2)


def test_graph_capture_of_explained_variance(ops):
    """One torch.cuda.graph capture of explained_variance on caller-owned out and work replays correctly on new ts, Us,
    Vs."""
    import torch

    B, N, M, J = 12, 257, 190, 8
    bt = batch(31, B, N, M, J, per_t=True, per_ts=True, distinct=B)
    t, ts, c, a, U, V, Us, Vs = dev(bt["t"], bt["ts"], bt["c"], bt["a"], bt["U"], bt["V"], bt["Us"], bt["Vs"])
    d, W, flag = ops.factor(t, c, a, U, V)
    out = torch.empty((B, M), dtype=torch.float64, device="cuda")
    work = torch.empty((B, M, J), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        ops.explained_variance(t, ts, c, U, W, d, Us, Vs, out=out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.explained_variance(t, ts, c, U, W, d, Us, Vs, out=out, work=work)
    # new queries for the same data: every draw's own, of another kind
    rng = np.random.default_rng(32)
    new = [P.draw_with_queries(1000 * 31 + k, N, J, t=dr["t"], ts=make_queries("dups", dr["t"], M, rng))
           for k, dr in enumerate(bt["draws"])]
    for dr, nw in zip(bt["draws"], new):
        assert np.array_equal(dr["U"], nw["U"]) and np.array_equal(dr["a"], nw["a"])   # the same data rows
    ts2, Us2, Vs2 = dev(np.stack([n["ts"] for n in new]), np.stack([n["Us"] for n in new]), np.stack([n["Vs"] for n in new]))
    ts.copy_(ts2); Us.copy_(Us2); Vs.copy_(Vs2)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    expect = ops.explained_variance(t, ts2, c, U, W, d, Us2, Vs2)
    assert torch.equal(out, expect)
    for b in (0, B - 1):
        nw = new[b]
        rd = P.dense_explained(nw["t"], nw["ts"], nw["c"], nw["a"], nw["U"], nw["V"], nw["Us"], nw["Vs"])
        assert P.err(nw["k0"] - host(out[b]), nw["k0"] - rd, floor=nw["k0"]) <= 1.0, b


def test_errors(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N, M, J = 2, 10, 7, 3
    bt = batch(41, B, N, M, J, per_t=False, per_ts=False)
    t, ts, c, a, U, V, Us, Vs = dev(bt["t"], bt["ts"], bt["c"], bt["a"], bt["U"], bt["V"], bt["Us"], bt["Vs"])
    d, W, flag = ops.factor(t, c, a, U, V)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="Invalid shape: ts"):
        ops.explained_variance(t, ts[:-1].contiguous(), c, U, W, d, Us, Vs)
    with pytest.raises(ValueError, match="Invalid shape: ts"):
        ops.explained_variance(t, z(B + 1, M), c, U, W, d, Us, Vs)
    with pytest.raises(ValueError, match="Invalid shape: Us"):
        ops.explained_variance(t, ts, c, U, W, d, Us[0], Vs)
    with pytest.raises(ValueError, match="Invalid shape: Us"):
        ops.explained_variance(t, ts, c, U, W, d, z(B, M, J + 1), Vs)
    with pytest.raises(ValueError, match="Invalid shape: Vs"):
        ops.explained_variance(t, ts, c, U, W, d, Us, z(B, M + 1, J))
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.explained_variance(t, ts, c, U, W, d, Us, Vs, out=z(B, M + 1))
    with pytest.raises(ValueError, match="Invalid shape: work"):
        ops.explained_variance(t, ts, c, U, W, d, Us, Vs, work=z(B, M))
    with pytest.raises(ValueError, match="alias"):
        ops.explained_variance(t, (per := z(B, M)), c, U, W, d, Us, Vs, out=per)
    with pytest.raises(ValueError, match="alias"):
        ops.explained_variance(t, ts, c, U, W, d, Us, Vs, work=Us)
    with pytest.raises(ValueError, match="alias"):
        ops.explained_variance(t, ts, c, U, W, d, Us, Vs, work=(buf := z(B, M, J)), out=buf.view(-1)[:B * M].view(B, M))
    # J = 40: declined by the entry point (widths 33 ... 128 have no kernel here), the usual ValueError
    with pytest.raises(ValueError, match="width not supported"):
        ops.explained_variance(z(N), z(M), z(40), z(B, N, 40), z(B, N, 40), z(B, N) + 1.0, z(B, M, 40), z(B, M, 40))

    x, diag, y = _gp_inputs(42, 3, 50)
    xd, dd, yd = dev(x, diag, y)
    kernel = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3)
    gp = G.GaussianProcess(kernel, xd, diag=dd)
    xs = torch.tensor([0.5, 0.4, 0.6], dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="sorted"):
        gp.predict_at(yd, xs, return_var=True)
    mu, var = gp.predict_at(yd, xs, return_var=True, check_sorted=False)   # (not checked: the caller's promise)
    assert tuple(var.shape) == (3, 3)
    with pytest.raises(ValueError, match="'t' must be"):
        gp.predict_at(yd, z(4, 3))
    with pytest.raises(ValueError, match="Invalid shape: y"):
        gp.predict_at(yd[:, :-1], xs.sort().values)
    conv = G.GaussianProcess(T.TermConvolution(kernel, 0.05), xd, diag=dd)
    with pytest.raises(ValueError, match="predict\\("):
        conv.predict_at(yd, xs.sort().values, return_var=True)
