# -*- coding: utf-8 -*-
"""GPU checks of the transit search under correlated noise: ops.whitened_transits (c2_whitened_transits,
csrc/c2_transit.hip) and GaussianProcess.transit_search.

References: the numpy restatement of the sweep (tests/transit_ref.py, pinned to dense algebra by tests/test_transit.py), fed
with the device's own d, W and Z0, and two dense generalized-least-squares fits per trial on the host.  Criterion: the
standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly.  Every trial set
has its template edges at midpoints between neighbouring sample distances (transit_ref.trials_for)."""
import numpy as np
import pytest

import transit_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
LENGTHS = [1, 2, 7, 8, 9, 16, 17, 33, 150]   # the 16-row staged block and its tails, from both sides
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
    return x.detach().cpu().numpy()


def check(key, x, xo, what=None):
    x = host(x) if hasattr(x, "cpu") else np.asarray(x, dtype=float)
    xo = np.asarray(xo, dtype=float)
    assert x.shape == xo.shape, (what, key, x.shape, xo.shape)
    assert np.array_equal(np.isnan(x), np.isnan(xo)), (what, key)
    m = ~np.isnan(xo)
    e = R.err(x[m], xo[m]) if m.any() and np.any(xo[m]) else (0.0 if not np.any(x[m]) else np.inf)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert e <= 1.0, (what, key, e)


def batch(seed, B, N, J, Q0, K, per_tc, per_tr, shift=0.0, **kw):
    """B seeded draws with Y0 = [design(t, Q0 - 1) | y] and a trial set each.  per_tc: every series on its own grid with its
    own rates, else all on the first draw's t and c (shared (N,) and (J,) arrays); per_tr: (B, K, 4) trials, else the first
    draw's (K, 4).  shift: added to every time before the trials are made (the celerite matrices depend on differences
    only).  kw: transit_ref.trials_for's."""
    draws = []
    for k in range(B):
        D = R.draw(1000 * seed + k, N, J, t=None if (per_tc or k == 0) else draws[0]["t"])
        D["Y0"] = np.concatenate([R.design(D["t"], Q0 - 1), D["y"][:, None]], axis=1)
        D["t"] = D["t"] + shift
        D["trials"] = R.trials_for(D["t"], K, seed=seed + k, **kw)
        draws.append(D)
    st = lambda key: np.stack([D[key] for D in draws])
    return dict(t=st("t") if per_tc else draws[0]["t"], c=st("c") if per_tc else draws[0]["c"], a=st("a"), U=st("U"), V=st("V"),
                Y0=st("Y0"), trials=st("trials") if per_tr else draws[0]["trials"])


def run(ops, bt):
    """(T on the device, the batched restatement on the device's own d, W, Z0)."""
    import torch

    t, c, a, U, V, Y0, trials = dev(*[bt[k] for k in ("t", "c", "a", "U", "V", "Y0", "trials")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    Z0 = ops.solve_lower(t, c, U, W, Y0)
    T = ops.whitened_transits(t, c, U, W, d, Z0, trials)
    torch.cuda.synchronize()
    B, N, J = U.shape
    full = lambda x, n: np.broadcast_to(x, (B,) + x.shape) if x.ndim == n else x
    want = R.whitened_transits_batched(full(bt["t"], 1), full(bt["c"], 1), bt["U"], host(W), host(d), host(Z0),
                                       full(bt["trials"], 2))
    return T, want, (t, c, U, W, d, Z0, trials)


@pytest.mark.parametrize("J", WIDTHS)
def test_op_vs_restatement(ops, J):
    """Every width on every length at K = 65, Q0 = 2, boxes and trapezoids, folded and single, lane by lane; B = 1 and 3,
    shared and per-series t, c and trials rotate so that each meets each length over the widths."""
    jx = WIDTHS.index(J)
    for i, N in enumerate(LENGTHS):
        B = (1, 3)[(i + jx) % 2]
        per_tc, per_tr = bool((i // 2 + jx) % 2), bool((i + jx // 2) % 2)
        T, want, _ = run(ops, batch(10 * J + N, B, N, J, 2, 65, per_tc, per_tr))
        assert tuple(T.shape) == (B, 65, 3)
        check("T vs restatement", T, want, (J, N, B, per_tc, per_tr))


@pytest.mark.parametrize("J", [3, 8, 32])
def test_lane_tail_and_columns(ops, J):
    """The lane tail, a second and a third wavefront and every accumulator count: K x Q0 at N = 33."""
    for K in (1, 2, 63, 64, 65, 130):
        for Q0 in (1, 2, 3, 8):
            B = 1 + (K + Q0) % 3
            T, want, _ = run(ops, batch(J + K + Q0, B, 33, J, Q0, K, bool(K % 2), bool(Q0 % 2)))
            assert tuple(T.shape) == (B, K, 1 + Q0)
            check("T vs restatement", T, want, (J, K, Q0, B))


@pytest.mark.parametrize("J", [2, 8, 32])
def test_mixed_wavefront_and_offset(ops, J):
    """Folded and single-event trials, boxes and trapezoids interleaved lane by lane (every neighbouring pair of lanes
    differs in kind), then the same on times offset by 2.45e6 with the epochs at the offset."""
    kinds = ("fold-box", "single-trap", "fold-trap", "single-box", "single-trap", "fold-box", "single-box")
    bt = batch(70 + J, 3, 33, J, 2, 130, True, True, kinds=kinds)
    assert len({tuple(r[[0, 3]] > 0) for r in bt["trials"][0][:7]}) == 4          # all four kinds among neighbouring lanes
    T, want, _ = run(ops, bt)
    check("T vs restatement, mixed wavefront", T, want, J)
    jd = batch(70 + J, 3, 33, J, 2, 130, True, True, shift=2.45e6, kinds=kinds)
    assert float(jd["trials"][..., 1].min()) > 2.4e6
    T, want, _ = run(ops, jd)
    check("T vs restatement, offset times", T, want, J)


@pytest.mark.parametrize("J,N", [(4, 150), (32, 40)])
def test_single_events_sorted_by_epoch(ops, J, N):
    """Single events sorted by epoch, the first and last quarter before t_0 and after t_{N-1}: their templates are zero at
    every row, so their products are exact zeros and the finish gives NaN there and only there."""
    import torch
    from celerite2_amd import periodogram as pg, transit as tr

    K = 130
    bt = batch(90 + J, 2, N, J, 2, K, True, True, kinds=("single-box", "single-trap"), outside=True)
    out = np.r_[0:K // 4, K - K // 4:K]
    n_in, _ = R.counts(bt["t"][0], bt["trials"][0])
    assert np.all(n_in[out] == 0) and np.all(np.delete(n_in, out) >= 2)
    assert np.all(np.diff(bt["trials"][..., 1], axis=-1) >= 0)
    T, want, ins = run(ops, bt)
    check("T vs restatement, single events", T, want, (J, N))
    assert bool((T[:, out] == 0).all()) and np.all(want[:, out] == 0)
    d, Z0, trials = ins[4], ins[5], ins[6]
    fit = tr.finish(pg.null_products(Z0, d), T, N, trials=trials)
    ref = tr.finish(torch.from_numpy(np.stack([R.null_products(host(Z0)[b], host(d)[b]) for b in range(2)])),
                    torch.from_numpy(want), N, trials=torch.from_numpy(bt["trials"]))
    nan = np.zeros(K, dtype=bool)
    nan[out] = True
    for name, x, xo in zip(fit._fields, fit, ref):
        if name != "chi2_null":
            assert np.array_equal(np.isnan(host(x)), np.broadcast_to(nan, (2, K))), name
        check("finish on the device's T vs on the restatement's, " + name, x, xo.numpy(), (J, N))


@pytest.mark.parametrize("J,N,K,Q0", [(2, 9, 5, 1), (8, 33, 65, 2), (32, 20, 40, 3), (16, 150, 130, 8)])
def test_plain_call_properties(ops, J, N, K, Q0):
    """Two calls give identical bits, a caller-owned `out` gives the same bits, inputs are unchanged, `out` may not alias an
    input, and a non-contiguous or mis-shaped input is refused."""
    import torch

    T0, want, ins = run(ops, batch(50 + J, 3, N, J, Q0, K, True, True))
    before = [x.clone() for x in ins]
    T1 = ops.whitened_transits(*ins)
    own = torch.full((3, K, 1 + Q0), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.whitened_transits(*ins, out=own) is own
    torch.cuda.synchronize()
    assert torch.equal(T0, T1) and torch.equal(T0, own)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))
    t, c, U, W, d, Z0, trials = ins
    pool = torch.zeros(max(own.numel(), Z0.numel()), dtype=torch.float64, device="cuda")
    pool[:Z0.numel()] = Z0.reshape(-1)
    with pytest.raises(ValueError, match="out must not alias Z0"):
        ops.whitened_transits(t, c, U, W, d, pool[:Z0.numel()].view(Z0.shape), trials, out=pool[:own.numel()].view(own.shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_transits(t, c, U, W, d, Z0.transpose(0, 1).contiguous().transpose(0, 1), trials)
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_transits(t, c, U, W, d, Z0, torch.stack([trials, trials], dim=-1)[..., 0])
    with pytest.raises(ValueError, match="Invalid shape: trials"):
        ops.whitened_transits(t, c, U, W, d, Z0, trials[:2])
    with pytest.raises(ValueError, match="Invalid shape: trials"):
        ops.whitened_transits(t, c, U, W, d, Z0, trials[..., :3].contiguous())
    with pytest.raises(ValueError, match="Invalid shape: Z0"):
        ops.whitened_transits(t, c, U, W, d, Z0[:, :-1].contiguous(), trials)
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.whitened_transits(*ins, out=own[:, :-1].contiguous())


def test_unsupported_sizes(ops):
    """J = 33 and Q0 = 9 return C2_ERR_UNSUPPORTED through ops (a ValueError naming the op), before any launch."""
    import torch

    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="whitened_transits: width not supported"):
        ops.whitened_transits(z(5), z(33), z(1, 5, 33), z(1, 5, 33), z(1, 5) + 1, z(1, 5, 2), z(3, 4))
    with pytest.raises(ValueError, match="whitened_transits: width not supported"):
        ops.whitened_transits(z(5), z(2), z(1, 5, 2), z(1, 5, 2), z(1, 5) + 1, z(1, 5, 9), z(3, 4))


def test_graph_capture(ops):
    """The op with a caller-owned `out` under torch.cuda.graph (one kernel node, no parallel branches): the replay writes
    the bits of the plain call."""
    import torch

    T0, _, ins = run(ops, batch(61, 3, 33, 8, 2, 130, True, True))
    out = torch.zeros_like(T0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.whitened_transits(*ins, out=out)              # (warm-up on the capturing stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.whitened_transits(*ins, out=out)
    torch.cuda.synchronize()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, T0)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, T0)


# ---- gp.transit_search --------------------------------------------------------------------------------------------------
def gp_case(B, N, seed=1):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.3, (B, N))
    A = np.stack([np.ones_like(x), x / 30.0 - 0.5, (x / 30.0 - 0.5) ** 2], axis=2)
    trials = np.stack([R.trials_for(x[b], 40, seed=seed + b) for b in range(B)])
    dip = np.stack([R.template(x[b], trials[b, :1])[:, 0] for b in range(B)])
    y = -1.5 * dip + 0.3 * rng.standard_normal((B, N)) + 0.3 + A @ np.array([0.5, -2.0, 1.0])
    return x, diag, A, y, trials


def make_kernel(J):
    import torch
    from celerite2_amd import terms as T

    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    k = T.SHOTerm(S0=tn(0.4), w0=tn(0.9), Q=tn(2.5), regime="under")                        # J = 2
    if J == 8:
        k = k + T.SHOTerm(S0=tn(0.2), w0=tn(2.3), Q=tn(4.0), regime="under") + T.SHOTerm(S0=tn(0.1), w0=tn(4.1), Q=tn(1.5), regime="under") \
            + T.RealTerm(a=tn(0.2), c=0.3) + T.RealTerm(a=tn(0.1), c=1.1)
    return k, tn


def dense_of(gp, x, b):
    c = host(gp._c)
    return R.dense(x[b], c[b] if c.ndim == 2 else c, host(gp._a)[b], host(gp._U)[b], host(gp._V)[b])


@pytest.mark.parametrize("J", [2, 8])
@pytest.mark.parametrize("design", ["mean", None, "batched3"])
def test_gp_transit_search_vs_dense(ops, design, J):
    """gp.transit_search with return_fit against two dense GLS fits per trial on the host at B = 3, N = 150, P0 = 1, 0 and 3;
    shared and per-series trials, a tensor mean; the plain call returns delta_chi2."""
    import torch
    from celerite2_amd import gp as G, transit as tr

    B, N, K = 3, 150, 40
    x, diag, A, y, trials = gp_case(B, N)
    x[...] = x[0]                                      # (one time grid, so that a shared trial set has midpoint edges everywhere)
    if design == "batched3":
        A = A * (1.0 + 0.5 * np.arange(B))[:, None, None]
    xd, dd, Ad, yd = dev(x, diag, A, y)
    kernel, tn = make_kernel(J)
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=tn(0.3))
    assert gp._U.shape[-1] == J
    use = {"mean": "mean", None: None, "batched3": Ad}[design]
    A0 = {"mean": A[..., :1] * 0 + 1, None: A[..., :0], "batched3": A}[design]
    trials[...] = trials[0]
    for trs in (trials, trials[0]):
        td, = dev(trs)
        want = [R.dense_search(dense_of(gp, x, b), x[b], A0[b], y[b] - 0.3, trs[b] if trs.ndim == 3 else trs) for b in range(B)]
        dchi2, depth, derr, chi2_0 = [np.stack([w[k] for w in want]) for k in range(4)]
        fit = gp.transit_search(yd, td, A=use, return_fit=True)
        assert isinstance(fit, tr.TransitSearch)
        assert all(tuple(v.shape) == (B, K) for v in fit[:4]) and tuple(fit.chi2_null.shape) == (B,)
        for b in range(B):
            what = (design, J, trs.ndim, b)
            check("gp delta_chi2 vs dense", fit.delta_chi2[b], dchi2[b], what)
            check("gp depth vs dense", fit.depth[b], depth[b], what)
            check("gp depth_err vs dense", fit.depth_err[b], derr[b], what)
            check("gp snr vs dense", fit.snr[b], depth[b] / derr[b], what)
        check("gp chi2_null vs dense", fit.chi2_null, chi2_0, (design, J))
        assert torch.equal(gp.transit_search(yd, td, A=use), fit.delta_chi2)


def test_quiet_failures_and_argument_errors(ops):
    """compute(quiet=True) with one series failing its factorisation: it holds NaN, its neighbours keep their bits; a
    repeated nuisance column is NaN throughout; an out-of-domain trial is NaN at that trial only; bad arguments are named."""
    import torch
    from celerite2_amd import gp as G

    B, N = 4, 33
    x, diag, A, y, trials = gp_case(B, N, seed=9)
    bad_diag, bad_A = diag.copy(), A.copy()
    bad_diag[1, 7] = -50.0            # not positive definite from row 7 on
    bad_A[2, :, 2] = bad_A[2, :, 1]   # rank 2
    trials[:, 5, 3] = 0.75 * trials[:, 5, 2]          # tau > w / 2
    xd, dd, bdd, Ad, bAd, yd, td = dev(x, diag, bad_diag, A, bad_A, y, trials)
    kernel, tn = make_kernel(2)
    clean = G.GaussianProcess(kernel, xd, diag=dd).transit_search(yd, td, return_fit=True)
    keep = np.arange(trials.shape[1]) != 5
    for v in clean[:4]:
        assert bool(torch.isnan(v[:, 5]).all()) and bool(torch.isfinite(v[:, keep]).all())
    gp = G.GaussianProcess(kernel)
    gp.compute(xd, diag=bdd, quiet=True)
    fit = gp.transit_search(yd, td, return_fit=True)
    for b in range(B):
        if b == 1:
            assert all(bool(torch.isnan(v[b]).all()) for v in fit)
        else:
            for got, want in zip(fit, clean):
                assert np.array_equal(host(got[b]), host(want[b]), equal_nan=True), b
    rank = G.GaussianProcess(kernel, xd, diag=dd).transit_search(yd, td, A=bAd, return_fit=True)
    full = G.GaussianProcess(kernel, xd, diag=dd).transit_search(yd, td, A=Ad, return_fit=True)
    for b in range(B):
        if b == 2:
            assert all(bool(torch.isnan(v[b]).all()) for v in rank)
        else:
            for nm, got, want in zip(rank._fields, rank, full):
                check("rank-deficient neighbour " + nm, got[b], host(want[b]), b)
    good = G.GaussianProcess(kernel, xd, diag=dd)
    for bad in (Ad[:, :-1], Ad[:-1], Ad[0, :, 0], Ad[..., None], torch.cat([Ad, Ad, Ad], dim=-1)[..., :8]):
        with pytest.raises(ValueError, match="Invalid shape: A"):
            good.transit_search(yd, td, A=bad.contiguous())
    with pytest.raises(ValueError, match="A must be"):
        good.transit_search(yd, td, A="ones")
    for bad in (td[:-1], td[..., :3], td[0, :, 0], td[None]):
        with pytest.raises(ValueError, match="Invalid shape: trials"):
            good.transit_search(yd, bad.contiguous())
    with pytest.raises(ValueError, match="Invalid shape: y"):
        good.transit_search(yd[:, :-1], td)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
