# -*- coding: utf-8 -*-
"""GPU checks of the held-out log predictive density and of what it is built on: ops.explained_variance(..., workspace=True)
(c2_explained_variance_fwd), ops.explained_variance_rev (c2_explained_variance_rev, csrc/c2_predvar_rev.hip),
autograd.explained_variance / predict_variance / predictive_log_density[_kernel] and
GaussianProcess.predict_variance_kernel / predictive_log_density_kernel.

References: the numpy restatement of the sweep with its states and of its reverse (tests/explained_variance_rev_ref.py, pinned
to complex-step derivatives and to the dense closed form by tests/test_explained_variance_rev.py), fed with the device's own
inputs and workspace, and the dense objective under torch float64 autograd on the CPU.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; a reference that is identically zero must be met exactly."""
import numpy as np
import pytest

import explained_variance_rev_ref as R
import predict_at_ref as P
import term_params_ref as TP
from inverse_diag_ref import err as ref_err

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
SHAPES = [(1, 1), (2, 9), (7, 8), (8, 7), (9, 33), (33, 9), (150, 40)]   # (N, M): ring 8, pending 4, unroll 4, from both sides
NAMES = ("bt", "bts", "bc", "bU", "bW", "bd", "bUs", "bVs")
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


def check(key, x, xo, what=None):
    x = host(x) if hasattr(x, "cpu") else np.asarray(x)
    xo = np.asarray(xo)
    if not np.any(xo):
        e = 0.0 if not np.any(x) else np.inf
    else:
        e = ref_err(x, xo)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert np.all(np.isfinite(x)) and e <= 1.0, (what, key, e)


def batch(seed, B, N, J, M, kind, per_series, distinct=3):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct); per_series: every series on its own
    grids with its own rates, else all on the first draw's t, ts and c (shared (N,), (M,) and (J,) arrays)."""
    draws = []
    for k in range(min(B, distinct)):
        rng = np.random.default_rng(1000 * seed + k + 17)
        t = P.draw(1000 * seed + k, N, J)["t"] if (per_series or k == 0) else draws[0]["t"]
        ts = R.query_grid(kind, t, rng, M) if (per_series or k == 0) else draws[0]["ts"]
        draws.append(P.draw_with_queries(1000 * seed + k, N, J, t=t, ts=ts))
    idx = [b % len(draws) for b in range(B)]
    st = lambda key: np.stack([draws[i][key] for i in idx])
    sh = lambda key: st(key) if per_series else draws[0][key]
    return dict(t=sh("t"), ts=sh("ts"), c=sh("c"), a=st("a"), U=st("U"), V=st("V"), Us=st("Us"), Vs=st("Vs"), y=st("y"),
                k0=np.array([draws[i]["k0"] for i in idx]))


def factored(ops, bt):
    t, ts, c, a, U, V, Us, Vs = dev(*[bt[k] for k in ("t", "ts", "c", "a", "U", "V", "Us", "Vs")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    return [t, ts, c, U, W, d, Us, Vs]


def series(args, b):
    """The host arrays of series b (a shared t / ts / c as it is)."""
    out = []
    for x, per in zip(args, (1, 1, 1, 2, 2, 1, 2, 2)):
        x = host(x)
        out.append(x[b] if x.ndim == per + 1 else x)
    return out


def grid(J):
    """Every shape with B = 3 and B = 65 (a padded group; a second workgroup at every G); grid kinds and shared / per-series
    t, ts, c rotate so that each meets each shape."""
    for i, (N, M) in enumerate(SHAPES):
        for B in (3, 65):
            yield N, M, B, R.GRID_KINDS[(i + J + (B == 65)) % 4], bool((i + (B == 65)) % 2)


def picks(B):
    return sorted(set(range(min(B, 3))) | {B - 2, B - 1} - {-1})


@pytest.mark.parametrize("J", WIDTHS)
def test_forward_with_workspace(ops, J):
    """r and work have the bits of the plain call; Sws, Rws against the restatement fed with the device's d, W."""
    import torch

    for N, M, B, kind, per in grid(J):
        args = factored(ops, batch(10 * J + N, B, N, J, M, kind, per))
        what = (J, N, M, B, kind, per)
        work0, work1 = torch.empty_like(args[6]), torch.empty_like(args[6])
        r0 = ops.explained_variance(*args, work=work0)
        r1, (Sws, Rws) = ops.explained_variance(*args, work=work1, workspace=True)
        torch.cuda.synchronize()
        assert tuple(Sws.shape) == (B, N, J, J) and tuple(Rws.shape) == (B, N, J, J), what
        assert torch.equal(r0, r1) and torch.equal(work0, work1), what
        for b in picks(B):
            rr, Xr, Sr, Rr = R.forward_ws(*series(args, b))
            check("r", r1[b], rr, what); check("work", work1[b], Xr, what)
            check("Sws", Sws[b], Sr, what); check("Rws", Rws[b], Rr, what)
        if B == 65:   # a repeat of a draw: identical inputs give identical bits
            assert torch.equal(Sws[63], Sws[0]) and torch.equal(Rws[64], Rws[1]), what


def rev_case(ops, bt, seed, what, every=False):
    import torch

    B, N, J = bt["U"].shape
    M = bt["Us"].shape[1]
    args = factored(ops, bt)
    br, = dev(np.random.default_rng(seed).standard_normal((B, M)))
    work = torch.empty_like(args[6])
    r, ws = ops.explained_variance(*args, work=work, workspace=True)
    got = ops.explained_variance_rev(*args, work, ws, br)
    torch.cuda.synchronize()
    assert [tuple(g.shape) for g in got] == [(B, N), (B, M), (B, J), (B, N, J), (B, N, J), (B, N), (B, M, J), (B, M, J)], what
    for b in (range(B) if every else picks(B)):
        sa = series(args, b)
        ref = R.reverse_rows(*sa, host(work)[b], host(ws[0])[b], host(ws[1])[b], host(br)[b])
        for nm, g, w in zip(NAMES, got, ref):
            check(nm, g[b], w, (what, b))
        # exact zeros: bUs in front of the data, bVs with no data row above
        nq = R.last_rows(sa[0], sa[1])
        assert not bool(got[6][b][torch.from_numpy(nq < 0).cuda()].any()), (what, b)
        assert not bool(got[7][b][torch.from_numpy(nq == N - 1).cuda()].any()), (what, b)
    return args, work, ws, br, got


@pytest.mark.parametrize("J", WIDTHS)
def test_reverse_vs_restatement(ops, J):
    """All eight outputs against the numpy reverse fed with the device's own inputs and workspace: grids with ties and
    repeated queries, all queries in front of the data, all behind it, M = 1; shared and per-series t / ts / c."""
    for N, M, B, kind, per in grid(J):
        rev_case(ops, batch(20 * J + N, B, N, J, M, kind, per), J + N, (J, N, M, B, kind, per))
    for kind in R.GRID_KINDS:   # M = 1 on every kind of grid
        rev_case(ops, batch(30 * J + 1, 3, 9, J, 1, kind, True), J, (J, 9, 1, 3, kind, True))


def dense_kernel(coefs, tau):
    """k(tau) for tau >= 0 from the celerite coefficients (torch)."""
    import torch
    ar, cr, ac, bc, cc, dc = coefs
    tau = tau[..., None]
    return (ar * torch.exp(-cr * tau)).sum(-1) + (torch.exp(-cc * tau) * (ac * torch.cos(dc * tau) + bc * torch.sin(dc * tau))).sum(-1)


def dense_objective(coefs, x, t, D, r, rs, noise):
    """The held-out log predictive density of one series from dense algebra (torch float64, CPU).  Lags are taken SIGNED
    under the masks (a query at a data time has that row on its lower side): abs has derivative 0 at a tie."""
    import torch
    N = x.shape[0]
    dx = x[:, None] - x[None, :]
    low = torch.tril(torch.ones(N, N, dtype=torch.bool), -1)
    Kl = torch.where(low, dense_kernel(coefs, torch.where(low, dx, torch.zeros_like(dx))), torch.zeros_like(dx))
    k0 = coefs[0].sum() + coefs[2].sum()
    K = Kl + Kl.T + torch.diag(k0 + D)
    ds = t[:, None] - x[None, :]                     # (M, N)
    up = ds >= 0
    Ks = dense_kernel(coefs, torch.where(up, ds, -ds))
    sol = torch.linalg.solve(K, torch.cat([r[:, None], Ks.T], dim=1))
    mu = Ks @ sol[:, 0]
    var = k0 - (Ks.T * sol[:, 1:]).sum(0) + noise
    return -0.5 * ((rs - mu) ** 2 / var + torch.log(var)).sum() - 0.5 * t.shape[0] * np.log(2.0 * np.pi)


RECS = [TP.rec("sho", (0, 1, 2), regime="under"), TP.rec("real", (3, 4)), TP.rec("matern32", (5, 6))]
SHARED_COLS = (4, 5)   # RealTerm.c and Matern32Term.sigma are 0-d tensors; the other parameters (B,) columns


def kernel_case(seed, B, N, M):
    rng = np.random.default_rng(seed)
    Pm = np.concatenate([TP.draw("sho", rng, B, regime="under")[1], TP.draw("real", rng, B)[1], TP.draw("matern32", rng, B)[1]], 1)
    Pm[:, SHARED_COLS] = Pm[0, SHARED_COLS]
    x = np.sort(rng.uniform(0, max(N, 2) / 10.0, (B, N)), axis=1)
    t = np.sort(rng.uniform(-0.3, max(N, 2) / 10.0 + 0.3, (B, M)), axis=1)
    if M > 3:
        t[:, 1] = x[:, N // 2]      # a tie with a data time
        t[:, 2] = t[:, 3]           # a repeated query
        t = np.sort(t, axis=1)
    ye, yen = np.sqrt(rng.uniform(0.1, 0.3, (B, N))), np.sqrt(rng.uniform(0.1, 0.3, (B, M)))
    y, ys = np.sin(x) + 0.1 * rng.standard_normal((B, N)), np.sin(t) + 0.1 * rng.standard_normal((B, M))
    return Pm, x, t, ye, yen, y, ys, rng.uniform(0.05, 0.4, B), float(rng.uniform(-0.3, 0.3))


def build_kernel(Pt, sc, ss):
    from celerite2_amd import terms as T
    return (T.SHOTerm(S0=Pt[:, 0], w0=Pt[:, 1], Q=Pt[:, 2], regime="under") + T.RealTerm(a=Pt[:, 3], c=sc)
            + T.Matern32Term(sigma=ss, rho=Pt[:, 6]))


def exact_series(Pb, xb, tb, yeb, yenb, jb, m, yb, ysb):
    """value, bP, bjitter, bmean, bx, bt, byerr, byerr_new, by, bys of ONE series: dense torch autograd down to the
    coefficients, term_params_ref.coefficients_rev from there to the parameters."""
    import torch
    tn = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
    coefs = [tn(v[0]) for v in TP.coefficients(RECS, Pb[None])]
    x, t, ye, yen, j, mean, y, ys = [tn(v) for v in (xb, tb, yeb, yenb, jb, m, yb, ysb)]
    val = dense_objective(coefs, x, t, ye * ye + j * j, y - mean, ys - mean, yen * yen + j * j)
    g = torch.autograd.grad(val, coefs + [x, t, ye, yen, j, mean, y, ys])
    bP = TP.coefficients_rev(RECS, Pb[None], [v.numpy()[None] for v in g[:6]])[0]
    return (float(val.detach()), bP) + tuple(g[k].numpy() for k in (10, 11, 6, 7, 8, 9, 12, 13))


@pytest.mark.parametrize("M", [1, 40])
@pytest.mark.parametrize("N", [2, 33, 150])
def test_predictive_log_density_kernel_vs_dense(ops, N, M):
    """SHO (under) + Real + Matern32, (B,) and 0-d parameters mixed, a (B,) jitter, a 0-d mean, yerr as sigma, noisy held-out
    values: the value and the gradient of every tensor -- x, t, y, ys, yerr, yerr_new, jitter and mean included."""
    import torch
    from celerite2_amd import autograd as ag

    B = 5
    Pm, x, t, ye, yen, y, ys, jit, mean = kernel_case(50 + N + M, B, N, M)
    Pt, xd, td, yed, yend, yd, ysd, jt = [v.requires_grad_() for v in dev(Pm, x, t, ye, yen, y, ys, jit)]
    sc, ss, mt = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in (Pm[0, 4], Pm[0, 5], mean)]
    lpd = ag.predictive_log_density_kernel(build_kernel(Pt, sc, ss), xd, yd, td, ysd, yerr=yed, jitter=jt, mean=mt, yerr_new=yend)
    assert tuple(lpd.shape) == (B,)
    lpd.sum().backward()
    want = [exact_series(Pm[b], x[b], t[b], ye[b], yen[b], jit[b], mean, y[b], ys[b]) for b in range(B)]
    what = (N, M)
    bP = np.stack([w[1] for w in want])
    check("lpd", lpd, np.array([w[0] for w in want]), what)
    per = [k for k in range(7) if k not in SHARED_COLS]
    check("lpd bP", Pt.grad[:, per], bP[:, per], what)
    assert not bool(Pt.grad[:, list(SHARED_COLS)].any())
    check("lpd bP shared", sc.grad, bP[:, 4].sum(), what)
    check("lpd bP shared", ss.grad, bP[:, 5].sum(), what)
    check("lpd bjitter", jt.grad, np.array([w[2] for w in want]), what)
    check("lpd bmean", mt.grad, np.sum([w[3] for w in want]), what)
    check("lpd bx", xd.grad, np.stack([w[4] for w in want]), what)
    check("lpd bt", td.grad, np.stack([w[5] for w in want]), what)
    check("lpd byerr", yed.grad, np.stack([w[6] for w in want]), what)
    check("lpd byerr_new", yend.grad, np.stack([w[7] for w in want]), what)
    check("lpd by", yd.grad, np.stack([w[8] for w in want]), what)
    check("lpd bys", ysd.grad, np.stack([w[9] for w in want]), what)


@pytest.mark.parametrize("per", [True, False])
def test_autograd_chain_vs_dense(ops, per):
    """autograd.factor -> autograd.explained_variance, and predict_variance / predictive_log_density on top of it, at the
    matrix level against explained_variance_rev_ref.dense_variance under torch autograd; shared t / ts / c get the batch sum."""
    import torch
    from celerite2_amd import autograd as ag

    B, N, M, J = 4, 33, 12, 5
    bt = batch(91, B, N, J, M, "mixed", per, distinct=B)
    keys = ("t", "ts", "c", "a", "U", "V", "Us", "Vs")
    leaves = [x.requires_grad_() for x in dev(*[bt[k] for k in keys])]
    t, ts, c, a, U, V, Us, Vs = leaves
    k0, bvar = dev(bt["k0"], np.random.default_rng(5).standard_normal((B, M)))
    var = ag.predict_variance(t, c, a, U, V, ts, Us, Vs, k0)
    d, W = ag.factor(t, c, a, U, V)
    assert torch.equal(var, k0[:, None] - ag.explained_variance(t, ts, c, U, W, d, Us, Vs))
    (var * bvar).sum().backward()
    cpu = [torch.tensor(bt[k], dtype=torch.float64, requires_grad=True) for k in keys]
    want = R.dense_variance(*cpu, torch.tensor(bt["k0"])[:, None])
    grads = torch.autograd.grad(want, cpu, torch.tensor(host(bvar)))
    check("chain var", var, want.detach().numpy(), per)
    for nm, leaf, g in zip(keys, leaves, grads):
        assert tuple(leaf.grad.shape) == tuple(g.shape), (nm, per)
        check("chain b" + nm, leaf.grad, g.numpy(), (nm, per))
    # the objective at the matrix level is the density of (mean, variance)
    y, ys = dev(bt["y"], np.random.default_rng(6).standard_normal((B, M)))
    with torch.no_grad():
        lpd = ag.predictive_log_density(t, c, a, U, V, y, ts, Us, Vs, k0, ys)
        mu = ag.predict_mean(t, c, a, U, V, y, ts, Us, Vs)
    ref = -0.5 * ((host(ys) - host(mu)) ** 2 / host(var) + np.log(2 * np.pi * host(var))).sum(1)
    check("matrix lpd", lpd, ref, per)


def test_gp_frontend(ops):
    """gp.predict_variance_kernel equals gp.predict_at(..., return_var=True)[1]; gp.predictive_log_density_kernel is the autograd
    function on the GP's own t, diag, mean and the density of predict_at's mean and variance."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N, M = 6, 150, 40
    rng = np.random.default_rng(12)
    x = np.sort(rng.uniform(0, 0.05 * N + 5, (B, N)), axis=1)
    tq = np.sort(rng.uniform(-1.0, 0.05 * N + 6, (B, M)), axis=1)
    diag = rng.uniform(0.05, 0.4, (B, N))
    y, ys = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3, np.sin(tq) + 0.3
    xd, td, dd, yd, ysd = dev(x, tq, diag, y, ys)
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kernel = T.SHOTerm(S0=tn(1.2), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.7), c=0.3)
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=tn(0.3))
    mu, var = gp.predict_at(yd, td, return_var=True)
    check("gp variance", gp.predict_variance_kernel(yd, td), host(var))
    lpd = gp.predictive_log_density_kernel(yd, td, ysd)
    assert tuple(lpd.shape) == (B,)
    assert torch.equal(lpd, ag.predictive_log_density_kernel(kernel, gp._t, yd, td, ysd, diag=gp._diag, mean=gp.mean))
    ref = -0.5 * ((ys - host(mu)) ** 2 / host(var) + np.log(2 * np.pi * host(var))).sum(1)
    check("gp lpd", lpd, ref)
    yen, = dev(rng.uniform(0.1, 0.3, (B, M)))
    lpd2 = gp.predictive_log_density_kernel(yd, td, ysd, jitter=tn(0.2), yerr_new=yen)
    var_j = gp.predict_variance_kernel(yd, td, jitter=tn(0.2))
    mu_j = gp.predict_kernel(yd, td, jitter=tn(0.2))
    vj = host(var_j) + host(yen) ** 2 + 0.04
    check("gp lpd jitter", lpd2, -0.5 * ((ys - host(mu_j)) ** 2 / vj + np.log(2 * np.pi * vj)).sum(1))


@pytest.mark.parametrize("J", [2, 8, 32])
def test_two_calls_give_identical_bits(ops, J):
    import torch

    B, N, M = 130, 200, 150
    args = factored(ops, batch(21, B, N, J, M, "ties", True, distinct=6))
    br, = dev(np.random.default_rng(J).standard_normal((B, M)))
    work = torch.empty_like(args[6])
    r, ws = ops.explained_variance(*args, work=work, workspace=True)
    g1 = ops.explained_variance_rev(*args, work, ws, br)
    g2 = ops.explained_variance_rev(*args, work, ws, br)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_graph_capture_of_the_forward_and_reverse_sweeps(ops):
    """One torch.cuda.graph capture of explained_variance(workspace) -> explained_variance_rev on caller-owned buffers
    replays to the eager bits on new data."""
    import torch

    B, N, M, J = 12, 257, 100, 8
    args = factored(ops, batch(31, B, N, J, M, "mixed", True, distinct=12))
    f64 = dict(dtype=torch.float64, device="cuda")
    r, work = torch.empty((B, M), **f64), torch.empty((B, M, J), **f64)
    ws = (torch.empty((B, N, J, J), **f64), torch.empty((B, N, J, J), **f64))
    out = tuple(torch.empty(s, **f64) for s in ((B, N), (B, M), (B, J), (B, N, J), (B, N, J), (B, N), (B, M, J), (B, M, J)))
    br, = dev(np.random.default_rng(5).standard_normal((B, M)))

    def chain():
        ops.explained_variance(*args, out=r, work=work, ws=ws)
        ops.explained_variance_rev(*args, work, ws, br, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    br.copy_(torch.from_numpy(np.random.default_rng(32).standard_normal((B, M))).cuda())
    for o in (r, work) + ws + out:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    work_e = torch.empty_like(work)
    r_e, ws_e = ops.explained_variance(*args, work=work_e, workspace=True)
    out_e = ops.explained_variance_rev(*args, work_e, ws_e, br)
    assert torch.equal(r, r_e) and torch.equal(work, work_e) and all(torch.equal(a, b) for a, b in zip(ws, ws_e))
    assert all(torch.equal(a, b) for a, b in zip(out, out_e))
    ref = R.reverse_rows(*series(args, 0), host(work)[0], host(ws[0])[0], host(ws[1])[0], host(br)[0])
    for nm, g, w in zip(NAMES, out, ref):
        check("graph " + nm, g[0], w)


def test_seventy_thousand_series(ops):
    """B = 70 000 x N = 4 x M = 3 x J = 2: seven distinct series repeated; the seven against the restatement, and EVERY series
    bit-identical to its repeat in the first seven."""
    import torch

    B, N, M, J, D = 70000, 4, 3, 2, 7
    rev = rev_case(ops, batch(8, D, N, J, M, "mixed", True, distinct=D), 8, "7 alone", every=True)
    args7, work7, ws7, br7, got7 = rev
    rep = lambda x: x.repeat((B // D,) + (1,) * (x.dim() - 1)).contiguous()
    args = [rep(x) for x in args7]
    br, work = rep(br7), torch.empty((B, M, J), dtype=torch.float64, device="cuda")
    r, ws = ops.explained_variance(*args, work=work, workspace=True)
    got = ops.explained_variance_rev(*args, work, ws, br)
    torch.cuda.synchronize()
    for big, small in zip((work,) + tuple(ws) + tuple(got), (work7,) + tuple(ws7) + tuple(got7)):
        assert torch.equal(big.reshape((B // D, D) + tuple(small.shape[1:])), small[None].expand((B // D,) + tuple(small.shape))), small.shape


def test_wide_models_are_refused(ops):
    import torch

    f = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")
    B, N, M, J = 2, 5, 3, 33
    args = [f(N), f(M), f(J), f(B, N, J), f(B, N, J), f(B, N), f(B, M, J), f(B, M, J)]
    with pytest.raises(ValueError, match="width not supported"):
        ops.explained_variance(*args, workspace=True)
    with pytest.raises(ValueError, match="width not supported"):
        ops.explained_variance_rev(*args, f(B, M, J), (f(B, N, J, J), f(B, N, J, J)), f(B, M))


def test_shape_and_aliasing_errors(ops):
    import torch

    args = factored(ops, batch(41, 2, 10, 3, 6, "mixed", False))
    t, ts, c, U, W, d, Us, Vs = args
    work = torch.empty_like(Us)
    r, ws = ops.explained_variance(*args, work=work, workspace=True)
    br = torch.ones_like(r)
    with pytest.raises(ValueError, match="Invalid shape: br"):
        ops.explained_variance_rev(*args, work, ws, br[:, :-1].contiguous())
    with pytest.raises(ValueError, match="Invalid shape: work"):
        ops.explained_variance_rev(*args, work[:1].contiguous(), ws, br)
    with pytest.raises(ValueError, match="Invalid shape: Sws"):
        ops.explained_variance_rev(*args, work, (work, ws[1]), br)
    with pytest.raises(ValueError, match="Invalid shape: Rws"):
        ops.explained_variance(*args, ws=(ws[0], work))
    with pytest.raises(ValueError, match="Invalid shape: Vs"):
        ops.explained_variance_rev(t, ts, c, U, W, d, Us, Vs[:, :-1].contiguous(), work, ws, br)
    with pytest.raises(ValueError, match="work must not alias Us"):
        ops.explained_variance(*args, work=Us, workspace=True)
    with pytest.raises(ValueError, match="Rws must not alias Sws"):
        ops.explained_variance(*args, ws=(ws[0], ws[0]))
    good = ops.explained_variance_rev(*args, work, ws, br)
    for k, (nm, other) in enumerate((("bt", d), ("bts", br), ("bU", U), ("bW", W), ("bd", d), ("bUs", Us), ("bVs", work))):
        k = k if k < 2 else k + 1   # (c is shared here: (J,) cannot stand in for bc (B, J))
        out = list(good)
        out[k] = other
        with pytest.raises(ValueError, match="%s must not alias" % nm):
            ops.explained_variance_rev(*args, work, ws, br, out=tuple(out))
    out = list(good)
    out[7] = out[6]
    with pytest.raises(ValueError, match="bVs must not alias bUs"):
        ops.explained_variance_rev(*args, work, ws, br, out=tuple(out))


def test_refusals_of_the_objective(ops):
    """A TermConvolution anywhere in the kernel's tree is refused with a ValueError that names `predict`; a failed
    factorisation raises LinAlgError."""
    import torch
    from celerite2_amd import autograd as ag, terms as T

    B, N, M = 3, 20, 5
    rng = np.random.default_rng(3)
    x, tq = np.sort(rng.uniform(0, 5, (B, N)), axis=1), np.sort(rng.uniform(0, 5, (B, M)), axis=1)
    xd, td, yd, ysd, dd = dev(x, tq, rng.standard_normal((B, N)), rng.standard_normal((B, M)), rng.uniform(0.1, 0.3, (B, N)))
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True)
    base = T.SHOTerm(S0=tn(1.2), w0=tn(0.9), Q=tn(2.5), regime="under")
    real = T.RealTerm(a=tn(0.7), c=0.3)
    with pytest.raises(ValueError, match="predict"):
        ag.predictive_log_density_kernel(T.TermConvolution(base + real, 0.05), xd, yd, td, ysd, diag=dd)
    nested = base + real
    nested.terms.append(T.TermConvolution(real, 0.05))   # (the constructors refuse this: the check must not rely on them)
    with pytest.raises(ValueError, match="predict"):
        ag.predictive_log_density_kernel(nested, xd, yd, td, ysd, diag=dd)
    bad = dd.clone()
    bad[1, 7] = -50.0   # not positive definite from row 7 on
    with pytest.raises(ag.LinAlgError):
        ag.predictive_log_density_kernel(base + real, xd, yd, td, ysd, diag=bad)
    ok = ag.predictive_log_density_kernel(base + real, xd, yd, td, ysd, diag=dd)
    assert tuple(ok.shape) == (B,) and bool(torch.isfinite(ok).all())


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
