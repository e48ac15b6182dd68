# -*- coding: utf-8 -*-
"""GPU checks of posterior draws at new times in linear time: ops.prior_draw (c2_prior_draw, csrc/c2_priordraw.hip) at
every width up to 32, and GaussianProcess.sample_at on top of it.

References: the numpy restatement of the recurrence (tests/sample_at_ref.py, pinned to dense algebra by
tests/test_sample_at.py) for individual draws, criterion the standing one per element with floor max |f_o|,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |f_o|; and, for sample_at as a distribution, the existing predict(y, t) and
predict(y, t, return_cov=True): fed identity normals the chain is a linear map A, so mean and A A^T are compared
deterministically (floor k(0) for the covariance).

The device and the restatement must agree about which points are determined, so every input is asserted to keep clear
of the threshold on the restatement: every event either is skipped with |d| <= tau a / 16 or has d >= 16 tau a."""
import numpy as np
import pytest

import sample_at_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
SIZES_N = [1, 2, 16, 17, 33, 150]      # one row, the eight-row ring and the four-event unroll and their neighbours
SIZES_M = [1, 15, 16, 17, 150]
DRAWS = [1, 2, 3, 8, 9, 33]            # one draw (its own kernel), inside one register block, a full block, more than one, five
KINDS = R.KINDS


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


def batch(seed, B, N, M, J, K, *, per_t, per_ts, kind="mixed", gap=False, distinct=5):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct) with K columns of normals each; data
    and query grids each either the first draw's, shared by the batch, or every draw's own."""
    rng = np.random.default_rng(seed)
    draws = []
    for k in range(min(B, distinct)):
        t = None if (per_t or k == 0) else draws[0]["t"]
        if t is None:
            t = R.draw(1000 * seed + k, N, J, gap=gap)["t"]
        ts = R.make_queries(kind, t, M, rng) if (per_ts or k == 0) else draws[0]["ts"]
        dr = R.draw_with_queries(1000 * seed + k, N, J, t=t, ts=ts)
        dr["nt"], dr["ns"] = rng.standard_normal((N, K)), rng.standard_normal((M, K))
        draws.append(dr)
    idx = [b % len(draws) for b in range(B)]
    stack = lambda key: np.stack([draws[i][key] for i in idx])
    return dict(draws=draws, idx=idx, t=stack("t") if per_t else draws[0]["t"], ts=stack("ts") if per_ts else draws[0]["ts"],
                c=stack("c"), U=stack("U"), V=stack("V"), Us=stack("Us"), Vs=stack("Vs"), nt=stack("nt"), ns=stack("ns"))


ARGS = ("t", "ts", "c", "U", "V", "Us", "Vs", "nt", "ns")


def restate(dr, what):
    """The restatement's draw for one distinct input, with the condition that keeps the device and the restatement from
    disagreeing about a skip asserted on every event."""
    ft, fs, events = R.prior_draw(*[dr[k] for k in ARGS], report=True)
    for kind_e, row, skipped, ratio in events:
        assert (abs(ratio) <= R.TAU / 16) if skipped else (ratio >= 16 * R.TAU), (what, kind_e, row, skipped, ratio)
    return ft, fs


def run_case(ops, bt, what):
    """ops.prior_draw against the restatement for every distinct draw; repeats of a draw give identical bits."""
    import torch

    B = bt["U"].shape[0]
    ft, fs = ops.prior_draw(*dev(*[bt[k] for k in ARGS]))
    torch.cuda.synchronize()
    assert tuple(ft.shape) == bt["nt"].shape and tuple(fs.shape) == bt["ns"].shape
    fth, fsh = host(ft), host(fs)
    seen = set()
    for b in range(B):
        k = bt["idx"][b]
        if k in seen:   # a repeat of a draw already compared: identical inputs give identical bits
            first = bt["idx"].index(k)
            assert torch.equal(ft[b], ft[first]) and torch.equal(fs[b], fs[first]), (what, b)
            continue
        seen.add(k)
        fto, fso = restate(bt["draws"][k], (what, b))
        fo = np.concatenate([fto, fso])
        e = R.err(np.concatenate([fth[b], fsh[b]]), fo)   # (floor: max |f_o| over both grids)
        assert e <= 1.0, (what, b, e)


@pytest.mark.parametrize("J", WIDTHS)
def test_prior_draw_vs_restatement(ops, J):
    """Every width; every pair of N in {1, 2, 16, 17, 33, 150} and M in {1, 15, 16, 17, 150}; B = 3 and 70 (a padded last
    wavefront); the four combinations of shared and per-series t and ts, the six kinds of query set and K in
    {1, 2, 3, 8, 9, 33} cycling over the pairs; one draw with the 50-unit gap."""
    n = 0
    for i, N in enumerate(SIZES_N):
        for k, M in enumerate(SIZES_M):
            B = (3, 70)[(i + k) % 2]
            per_t, per_ts = bool(n & 1), bool(n & 2)
            kind = KINDS[(n + J) % len(KINDS)]
            K = DRAWS[(n + 2 * J) % len(DRAWS)]
            bt = batch(100 * J + n, B, N, M, J, K, per_t=per_t, per_ts=per_ts, kind=kind)
            run_case(ops, bt, (J, N, M, B, K, per_t, per_ts, kind))
            n += 1
    bt = batch(100 * J + 99, 3, 150, 150, J, 9, per_t=True, per_ts=True, gap=True)
    run_case(ops, bt, (J, "gap"))


@pytest.mark.parametrize("J", [8, 32])
def test_prior_draw_long_series(ops, J):
    """N = 4096 with M = 4097, and N = 4097 with M = 256, K = 2, against the restatement."""
    for N, M, per in ((4096, 4097, True), (4097, 256, False)):
        bt = batch(77 + J, 2, N, M, J, 2, per_t=per, per_ts=not per, distinct=2)
        run_case(ops, bt, (J, N, M))


@pytest.mark.parametrize("J,K", [(1, 5), (3, 1), (8, 9), (32, 33)])
def test_in_place_equals_out_of_place(ops, J, K):
    """ft is nt and fs is ns: bit for bit the out-of-place result."""
    import torch

    bt = batch(55 + J, 7, 45, 37, J, K, per_t=True, per_ts=True, kind="dups", distinct=7)
    args = dev(*[bt[k] for k in ARGS])
    ft, fs = ops.prior_draw(*args)
    nt, ns = args[-2].clone(), args[-1].clone()
    ft2, fs2 = ops.prior_draw(*args[:-2], nt, ns, ft=nt, fs=ns)
    assert ft2 is nt and fs2 is ns
    assert bool(torch.isfinite(ft).all()) and torch.equal(ft, nt) and torch.equal(fs, ns)
    assert not torch.equal(ft, args[-2])


def _gp_inputs(seed, B, N):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 0.05 * N + 5, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.4, (B, N))
    y = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3
    return x, diag, y


def _kernels():
    import torch
    from celerite2_amd import terms as T

    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kf = (T.SHOTerm(S0=np.array([1.2, 1.0, 0.8]), w0=0.9, Q=2.5) + T.RealTerm(a=np.array([0.7, 0.5, 0.9]), c=0.3)
          + T.Matern32Term(sigma=0.5, rho=2.0))
    kt = (T.SHOTerm(S0=t([1.2, 1.0, 0.8]), w0=t(0.9), Q=t(2.5), regime="under") + T.RealTerm(a=t([0.7, 0.5, 0.9]), c=0.3)
          + T.Matern32Term(sigma=t(0.5), rho=t(2.0)))
    return t, (kf, kt)


@pytest.mark.parametrize("grid", ["new", "data_and_duplicates"])
def test_sample_at_is_the_conditional_distribution(ops, grid):
    """B = 3 with per-series hyper-parameters and times, N = 12, M = 9, SHO + Real + Matern32 with float and with tensor
    hyper-parameters, a tensor mean.  Normals: the identity over (nt, ns, ne) -- 2 N + M draws -- plus one zero draw,
    K = 34 (five register blocks).  The zero draw is predict(y, t); the others minus it are A with
    A A^T = predict(y, t, return_cov=True).  Also on a query grid of data times and duplicates, where the dense
    covariance is singular and a Cholesky factor does not exist; include_mean both ways."""
    import torch
    from celerite2_amd import gp as G

    B, N, M = 3, 12, 9
    K = 2 * N + M + 1
    x, diag, y = _gp_inputs(14, B, N)
    rng = np.random.default_rng(15)
    if grid == "new":
        xs = np.sort(rng.uniform(x.min() - 1.0, x.max() + 1.0, (B, M)), axis=1)
    else:   # three data times, one of them twice more, two duplicated new times, one single
        new = rng.uniform(x.min(), x.max(), (B, 3))
        xs = np.sort(np.concatenate([x[:, [0, 5, 11, 5, 5]], new[:, [0, 0, 1, 1]]], axis=1), axis=1)
    xd, dd, yd, xsd = dev(x, diag, y, xs)
    Z = np.concatenate([np.eye(K - 1), np.zeros((K - 1, 1))], axis=1)
    normals = [torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z, (B,) + z.shape))).cuda()
               for z in (Z[:N], Z[N:N + M], Z[N + M:])]
    t, kernels = _kernels()
    for kernel in kernels:
        gp = G.GaussianProcess(kernel, xd, diag=dd, mean=t(0.3))
        k0 = gp.condition(yd, xsd)._k0()
        k0max = float(k0.max()) if torch.is_tensor(k0) else float(k0)
        for include_mean in (True, False):
            mu_o, cov_o = gp.predict(yd, xsd, return_cov=True, include_mean=include_mean)
            out = gp.sample_at(yd, xsd, size=K, normals=normals, include_mean=include_mean)
            assert tuple(out.shape) == (B, K, M)
            e = R.err(host(out[:, -1]), host(mu_o))
            assert e <= 1.0, (grid, "mean", include_mean, e)
            A = out[:, :-1] - out[:, -1:]                     # (B, K - 1, M): row k = the map applied to unit vector k
            e = R.err(host(A.transpose(1, 2) @ A), host(cov_o), floor=k0max)
            assert e <= 1.0, (grid, "covariance", include_mean, e)
        for z in normals:
            assert float(z.abs().max()) == 1.0 and float(z.sum()) == z.shape[1] * B   # the caller's normals are not written


def test_generator_and_shapes(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N, M = 5, 60, 41
    x, diag, y = _gp_inputs(16, B, N)
    xs = np.sort(np.random.default_rng(17).uniform(x.min() - 1.0, x.max() + 1.0, M))
    xd, dd, yd, xsd = dev(x, diag, y, xs)
    gp = G.GaussianProcess(T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3), xd, diag=dd, mean=0.3)
    gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)
    one = gp.sample_at(yd, xsd, generator=gen(1))
    assert tuple(one.shape) == (B, M) and bool(torch.isfinite(one).all())
    assert torch.equal(one, gp.sample_at(yd, xsd, generator=gen(1)))
    assert not torch.equal(one, gp.sample_at(yd, xsd, generator=gen(2)))
    three = gp.sample_at(yd, xsd, size=3, generator=gen(1))
    assert tuple(three.shape) == (B, 3, M)
    assert torch.equal(three, gp.sample_at(yd, xsd, size=3, generator=gen(1)))
    # the generator is consumed as randn (B, N, K), (B, M, K), (B, N, K), in that order
    g = gen(1)
    normals = [torch.randn((B, L, 3), dtype=torch.float64, device="cuda", generator=g) for L in (N, M, N)]
    assert torch.equal(three, gp.sample_at(yd, xsd, size=3, normals=normals))
    # draws scatter around the conditional mean by no more than a few standard deviations
    mu, var = gp.predict_at(yd, xsd, return_var=True)
    assert bool(((three - mu[:, None]).abs() <= 6.0 * var.sqrt()[:, None]).all())


def test_failed_series_gives_nan_and_leaves_its_neighbours_alone(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N, M, K = 9, 100, 64, 3
    x, diag, y = _gp_inputs(9, B, N)
    bad = diag.copy()
    bad[4, 37] = -50.0   # not positive definite from row 37 on
    xs = np.sort(np.random.default_rng(10).uniform(x.min() - 1.0, x.max() + 1.0, M))
    kernel = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3)
    xd, dd, bd, yd, xsd = dev(x, diag, bad, y, xs)
    good = G.GaussianProcess(kernel, xd, diag=dd, mean=0.3)
    gp = G.GaussianProcess(kernel, mean=0.3).compute(xd, diag=bd, quiet=True)
    assert host(gp._flag).tolist() == [0, 0, 0, 0, 37, 0, 0, 0, 0]
    g = torch.Generator(device="cuda").manual_seed(3)
    normals = [torch.randn((B, L, K), dtype=torch.float64, device="cuda", generator=g) for L in (N, M, N)]
    got, want = gp.sample_at(yd, xsd, size=K, normals=normals), good.sample_at(yd, xsd, size=K, normals=normals)
    ok = [b for b in range(B) if b != 4]
    assert bool(torch.isnan(got[4]).all())
    assert torch.equal(got[ok], want[ok])   # bit-identical to the same batch without the failure
    assert bool(torch.isfinite(want).all())
    assert bool(torch.isnan(gp.sample_at(yd, xsd, normals=[z[..., :1].contiguous() for z in normals])[4]).all())


def test_seventy_thousand_series(ops):
    """B = 70 000 x N = 16 x M = 8 x J = 4 x K = 1: runs, the results are finite, and the first and last series equal the
    same series run alone."""
    import torch

    B, N, M, J = 70000, 16, 8, 4
    rng = np.random.default_rng(8)
    base = R.draw_with_queries(8, N, J, M)
    scale = rng.uniform(0.5, 2.0, B)
    U, Us = base["U"][None] * scale[:, None, None], base["Us"][None] * scale[:, None, None]
    V, Vs = np.broadcast_to(base["V"][None], (B, N, J)), np.broadcast_to(base["Vs"][None], (B, M, J))
    nt, ns = rng.standard_normal((B, N, 1)), rng.standard_normal((B, M, 1))
    t, ts, c, Ud, Vd, Usd, Vsd, ntd, nsd = dev(base["t"], base["ts"], base["c"], U, V, Us, Vs, nt, ns)
    ft, fs = ops.prior_draw(t, ts, c, Ud, Vd, Usd, Vsd, ntd, nsd)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ft).all()) and bool(torch.isfinite(fs).all())
    for b in (0, B - 1):
        s = slice(b, b + 1)
        ft1, fs1 = ops.prior_draw(t, ts, c, *[x[s].contiguous() for x in (Ud, Vd, Usd, Vsd, ntd, nsd)])
        assert torch.equal(ft[b], ft1[0]) and torch.equal(fs[b], fs1[0]), b
        fto, fso = restate(dict(base, U=U[b], V=V[b], Us=Us[b], Vs=Vs[b], nt=nt[b], ns=ns[b]), b)
        assert R.err(np.concatenate([host(ft[b]), host(fs[b])]), np.concatenate([fto, fso])) <= 1.0, b


@pytest.mark.parametrize("J", [2, 8, 32])
def test_two_calls_give_identical_bits(ops, J):
    import torch

    bt = batch(21, 130, 200, 170, J, 9, per_t=True, per_ts=True, distinct=6)
    args = dev(*[bt[k] for k in ARGS])
    ft1, fs1 = ops.prior_draw(*args)
    ft2, fs2 = ops.prior_draw(*args)
    assert bool(torch.isfinite(ft1).all()) and bool(torch.isfinite(fs1).all())
    assert torch.equal(ft1, ft2) and torch.equal(fs1, fs2)


def test_graph_capture_of_prior_draw(ops):
    """One torch.cuda.graph capture of prior_draw on caller-owned ft and fs replays correctly after new normals and a new
    query grid are copied in."""
    import torch

    B, N, M, J, K = 12, 257, 190, 8, 9
    bt = batch(31, B, N, M, J, K, per_t=True, per_ts=True, distinct=B)
    args = dev(*[bt[k] for k in ARGS])
    t, ts, c, U, V, Us, Vs, nt, ns = args
    ft, fs = torch.empty_like(nt), torch.empty_like(ns)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        ops.prior_draw(*args, ft=ft, fs=fs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.prior_draw(*args, ft=ft, fs=fs)
    # new queries and new normals for the same data: every draw's own, of another kind
    rng = np.random.default_rng(32)
    new = [R.draw_with_queries(1000 * 31 + k, N, J, t=dr["t"], ts=R.make_queries("dups", dr["t"], M, rng))
           for k, dr in enumerate(bt["draws"])]
    for dr, nw in zip(bt["draws"], new):
        assert np.array_equal(dr["U"], nw["U"])   # the same data rows
        nw["nt"], nw["ns"] = rng.standard_normal((N, K)), rng.standard_normal((M, K))
    st = lambda key: np.stack([n[key] for n in new])
    ts2, Us2, Vs2, nt2, ns2 = dev(st("ts"), st("Us"), st("Vs"), st("nt"), st("ns"))
    ts.copy_(ts2); Us.copy_(Us2); Vs.copy_(Vs2); nt.copy_(nt2); ns.copy_(ns2)
    ft.zero_(); fs.zero_()
    graph.replay()
    torch.cuda.synchronize()
    ft_e, fs_e = ops.prior_draw(t, ts2, c, U, V, Us2, Vs2, nt2, ns2)
    assert torch.equal(ft, ft_e) and torch.equal(fs, fs_e)
    for b in (0, B - 1):
        fto, fso = restate(new[b], b)
        assert R.err(np.concatenate([host(ft[b]), host(fs[b])]), np.concatenate([fto, fso])) <= 1.0, b


def test_errors(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N, M, J, K = 2, 10, 7, 3, 4
    bt = batch(41, B, N, M, J, K, per_t=False, per_ts=False)
    t, ts, c, U, V, Us, Vs, nt, ns = dev(*[bt[k] for k in ARGS])
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="Invalid shape: t "):
        ops.prior_draw(t[:-1].contiguous(), ts, c, U, V, Us, Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: ts"):
        ops.prior_draw(t, ts[:-1].contiguous(), c, U, V, Us, Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: ts"):
        ops.prior_draw(t, z(B + 1, M), c, U, V, Us, Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: c"):
        ops.prior_draw(t, ts, z(B, J + 1), U, V, Us, Vs, nt, ns)
    with pytest.raises(ValueError, match="U must be"):
        ops.prior_draw(t, ts, c, U[0], V, Us, Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: V"):
        ops.prior_draw(t, ts, c, U, z(B, N, J + 1), Us, Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: Us"):
        ops.prior_draw(t, ts, c, U, V, Us[0], Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: Us"):
        ops.prior_draw(t, ts, c, U, V, z(B, M, J + 1), Vs, nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: Vs"):
        ops.prior_draw(t, ts, c, U, V, Us, z(B, M + 1, J), nt, ns)
    with pytest.raises(ValueError, match="Invalid shape: nt"):
        ops.prior_draw(t, ts, c, U, V, Us, Vs, nt[..., 0], ns)
    with pytest.raises(ValueError, match="Invalid shape: nt"):
        ops.prior_draw(t, ts, c, U, V, Us, Vs, z(B, N + 1, K), ns)
    with pytest.raises(ValueError, match="Invalid shape: ns"):
        ops.prior_draw(t, ts, c, U, V, Us, Vs, nt, z(B, M, K + 1))
    with pytest.raises(ValueError, match="Invalid shape: ft"):
        ops.prior_draw(t, ts, c, U, V, Us, Vs, nt, ns, ft=z(B, N, K + 1))
    with pytest.raises(ValueError, match="Invalid shape: fs"):
        ops.prior_draw(t, ts, c, U, V, Us, Vs, nt, ns, fs=z(B, M))
    # aliasing: only ft is nt and fs is ns
    with pytest.raises(ValueError, match="alias"):   # (K = J: a draw has the shape of U)
        ops.prior_draw(t, ts, c, U, V, Us, Vs, z(B, N, J), z(B, M, J), ft=U)
    with pytest.raises(ValueError, match="alias"):
        ops.prior_draw(t, ts, c, U, V, Us, Vs, z(B, N, J), z(B, M, J), fs=Vs)
    sq = lambda: (z(B, M, J), z(B, M, J))   # (N = M: ft and fs have one shape)
    with pytest.raises(ValueError, match="alias"):
        ops.prior_draw(ts, ts, c, *sq(), Us, Vs, z(B, M, K), z(B, M, K), ft=(same := z(B, M, K)), fs=same)
    with pytest.raises(ValueError, match="alias"):
        ops.prior_draw(ts, ts, c, *sq(), Us, Vs, (a := z(B, M, K)), (b := z(B, M, K)), ft=b, fs=a)
    # J = 40: declined by the entry point (widths 33 ... 128 have no kernel here), the usual ValueError
    with pytest.raises(ValueError, match="width not supported"):
        ops.prior_draw(z(N), z(M), z(40), z(B, N, 40), z(B, N, 40), z(B, M, 40), z(B, M, 40), z(B, N, 1), z(B, M, 1))

    x, diag, y = _gp_inputs(42, 3, 50)
    xd, dd, yd = dev(x, diag, y)
    kernel = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3)
    gp = G.GaussianProcess(kernel, xd, diag=dd)
    xs = torch.tensor([0.5, 0.4, 0.6], dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="sorted"):
        gp.sample_at(yd, xs)
    assert tuple(gp.sample_at(yd, xs, check_sorted=False).shape) == (3, 3)   # (not checked: the caller's promise)
    with pytest.raises(ValueError, match="'t' must be"):
        gp.sample_at(yd, z(4, 3))
    with pytest.raises(ValueError, match="Invalid shape: y"):
        gp.sample_at(yd[:, :-1], xs.sort().values)
    with pytest.raises(ValueError, match="Invalid shape: normals ns"):
        gp.sample_at(yd, xs.sort().values, size=2, normals=(z(3, 50, 2), z(3, 3, 1), z(3, 50, 2)))
    conv = G.GaussianProcess(T.TermConvolution(kernel, 0.05), xd, diag=dd)
    with pytest.raises(ValueError, match=r"condition\(y, t\)\.sample"):
        conv.sample_at(yd, xs.sort().values)
