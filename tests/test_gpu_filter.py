# -*- coding: utf-8 -*-
"""GPU checks of the streaming updates: ops.filter_append / filter_absorb / filter_forecast (include/celerite2_amd_filter.h,
csrc/c2_filter.hip) at every group size, and stream.Filter / GaussianProcess.filter on top of them.

References: the numpy restatement (tests/filter_ref.py, pinned to the reference's recursions and to dense algebra by
tests/test_filter.py), the device's own ops.factor + ops.solve_lower of the whole series, gp.log_likelihood, dense
conditioning and gp.predict_at.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (variances: the
floor relative to max(k(0), max D); means: relative to max(|mu_o|, |y|)).  Every dense input has a condition number <= 1e6,
asserted per draw."""
import functools

import numpy as np
import pytest

import filter_ref as F

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 5, 8, 16, 17, 32]
HEAD_ROWS = 7   # rows absorbed before the M rows under test


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


def check(key, x, xo, floor=None):
    e = F.err(host(x) if hasattr(x, "cpu") else x, xo, floor)
    assert e <= 1.0, (key, e)


@functools.lru_cache(maxsize=None)
def reference(seed, N, J, gap=False):
    """One seeded draw with its factors, its z and the chain of states: states[n] = the state behind row n - 1."""
    cs = F.draw(seed, N, J, gap=gap)
    cond = np.linalg.cond(F.dense(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"]))
    assert cond <= 1e6, (seed, N, J, cond)
    cs["d"], cs["W"] = F.factor(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
    cs["z"] = F.solve_lower(cs["t"], cs["c"], cs["U"], cs["W"], cs["y"])
    states = [F.empty(J)]
    for n in range(N):
        states.append(F.append(states[-1], cs["c"], *(cs[k][n:n + 1] for k in "taUVy"))[0])
    cs["states"] = states
    return cs


def batch(seed, B, N, J, *, distinct=5, gap=False):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct), each on its own grid."""
    draws = [reference(1000 * seed + k, N, J, gap) for k in range(min(B, distinct))]
    idx = [b % len(draws) for b in range(B)]
    bt = {key: np.stack([draws[i][key] for i in idx]) for key in "tcaUVydWz"}
    bt.update(draws=draws, idx=idx, B=B, N=N, J=J)
    return bt


def states_of(bt, n):
    return np.stack([bt["draws"][i]["states"][n] for i in bt["idx"]])


def check_state(key, st, st_o, J):
    st = host(st)
    assert np.array_equal(st[:, :2], st_o[:, :2]), key                      # t_last and n: exact
    check((key, "sums"), st[:, 2:4], st_o[:, 2:4])
    check((key, "F"), st[:, 4:4 + J], st_o[:, 4:4 + J])
    check((key, "S"), st[:, 4 + J:], st_o[:, 4 + J:])
    S = st[:, 4 + J:].reshape(-1, J, J)
    assert np.array_equal(S, S.transpose(0, 2, 1)), key                     # both triangles, equal to the bit


def rows(bt, lo, hi):
    return dev(*(bt[k][:, lo:hi] for k in "taUVy"))


# ---- group and wave boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", WIDTHS)
def test_group_and_wave_boundaries(ops, J):
    """Every group size (J and the next power of two), partial wavefronts (B = 1, 3, 65, 130) and M on both sides of 16:
    HEAD_ROWS rows from the empty state, then M rows; absorb of the same head from its factors gives the same state."""
    for B in (1, 3, 65, 130):
        for M in (1, 2, 17, 33):
            n0, N = HEAD_ROWS, HEAD_ROWS + M
            bt = batch(J, B, N, J)
            key = (J, B, M)
            c, = dev(bt["c"])
            t, a, U, V, y = rows(bt, 0, n0)
            st, d, W, z, flag = ops.filter_append(ops.filter_init(B, J, "cuda"), t, c, a, U, V, y)
            assert int(flag.abs().sum()) == 0, key
            check_state((key, "head"), st, states_of(bt, n0), J)
            t, Wd, dd, zd = dev(bt["t"][:, :n0], bt["W"][:, :n0], bt["d"][:, :n0], bt["z"][:, :n0])
            check_state((key, "absorb"), ops.filter_absorb(ops.filter_init(B, J, "cuda"), t, c, Wd, dd, zd), states_of(bt, n0), J)
            t, a, U, V, y = rows(bt, n0, N)
            st1, d, W, z, flag = ops.filter_append(st, t, c, a, U, V, y)
            assert int(flag.abs().sum()) == 0, key
            check((key, "d"), d, bt["d"][:, n0:])
            check((key, "W"), W, bt["W"][:, n0:])
            check((key, "z"), z, bt["z"][:, n0:])
            check_state((key, "tail"), st1, states_of(bt, N), J)
            check_state((key, "input kept"), st, states_of(bt, n0), J)   # out was a tensor of its own


# ---- a whole series in chunks, against the device's own factor + solve_lower --------------------------------------------
CUTS = [0, 1, 2, 7, 23, 40, 150]   # chunks of 1, 1, 5, 16, 17 and the rest


@pytest.mark.parametrize("J", [3, 8, 32])
def test_whole_series_against_device_ops(ops, J):
    import torch

    bt = batch(40 + J, 5, 150, J, gap=(J == 8))
    t, c, a, U, V, y = dev(*(bt[k] for k in "tcaUVy"))
    d_o, W_o, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    z_o = ops.solve_lower(t, c, U, W_o, y[..., None].contiguous())[..., 0]
    st = ops.filter_init(5, J, "cuda")
    parts = []
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        tm, am, Um, Vm, ym = (x[:, lo:hi].contiguous() for x in (t, a, U, V, y))
        _, d, W, z, flag = ops.filter_append(st, tm, c, am, Um, Vm, ym, out=st)
        assert int(flag.abs().sum()) == 0
        parts.append((d, W, z))
    d, W, z = (torch.cat([p[i] for p in parts], dim=1) for i in range(3))
    check("d", d, host(d_o))
    check("W", W, host(W_o))
    check("z", z, host(z_o))
    check_state("end", st, states_of(bt, 150), J)
    ll_o = -0.5 * ((z_o * z_o / d_o).sum(dim=1) + torch.log(d_o).sum(dim=1) + 150 * np.log(2 * np.pi))
    ll = -0.5 * (st[:, 3] + st[:, 2] + st[:, 1] * np.log(2 * np.pi))
    check("ll", ll, host(ll_o))


# ---- stream.Filter and gp.filter -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gp_case():
    """B = 4 series of N = 150 rows on their own grids under an SHO + real kernel, the GP of the whole series and of its
    first 100 rows."""
    from celerite2_amd import gp as G, terms

    rng = np.random.default_rng(77)
    B, N, n0 = 4, 150, 100
    t = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    yerr = rng.uniform(0.2, 0.5, (B, N))
    y = rng.normal(size=(B, N)) + 0.3
    kernel = terms.SHOTerm(S0=1.2, w0=1.1, Q=2.5) + terms.RealTerm(a=0.8, c=0.3)
    td, ed, yd = dev(t, yerr, y)
    full = G.GaussianProcess(kernel, td, yerr=ed, mean=0.3)
    for b in range(B):
        K = F.dense(t[b], host(full._c), host(full._a[b]), host(full._U[b]), host(full._V[b]))
        assert np.linalg.cond(K) <= 1e6
    head = G.GaussianProcess(kernel, td[:, :n0].contiguous(), yerr=ed[:, :n0].contiguous(), mean=0.3)
    return dict(B=B, N=N, n0=n0, t=td, yerr=ed, y=yd, kernel=kernel, full=full, head=head, k0=1.2 * 1.1 * 2.5 + 0.8)


def _full_z(g):
    from celerite2_amd import ops as o
    gp = g["full"]
    return o.solve_lower(gp._t, gp._c, gp._U, gp._W, (g["y"] - 0.3)[..., None].contiguous())[..., 0]


def test_filter_from_nothing_is_the_gp(gp_case):
    """Filter.empty + chunked appends: innovations and variances are the z and d of gp.compute on the whole series, the
    log-likelihood is gp.log_likelihood."""
    import torch
    from celerite2_amd.stream import Filter

    g = gp_case
    flt = Filter.empty(g["kernel"], g["B"], mean=0.3)
    zs, ds = [], []
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        upd = flt.append(g["t"][:, lo:hi], g["y"][:, lo:hi], yerr=g["yerr"][:, lo:hi])
        assert int(upd.flag.abs().sum()) == 0
        zs.append(upd.innovation)
        ds.append(upd.variance)
        assert torch.equal(upd.score, upd.innovation / torch.sqrt(upd.variance))
    check("d", torch.cat(ds, dim=1), host(g["full"]._d))
    check("z", torch.cat(zs, dim=1), host(_full_z(g)))
    check("ll", flt.log_likelihood, host(g["full"].log_likelihood(g["y"])))
    assert torch.equal(flt.n, torch.full((g["B"],), g["N"], dtype=torch.int64, device="cuda"))
    assert torch.equal(flt.t_last, g["t"][:, -1])


def test_filter_from_gp_filter(gp_case):
    """gp.filter(y) on the head, then the tail appended: the same d, z and log-likelihood as the GP of the whole series;
    clone() is independent of the original."""
    import torch

    g = gp_case
    n0 = g["n0"]
    flt = g["head"].filter(g["y"][:, :n0].contiguous())
    check("ll of the head", flt.log_likelihood, host(g["head"].log_likelihood(g["y"][:, :n0].contiguous())))
    keep = flt.clone()
    before = keep.state.clone()
    upd = flt.append(g["t"][:, n0:], g["y"][:, n0:], yerr=g["yerr"][:, n0:])
    assert int(upd.flag.abs().sum()) == 0
    check("d", upd.variance, host(g["full"]._d)[:, n0:])
    check("z", upd.innovation, host(_full_z(g))[:, n0:])
    check("ll", flt.log_likelihood, host(g["full"].log_likelihood(g["y"])))
    assert torch.equal(keep.state, before) and not torch.equal(flt.state, before)
    with pytest.raises(ValueError, match="sorted"):
        flt.append(g["t"][:, n0:], g["y"][:, n0:], yerr=g["yerr"][:, n0:])   # before t_last now
    with pytest.raises(ValueError, match="sorted"):
        keep.append(g["t"][:, n0:].flip(1), g["y"][:, n0:], yerr=g["yerr"][:, n0:])


def test_forecast_against_predict_at(gp_case):
    """Beyond the end of the data Filter.forecast is gp.predict_at (mean and variance) plus the query's own white noise."""
    import torch

    g = gp_case
    flt = g["full"].filter(g["y"])
    ts = g["t"][:, -1:] + torch.linspace(0.25, 6.25, 13, dtype=torch.float64, device="cuda")[None, :]
    diag = torch.full_like(ts, 0.04)
    mu, var = flt.forecast(ts, diag=diag)
    mu_o, var_o = g["full"].predict_at(g["y"], ts, return_var=True)
    floor = max(float(mu_o.abs().max()), float(g["y"].abs().max()))
    check("mu", mu, host(mu_o), floor)
    check("var", var, host(var_o) + 0.04, max(g["k0"], float(g["yerr"].max()) ** 2))
    mu0, _ = flt.forecast(ts, include_mean=False)
    check("mu without mean", mu0, host(mu_o) - 0.3, floor)
    with pytest.raises(ValueError, match="before the last"):
        flt.forecast(ts - 1.0)


def test_forecast_against_dense_conditioning(ops):
    """ops.filter_forecast from the state behind row n0 - 1 at every later row of the series: the dense conditional of that
    row on the first n0 rows.  Widths on both sides of a group size; more query rows than 16."""
    for J, N in ((1, 40), (5, 70), (8, 150), (17, 60)):
        bt = batch(70 + J, 3, N, J)
        n0 = N // 2 + 1
        st, = dev(states_of(bt, n0))
        t, c, a, U = dev(bt["t"][:, n0:], bt["c"], bt["a"][:, n0:], bt["U"][:, n0:])
        mu, var = ops.filter_forecast(st, t, c, a, U)
        for b in range(3):
            cs = bt["draws"][bt["idx"][b]]
            K = F.dense(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
            mu_o, var_o = F.dense_forecast(K, cs["y"], n0)
            check((J, b, "mu"), mu[b], mu_o, max(np.abs(mu_o).max(), np.abs(cs["y"]).max()))
            check((J, b, "var"), var[b], var_o)
        empty_mu, empty_var = ops.filter_forecast(ops.filter_init(3, J, "cuda"), t, c, a, U)
        assert not bool(empty_mu.any()) and bool((empty_var == a).all())   # nothing absorbed: the prior


# ---- ragged counts, in place, sentinels -----------------------------------------------------------------------------------
def test_ragged_counts_and_in_place(ops):
    """count includes 0 and M: rows beyond count are untouched in sentinel-filled outputs, a count-0 state stays
    bit-identical (into a tensor of its own and in place), the rows taken are the restatement's; `out is state` gives the
    bits of the out-of-place call."""
    import torch

    J, M, n0 = 5, 6, HEAD_ROWS
    counts = np.array([0, 6, 2, 0, 1, 6, 3, 5, 0, 4], dtype=np.int32)
    B = len(counts)
    bt = batch(91, B, n0 + M, J)
    st0, c, cnt = dev(states_of(bt, n0), bt["c"], counts)
    t, a, U, V, y = rows(bt, n0, n0 + M)
    sent = -7.0
    d, W, z = (torch.full(s, sent, dtype=torch.float64, device="cuda") for s in ((B, M), (B, M, J), (B, M)))
    st1, d, W, z, flag = ops.filter_append(st0, t, c, a, U, V, y, count=cnt, d=d, W=W, z=z)
    assert int(flag.abs().sum()) == 0
    taken = np.arange(M)[None, :] < counts[:, None]
    for x, key in ((d, "d"), (W, "W"), (z, "z")):
        x, xo = host(x), bt[key][:, n0:]
        assert np.all(x[~taken] == sent), key
        check(key, x[taken], xo[taken])
    want = np.stack([bt["draws"][i]["states"][n0 + k] for i, k in zip(bt["idx"], counts)])
    check_state("ragged", st1, want, J)
    assert torch.equal(st1[cnt == 0], st0[cnt == 0])
    # absorb and forecast take count too
    Wd, dd, zd = dev(bt["W"][:, n0:], bt["d"][:, n0:], bt["z"][:, n0:])
    st2 = ops.filter_absorb(st0, t, c, Wd, dd, zd, count=cnt)
    check_state("ragged absorb", st2, want, J)
    assert torch.equal(st2[cnt == 0], st0[cnt == 0])
    mu, var = (torch.full((B, M), sent, dtype=torch.float64, device="cuda") for _ in range(2))
    ops.filter_forecast(st0, t, c, a, U, count=cnt, mu=mu, var=var)
    full_mu, full_var = ops.filter_forecast(st0, t, c, a, U)
    tk = torch.from_numpy(taken).cuda()
    assert bool((mu[~tk] == sent).all()) and bool((var[~tk] == sent).all())
    assert torch.equal(mu[tk], full_mu[tk]) and torch.equal(var[tk], full_var[tk])
    # in place
    st_in = st0.clone()
    out, d2, W2, z2, _ = ops.filter_append(st_in, t, c, a, U, V, y, count=cnt, out=st_in)
    assert out is st_in and torch.equal(st_in, st1)
    assert torch.equal(d2[tk], d[tk]) and torch.equal(z2[tk], z[tk])
    st_in = st0.clone()
    assert ops.filter_absorb(st_in, t, c, Wd, dd, zd, count=cnt, out=st_in) is st_in and torch.equal(st_in, st2)


def test_empty_state_far_below_t_last(ops):
    """n == 0 and a first time of -1e4 under a stale t_last of +1e6: exp would overflow and 0 * inf poison S; the result is
    finite and equal to row 0 of factor (d = a, W = V / a, z = y)."""
    import torch

    for J in (2, 8):
        bt = batch(95, 3, 4, J)
        st = ops.filter_init(3, J, "cuda")
        st[:, 0] = 1e6
        t, c, a, U, V, y = dev(bt["t"] - 1e4, bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
        st, d, W, z, flag = ops.filter_append(st, t, c, a, U, V, y)
        assert int(flag.abs().sum()) == 0 and bool(torch.isfinite(st).all())
        assert torch.equal(d[:, 0], a[:, 0]) and torch.equal(z[:, 0], y[:, 0])
        check("W0", W[:, 0], bt["V"][:, 0] / bt["a"][:, 0, None])
        check("d", d, bt["d"])
        check("W", W, bt["W"])


def test_failure_is_local(ops):
    """A row whose `a` makes d <= 0: the flag is its 1-based index, the rows before it (and its own d) are written, the
    series' state is bitwise unchanged -- in place and into a tensor of its own -- and its neighbours in the same wavefront
    equal their run without it.  A NaN pivot passes the test."""
    import torch

    J, M, n0, B = 3, 6, HEAD_ROWS, 16   # G = 4: all 16 series in one wavefront
    bt = batch(97, B, n0 + M, J)
    st0, c = dev(states_of(bt, n0), bt["c"])
    t, a, U, V, y = rows(bt, n0, n0 + M)
    good = ops.filter_append(st0, t, c, a, U, V, y)
    bad_a = a.clone()
    bad_a[5, 2] = -1.0
    bad_a[9, 0] = -1.0
    bad_a[12, 3] = float("nan")
    sent = -7.0
    for in_place in (False, True):
        st_in = st0.clone()
        d, W, z = (torch.full(s, sent, dtype=torch.float64, device="cuda") for s in ((B, M), (B, M, J), (B, M)))
        st1, d, W, z, flag = ops.filter_append(st_in, t, c, bad_a, U, V, y, out=st_in if in_place else None, d=d, W=W, z=z)
        want = torch.zeros(B, dtype=torch.int32, device="cuda")
        want[5], want[9] = 3, 1
        assert torch.equal(flag, want)
        assert torch.equal(st1[5], st0[5]) and torch.equal(st1[9], st0[9])
        ok = torch.ones(B, dtype=torch.bool, device="cuda")
        ok[[5, 9, 12]] = False
        for x, xg in zip((st1, d, W, z), good):
            assert torch.equal(x[ok], xg[ok])
        assert torch.equal(d[5, :2], good[1][5, :2]) and torch.equal(W[5, :2], good[2][5, :2]) and torch.equal(z[5, :2], good[3][5, :2])
        assert float(d[5, 2]) <= 0 and bool((d[5, 3:] == sent).all()) and bool((W[5, 2:] == sent).all()) and bool((z[5, 2:] == sent).all())
        assert float(d[9, 0]) <= 0 and bool((d[9, 1:] == sent).all()) and bool((z[9] == sent).all())
        assert torch.equal(d[12, :3], good[1][12, :3]) and bool(torch.isnan(d[12, 3:]).all()) and bool(torch.isnan(st1[12, 2:]).all())


def test_two_calls_give_identical_bits(ops):
    import torch

    for J, B in ((8, 130), (17, 65)):
        bt = batch(99, B, HEAD_ROWS + 17, J)
        st0, c = dev(states_of(bt, HEAD_ROWS), bt["c"])
        t, a, U, V, y = rows(bt, HEAD_ROWS, HEAD_ROWS + 17)
        one, two = ops.filter_append(st0, t, c, a, U, V, y), ops.filter_append(st0, t, c, a, U, V, y)
        for x, x2 in zip(one, two):
            assert torch.equal(x, x2)
        f1, f2 = ops.filter_forecast(one[0], t + 40.0, c, a, U), ops.filter_forecast(two[0], t + 40.0, c, a, U)
        assert torch.equal(f1[0], f2[0]) and torch.equal(f1[1], f2[1])


# ---- offsets and strides ----------------------------------------------------------------------------------------------------
def _odd(x):
    """A contiguous copy of x that starts at an odd element (8 mod 16 bytes) of its buffer."""
    import torch

    buf = torch.empty(x.numel() + 3, dtype=x.dtype, device=x.device)
    off = 1 if buf.data_ptr() % 16 == 0 else 2
    if x.dtype == torch.int32:
        off = 1
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert x.dtype == torch.int32 or v.data_ptr() % 16 == 8
    return v


def test_odd_offsets_and_shared_strides(ops):
    """Every array starting at an odd element gives the bits of the aligned call; t and c shared by the batch (stride 0) give
    the bits of the same values repeated per series.  One draw, B series that differ in their noise and their data."""
    import torch

    J, M, n0, B = 5, 9, HEAD_ROWS, 7
    cs = reference(3100, n0 + M, J)
    scale = 1.0 + np.arange(B)
    A, Y = cs["a"][None, :] + 0.01 * scale[:, None], cs["y"][None, :] * scale[:, None]
    tile = lambda x: np.ascontiguousarray(np.broadcast_to(x, (B,) + x.shape))
    heads = [F.append(F.empty(J), cs["c"], cs["t"][:n0], A[b, :n0], cs["U"][:n0], cs["V"][:n0], Y[b, :n0]) for b in range(B)]
    assert all(h[4] == 0 for h in heads)
    st0, t1, c1, tB, cB = dev(np.stack([h[0] for h in heads]), cs["t"][n0:], cs["c"], tile(cs["t"][n0:]), tile(cs["c"]))
    a, U, V, y = dev(A[:, n0:], tile(cs["U"][n0:]), tile(cs["V"][n0:]), Y[:, n0:])
    cnt, = dev(np.array([9, 0, 4, 9, 1, 7, 2], dtype=np.int32))
    tk = torch.arange(M, device="cuda")[None, :] < cnt[:, None]
    sent = lambda x: torch.full_like(x, -7.0)

    def same(got, want):   # state and flag whole, d / W / z in the rows taken (the rest was never written)
        for x, xw in zip(got, want):
            rowwise = x.dim() >= 2 and x.shape[1] == M
            assert torch.equal(x[tk], xw[tk]) if rowwise else torch.equal(x, xw)

    base = ops.filter_append(st0, tB, cB, a, U, V, y, count=cnt)
    assert int(base[4].abs().sum()) == 0
    same(ops.filter_append(st0, t1, c1, a, U, V, y, count=cnt), base)
    same(ops.filter_append(_odd(st0), _odd(tB), _odd(cB), _odd(a), _odd(U), _odd(V), _odd(y), count=_odd(cnt),
                           out=_odd(torch.empty_like(st0)), d=_odd(sent(a)), W=_odd(sent(V)), z=_odd(sent(y))), base)
    same(ops.filter_append(_odd(st0), _odd(t1), _odd(c1), _odd(a), _odd(U), _odd(V), _odd(y), count=_odd(cnt)), base)
    _, d, W, z, _ = ops.filter_append(st0, tB, cB, a, U, V, y)
    absorbed = ops.filter_absorb(st0, tB, cB, W, d, z)
    assert torch.equal(ops.filter_absorb(st0, t1, c1, W, d, z), absorbed)
    assert torch.equal(ops.filter_absorb(_odd(st0), _odd(t1), _odd(c1), _odd(W), _odd(d), _odd(z), out=_odd(torch.empty_like(st0))), absorbed)
    fc = ops.filter_forecast(st0, tB, cB, a, U)
    for got in (ops.filter_forecast(st0, t1, c1, a, U),
                ops.filter_forecast(_odd(st0), _odd(t1), _odd(c1), _odd(a), _odd(U), mu=_odd(sent(a)), var=_odd(sent(a)))):
        assert torch.equal(got[0], fc[0]) and torch.equal(got[1], fc[1])
