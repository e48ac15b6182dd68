# -*- coding: utf-8 -*-
"""GPU checks of the forecast sample paths: ops.filter_draw (include/celerite2_amd_filter_draw.h, csrc/c2_filter_draw.hip) at
every group size and on both sides of a pass of draws, and stream.Filter.sample_forecast / forecast_joint_log_density on top.

References: the numpy restatement (tests/filter_draw_ref.py, pinned to dense conditioning -- mu_c + cholesky(Sigma_c) @ eps --
by tests/test_filter_draw.py), ops.filter_append for the bits of d and flag, dense conditioning itself, and torch's own
float64 derivative of the dense conditional density.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o|
(inverse_diag_ref.err); the draws are those of tests/test_gpu_filter.py (condition number <= 1e6, asserted there per draw),
every other dense input is asserted here."""
import numpy as np
import pytest

import filter_draw_ref as D
import filter_ref as F
from test_gpu_filter import HEAD_ROWS, WIDTHS, _odd, batch, dev, host, reference, states_of
from test_gpu_filter_rev import _kernel_case, check
from test_gpu_filter_stream_rev import N0, _compare, _fed

pytestmark = pytest.mark.gpu
SENT = -7.0


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


def case(bt, n0, M, K, seed=0):
    """The restatement's state behind row n0 - 1, the M rows behind it, and K columns of normals per row (host arrays)."""
    h = dict(state=states_of(bt, n0), c=bt["c"], **{k: bt[k][:, n0:n0 + M] for k in "taUV"})
    h["eps"] = np.random.default_rng(1000 * seed + K).normal(size=(bt["B"], M, K))
    return h


def restated(h, counts=None, eps=None):
    """D.draw_paths per series -> paths (B, M, K), d (B, M) (NaN where nothing is written) and flag (B,)."""
    eps = h["eps"] if eps is None else eps
    B, M, K = eps.shape
    paths, d, flag = np.full((B, M, K), np.nan), np.full((B, M), np.nan), np.zeros(B, dtype=np.int32)
    for b in range(B):
        m = M if counts is None else int(counts[b])
        t = h["t"] if h["t"].ndim == 1 else h["t"][b]
        c = h["c"] if h["c"].ndim == 1 else h["c"][b]
        paths[b, :m], d[b, :m], flag[b] = D.draw_paths(h["state"][b], c, t[:m], h["a"][b, :m], h["U"][b, :m], h["V"][b, :m],
                                                       eps[b, :m])
    return paths, d, flag


def on_device(h):
    return {k: dev(v)[0] for k, v in h.items()}


def call(ops, g, eps=None, **kw):
    return ops.filter_draw(g["state"], g["t"], g["c"], g["a"], g["U"], g["V"], g["eps"] if eps is None else eps, **kw)


def check_draw(key, got, want):
    paths, d, flag = got
    paths_o, d_o, flag_o = want
    assert np.array_equal(host(flag), flag_o), key
    written = ~np.isnan(d_o)
    check((key, "d"), host(d)[written], d_o[written])
    written = ~np.isnan(paths_o)
    check((key, "paths"), host(paths)[written], paths_o[written])


def append_d_flag(ops, g, seed=5):
    """d and flag of ops.filter_append on the same rows with an arbitrary y."""
    import torch

    y = torch.from_numpy(np.random.default_rng(seed).normal(size=tuple(g["a"].shape))).cuda()
    _, d, _, _, flag = ops.filter_append(g["state"], g["t"], g["c"], g["a"], g["U"], g["V"], y)
    return d, flag


# ---- group and wave boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", WIDTHS)
def test_group_and_wave_boundaries(ops, J):
    """Every group size (J and the next power of two), partial wavefronts (B = 1, 3, 65, 130) and M on both sides of 16 and
    32 at K = 3, from a state with HEAD_ROWS rows: paths and d against the restatement; d and flag have the bits of
    ops.filter_append on the same rows (with an arbitrary y); the state is bit for bit as before."""
    import torch

    for B in (1, 3, 65, 130):
        for M in (1, 2, 17, 33):
            key = (J, B, M)
            h = case(batch(J, B, HEAD_ROWS + M, J), HEAD_ROWS, M, 3, seed=J)
            g = on_device(h)
            before = g["state"].clone()
            got = call(ops, g)
            check_draw(key, got, restated(h))
            d_a, flag_a = append_d_flag(ops, g)
            assert torch.equal(got[1], d_a) and torch.equal(got[2], flag_a), key
            assert torch.equal(g["state"], before), key


@pytest.mark.parametrize("J", [2, 8, 17])
def test_draw_counts_around_a_pass(ops, J):
    """K on both sides of the draws one pass carries (KC = ops.filter_draw_chunk(J)) and beyond two passes, at B = 65 and
    M = 17: paths and d against the restatement, d and flag the append's bits at every K."""
    import torch

    KC = ops.filter_draw_chunk(J)
    assert KC >= 1
    B, M = 65, 17
    bt = batch(J, B, HEAD_ROWS + M, J)
    for K in sorted({1, 17, 70, KC - 1, KC, KC + 1, 2 * KC + 3} - {0}):
        h = case(bt, HEAD_ROWS, M, K, seed=50 + J)
        g = on_device(h)
        got = call(ops, g)
        check_draw((J, K), got, restated(h))
        d_a, flag_a = append_d_flag(ops, g)
        assert torch.equal(got[1], d_a) and torch.equal(got[2], flag_a), (J, K)


def test_a_draw_does_not_depend_on_its_slot(ops):
    """Draw k of a K = 70 call has the bits of the same normals drawn alone with K = 1, wherever k falls in a pass; two calls
    give identical bits; the state is not written."""
    import torch

    for J, B in ((1, 70), (3, 33), (8, 65), (32, 5)):
        M, K = 17, 70
        h = case(batch(J, B, HEAD_ROWS + M, J), HEAD_ROWS, M, K, seed=60 + J)
        g = on_device(h)
        before = g["state"].clone()
        one, two = call(ops, g), call(ops, g)
        for x, x2 in zip(one, two):
            assert torch.equal(x, x2), J
        assert torch.equal(g["state"], before), J
        KC = ops.filter_draw_chunk(J)
        for k in sorted({0, 1, 5, KC - 1, KC, KC + 1, 2 * KC, K - 1}):
            alone = call(ops, g, g["eps"][:, :, k:k + 1].contiguous())
            assert torch.equal(alone[0][:, :, 0], one[0][:, :, k]), (J, k)
            assert torch.equal(alone[1], one[1]) and torch.equal(alone[2], one[2]), (J, k)


# ---- ragged counts, sentinels -------------------------------------------------------------------------------------------------
def test_ragged_counts_in_sentinel_filled_outputs(ops):
    """count includes 0 and M: nothing beyond the count is touched in sentinel-filled paths and d, the rows taken are the
    restatement's and have the bits of the call without a count."""
    import torch

    for J, K in ((5, 3), (2, 37)):
        M = 6
        counts = np.array([0, 6, 2, 0, 1, 6, 3, 5, 0, 4], dtype=np.int32)
        B = len(counts)
        h = case(batch(91, B, HEAD_ROWS + M, J), HEAD_ROWS, M, K, seed=70)
        g = on_device(h)
        cnt, = dev(counts)
        paths = torch.full((B, M, K), SENT, dtype=torch.float64, device="cuda")
        d = torch.full((B, M), SENT, dtype=torch.float64, device="cuda")
        got = call(ops, g, count=cnt, paths=paths, d=d)
        assert got[0] is paths and got[1] is d and int(got[2].abs().sum()) == 0
        taken = torch.arange(M, device="cuda")[None, :] < cnt[:, None]
        assert bool((paths[~taken] == SENT).all()) and bool((d[~taken] == SENT).all())
        check_draw((J, "ragged"), got, restated(h, counts))
        full = call(ops, g)
        assert torch.equal(paths[taken], full[0][taken]) and torch.equal(d[taken], full[1][taken])


def test_failure_is_local(ops):
    """A row whose `a` makes d <= 0: the flag is its 1-based index, the rows before it (and its own d) are written and nothing
    behind them, and the series' neighbours in the same wavefront equal their run without it.  A NaN pivot passes the test,
    as in the append.  Also beyond one pass of draws."""
    import torch

    J, M, B = 3, 6, 16   # G = 4: all 16 series in one wavefront
    for K in (5, 70):
        h = case(batch(97, B, HEAD_ROWS + M, J), HEAD_ROWS, M, K, seed=80)
        g = on_device(h)
        good = call(ops, g)
        assert int(good[2].abs().sum()) == 0
        bad = dict(g, a=g["a"].clone())
        bad["a"][5, 2] = -1.0
        bad["a"][9, 0] = -1.0
        bad["a"][12, 3] = float("nan")
        paths = torch.full((B, M, K), SENT, dtype=torch.float64, device="cuda")
        d = torch.full((B, M), SENT, dtype=torch.float64, device="cuda")
        _, _, flag = call(ops, bad, paths=paths, d=d)
        want = torch.zeros(B, dtype=torch.int32, device="cuda")
        want[5], want[9] = 3, 1
        assert torch.equal(flag, want)
        d_a, flag_a = append_d_flag(ops, bad)
        assert torch.equal(flag, flag_a) and torch.equal(d[5, :3], d_a[5, :3]) and torch.equal(d[9, :1], d_a[9, :1])
        ok = torch.ones(B, dtype=torch.bool, device="cuda")
        ok[[5, 9, 12]] = False
        assert torch.equal(paths[ok], good[0][ok]) and torch.equal(d[ok], good[1][ok])
        assert torch.equal(paths[5, :2], good[0][5, :2]) and torch.equal(d[5, :2], good[1][5, :2])
        assert float(d[5, 2]) <= 0 and bool((d[5, 3:] == SENT).all()) and bool((paths[5, 2:] == SENT).all())
        assert float(d[9, 0]) <= 0 and bool((d[9, 1:] == SENT).all()) and bool((paths[9] == SENT).all())
        assert torch.equal(paths[12, :3], good[0][12, :3]) and torch.equal(d[12, :3], good[1][12, :3])
        assert bool(torch.isnan(d[12, 3:]).all()) and bool(torch.isnan(paths[12, 3:]).all())


# ---- offsets and strides ----------------------------------------------------------------------------------------------------
def test_odd_offsets_and_shared_strides(ops):
    """Every array starting at an odd element gives the bits of the aligned call; t and c shared by the batch (stride 0) give
    the bits of the same values repeated per series.  One draw, B series that differ in their noise and their data."""
    import torch

    J, M, n0, B, K = 5, 9, HEAD_ROWS, 7, 35
    cs = reference(3100, n0 + M, J)
    scale = 1.0 + np.arange(B)
    A, Y = cs["a"][None, :] + 0.01 * scale[:, None], cs["y"][None, :] * scale[:, None]
    tile = lambda x: np.ascontiguousarray(np.broadcast_to(x, (B,) + x.shape))
    heads = [F.append(F.empty(J), cs["c"], cs["t"][:n0], A[b, :n0], cs["U"][:n0], cs["V"][:n0], Y[b, :n0]) for b in range(B)]
    assert all(h[4] == 0 for h in heads)
    st0, t1, c1, tB, cB = dev(np.stack([h[0] for h in heads]), cs["t"][n0:], cs["c"], tile(cs["t"][n0:]), tile(cs["c"]))
    a, U, V, eps = dev(A[:, n0:], tile(cs["U"][n0:]), tile(cs["V"][n0:]), np.random.default_rng(9).normal(size=(B, M, K)))
    cnt, = dev(np.array([9, 0, 4, 9, 1, 7, 2], dtype=np.int32))
    tk = torch.arange(M, device="cuda")[None, :] < cnt[:, None]
    sent = lambda x: torch.full_like(x, SENT)

    def same(got, want):   # flag whole, paths and d in the rows taken (the rest was never written)
        assert torch.equal(got[0][tk], want[0][tk]) and torch.equal(got[1][tk], want[1][tk]) and torch.equal(got[2], want[2])

    base = ops.filter_draw(st0, tB, cB, a, U, V, eps, count=cnt)
    assert int(base[2].abs().sum()) == 0
    h = dict(state=host(st0), t=cs["t"][n0:], c=cs["c"], a=A[:, n0:], U=host(U), V=host(V), eps=host(eps))
    check_draw("shared", base, restated(h, host(cnt)))
    same(ops.filter_draw(st0, t1, c1, a, U, V, eps, count=cnt), base)
    same(ops.filter_draw(_odd(st0), _odd(tB), _odd(cB), _odd(a), _odd(U), _odd(V), _odd(eps), count=_odd(cnt),
                         paths=_odd(sent(eps)), d=_odd(sent(a))), base)
    same(ops.filter_draw(_odd(st0), _odd(t1), _odd(c1), _odd(a), _odd(U), _odd(V), _odd(eps), count=_odd(cnt)), base)


def test_empty_state_far_below_t_last(ops):
    """n == 0 and a first time of -1e4 under a stale t_last of +1e6: p := 0, the paths are a prior draw (the restatement's,
    which tests/test_filter_draw.py pins to cholesky(K) @ eps) and d is that of factor."""
    import torch

    for J in (2, 8):
        bt = batch(95, 3, 4, J)
        h = case(bt, 0, 4, 6, seed=90)
        h["state"] = h["state"].copy()
        h["state"][:, 0] = 1e6
        h["t"] = h["t"] - 1e4
        got = call(ops, on_device(h))
        assert bool(torch.isfinite(got[0]).all())
        check_draw((J, "empty"), got, restated(h))
        check((J, "d"), got[1], bt["d"])


# ---- a batch beyond 65535 series ---------------------------------------------------------------------------------------------
def test_large_batch(ops):
    """B = 70000 at J = 2, M = 2, K = 3: seven distinct series tiled, every series against its distinct one's restatement,
    replicas bit-identical (the entry point is not in the census of tests/large_batch_cases.py)."""
    import torch

    J, M, K, R, B = 2, 2, 3, 7, 70000
    h = case(batch(93, R, HEAD_ROWS + M, J, distinct=R), HEAD_ROWS, M, K, seed=93)
    tile = lambda x: np.ascontiguousarray(np.tile(x, (B // R,) + (1,) * (x.ndim - 1)))
    got = call(ops, on_device({k: tile(v) for k, v in h.items()}))
    for x in got:
        assert tuple(x.shape)[0] == B
        assert torch.equal(x.view((B // R, R) + x.shape[1:]), x[:R].expand((B // R, R) + x.shape[1:]))   # every tile
    check_draw("large", [x[:R] for x in got], restated(h))


# ---- stream.Filter -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gp_case():
    """B = 4 series of 170 rows on their own grids under an SHO + real kernel and a mean: the filter of the 150-row head, the
    dense matrix of all rows (condition number asserted) and the celerite diagonal without noise, k(0)."""
    from celerite2_amd import gp as G, terms

    rng = np.random.default_rng(79)
    B, N, n0 = 4, 170, 150
    t = np.sort(rng.uniform(0.0, 34.0, (B, N)), axis=1)
    yerr = rng.uniform(0.2, 0.5, (B, N))
    y = rng.normal(size=(B, N)) + 0.3
    kernel = terms.SHOTerm(S0=1.2, w0=1.1, Q=2.5) + terms.RealTerm(a=0.8, c=0.3)
    td, ed, yd = dev(t, yerr, y)
    full = G.GaussianProcess(kernel, td, yerr=ed, mean=0.3)
    mats = [[host(x) for x in (full._c, full._a[b], full._U[b], full._V[b])] for b in range(B)]
    head = G.GaussianProcess(kernel, td[:, :n0].contiguous(), yerr=ed[:, :n0].contiguous(), mean=0.3)
    flt = head.filter(yd[:, :n0].contiguous())
    return dict(B=B, N=N, n0=n0, t=td, yerr=ed, y=yd, th=t, yh=y, eh=yerr, kernel=kernel, mats=mats, flt=flt,
                k0=1.2 * 1.1 * 2.5 + 0.8)


def _conditional(g, b, latent):
    """mu_c (without the mean) and Sigma_c of the tail of series b given its head, dense; the condition numbers asserted."""
    c, a, U, V = g["mats"][b]
    a = a.copy()
    if latent:
        a[g["n0"]:] = g["k0"]
    K = F.dense(g["th"][b], c, a, U, V)
    mu, Sig = D.dense_conditional(K, g["yh"][b] - 0.3, g["n0"])
    assert np.linalg.cond(K) <= 1e6 and np.linalg.cond(Sig) <= 1e6
    return mu, Sig


def test_sample_forecast_is_the_dense_conditional_draw(gp_case):
    """Filter.sample_forecast from gp.filter(y) of a 150-row head at the 20 times of the tail: mean + mu_c + cholesky(Sigma_c)
    @ eps for the dense conditional of the tail given the head, latent and with noise; (B, size, M), and (B, M) for size=None,
    equal to size=1; the filter is not changed; the same generator gives the same draws."""
    import torch

    g = gp_case
    B, n0, M, K = g["B"], g["n0"], g["N"] - g["n0"], 5
    flt = g["flt"]
    before = flt.state.clone()
    eps = np.random.default_rng(5).normal(size=(B, M, K))
    nrm, = dev(eps)
    for latent in (True, False):
        kw = {} if latent else dict(yerr=g["yerr"][:, n0:])
        out = flt.sample_forecast(g["t"][:, n0:], size=K, normals=nrm, **kw)
        assert tuple(out.shape) == (B, K, M)
        bare = flt.sample_forecast(g["t"][:, n0:], size=K, normals=nrm, include_mean=False, **kw)
        for b in range(B):
            mu, Sig = _conditional(g, b, latent)
            ref = (mu[:, None] + np.linalg.cholesky(Sig) @ eps[b]).T
            floor = max(np.abs(ref).max(), np.abs(g["yh"][b]).max())
            check((latent, b), out[b], ref + 0.3, floor)
            check((latent, b, "no mean"), bare[b], ref, floor)
        one = flt.sample_forecast(g["t"][:, n0:], normals=nrm[:, :, :1].contiguous(), **kw)
        assert tuple(one.shape) == (B, M)
        assert torch.equal(one, flt.sample_forecast(g["t"][:, n0:], size=1, normals=nrm[:, :, :1].contiguous(), **kw)[:, 0])
        assert torch.equal(one, out[:, 0])   # (a draw does not depend on how many are drawn with it)
    assert torch.equal(flt.state, before)
    gen = lambda: torch.Generator(device="cuda").manual_seed(11)
    a, b2 = (flt.sample_forecast(g["t"][:, n0:], size=3, generator=gen()) for _ in range(2))
    assert torch.equal(a, b2) and bool(torch.isfinite(a).all()) and not torch.equal(a[:, 0], a[:, 1])
    # a shared time grid (M,)
    ts = g["t"][:, n0 - 1].max() + torch.linspace(0.5, 4.0, 6, dtype=torch.float64, device="cuda")
    shared = flt.sample_forecast(ts, size=2, normals=nrm[:, :6, :2].contiguous())
    assert torch.equal(shared, flt.sample_forecast(ts[None, :].expand(B, 6).contiguous(), size=2, normals=nrm[:, :6, :2].contiguous()))


def test_sample_forecast_nan_rows_and_refusals(gp_case):
    """NaN in every row of a failed series and in the rows beyond `count`; unsorted and early times and normals of the wrong
    shape are refused."""
    import torch

    g = gp_case
    B, n0, M = g["B"], g["n0"], g["N"] - g["n0"]
    flt, t = g["flt"], g["t"][:, n0:]
    nrm = torch.randn((B, M, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    good = flt.sample_forecast(t, size=2, normals=nrm)
    cnt, = dev(np.array([M, 0, 3, 7], dtype=np.int32))
    out = flt.sample_forecast(t, size=2, normals=nrm, count=cnt)
    taken = (torch.arange(M, device="cuda")[None, :] < cnt[:, None])[:, None, :].expand(B, 2, M)
    assert bool(torch.isnan(out[~taken]).all()) and torch.equal(out[taken], good[taken])
    diag = torch.full((B, M), 0.04, dtype=torch.float64, device="cuda")
    diag[2, 4] = -50.0   # the predictive variance of that would-be observation comes out negative
    out = flt.sample_forecast(t, size=2, normals=nrm, diag=diag)
    assert bool(torch.isnan(out[2]).all()) and bool(torch.isfinite(out[[0, 1, 3]]).all())
    with pytest.raises(ValueError, match="sorted"):
        flt.sample_forecast(t.flip(1), size=2, normals=nrm)
    with pytest.raises(ValueError, match="before the last"):
        flt.sample_forecast(t - 10.0, size=2, normals=nrm)
    with pytest.raises(ValueError, match="normals"):
        flt.sample_forecast(t, size=3, normals=nrm)
    with pytest.raises(ValueError, match="normals"):
        flt.sample_forecast(t, normals=nrm)
    with pytest.raises(ValueError, match="only one"):
        flt.sample_forecast(t, yerr=diag, diag=diag)


def test_joint_log_density_is_the_dense_conditional_density(gp_case):
    """forecast_joint_log_density of the tail from the filter of the head: log N(y_tail | mean + mu_c, Sigma_c), dense; with
    M = 1 it is forecast_log_density; it is the sum of the one-row densities of successive appends on a clone; with a count
    it is that of the rows taken; NaN for a series with a failing row; the filter is bit for bit as before."""
    import torch

    g = gp_case
    B, n0, N = g["B"], g["n0"], g["N"]
    M = N - n0
    flt = g["flt"]
    before = flt.state.clone()
    t, y, e = g["t"][:, n0:], g["y"][:, n0:], g["yerr"][:, n0:]
    val = flt.forecast_joint_log_density(t, y, yerr=e)
    assert tuple(val.shape) == (B,) and not val.requires_grad

    def dense_density(b, m):
        c, a, U, V = g["mats"][b]
        K = F.dense(g["th"][b, :n0 + m], c, a[:n0 + m], U[:n0 + m], V[:n0 + m])
        mu, Sig = D.dense_conditional(K, g["yh"][b, :n0 + m] - 0.3, n0)
        assert np.linalg.cond(Sig) <= 1e6
        r = g["yh"][b, n0:n0 + m] - 0.3 - mu
        return -0.5 * (r @ np.linalg.solve(Sig, r) + np.linalg.slogdet(Sig)[1] + m * np.log(2 * np.pi))

    check("dense", val, np.array([dense_density(b, M) for b in range(B)]))
    one = flt.forecast_joint_log_density(t[:, :1], y[:, :1], yerr=e[:, :1])
    check("M = 1", one, host(flt.forecast_log_density(t[:, :1], y[:, :1], yerr=e[:, :1])))
    assert not torch.equal(val, flt.forecast_log_density(t, y, yerr=e))   # (the marginal densities are another number)
    walk, total = flt.clone(), torch.zeros(B, dtype=torch.float64, device="cuda")
    for m in range(M):
        upd = walk.append(t[:, m:m + 1], y[:, m:m + 1], yerr=e[:, m:m + 1])
        total += -0.5 * (upd.innovation ** 2 / upd.variance + torch.log(upd.variance) + np.log(2 * np.pi))[:, 0]
    check("successive appends", val, host(total))
    counts = np.array([M, 0, 3, 7], dtype=np.int32)
    cnt, = dev(counts)
    part = flt.forecast_joint_log_density(t, y, yerr=e, count=cnt)
    assert float(part[1]) == 0.0 and torch.equal(part[0], val[0])
    check("count", part[2:], np.array([dense_density(b, int(counts[b])) for b in (2, 3)]))
    diag = e ** 2
    diag[2, 4] = -50.0
    failed = flt.forecast_joint_log_density(t, y, diag=diag)
    assert bool(torch.isnan(failed[2])) and torch.equal(failed[[0, 1, 3]], val[[0, 1, 3]])
    assert torch.equal(flt.state, before)
    with pytest.raises(ValueError, match="required"):
        flt.forecast_joint_log_density(t, y)
    with pytest.raises(ValueError, match="sorted"):
        flt.forecast_joint_log_density(t.flip(1), y, yerr=e)


def _dense_kernel(p, tau):
    """k(tau) of _kernel_case's SHO (underdamped) + real kernel, in torch."""
    import torch

    f = torch.sqrt(4.0 * p["Q"] ** 2 - 1.0)
    a, c = p["S0"] * p["w0"] * p["Q"], 0.5 * p["w0"] / p["Q"]
    return (a * torch.exp(-c * tau) * (torch.cos(c * f * tau) + torch.sin(c * f * tau) / f)
            + p["a"] * torch.exp(-p["c"] * tau))


def test_joint_log_density_trains_like_the_dense_conditional_density():
    """On a filter with tensor hyper-parameters, a jitter and a mean, fed the head in six appends: the value and the gradient
    in all seven parameters of forecast_joint_log_density of the tail are those of the dense conditional density
    log N(y_tail | mean + mu_c, Sigma_c), built and differentiated by torch in float64; the filter's state is not rebound."""
    import torch
    from celerite2_amd.stream import Filter

    B, N, t, yerr, y, params, kernel = _kernel_case()
    p = params()
    flt = _fed(Filter.empty(kernel(p), B, mean=p["mean"], jitter=p["jitter"]), t, y, yerr, N0)
    state = flt.state
    val = flt.forecast_joint_log_density(t[:, N0:], y[:, N0:], yerr=yerr[:, N0:])
    assert tuple(val.shape) == (B,) and val.requires_grad and flt.state is state

    po = params()
    th, eh, yh = t.cpu(), yerr.cpu(), y.cpu()
    pc = {k: v.detach().cpu().requires_grad_() for k, v in po.items()}
    vals = []
    for b in range(B):
        K = _dense_kernel(pc, (th[b, :, None] - th[b, None, :]).abs()) + torch.diag(eh[b] ** 2 + pc["jitter"] ** 2)
        assert float(torch.linalg.cond(K.detach())) <= 1e6
        r = yh[b] - pc["mean"]
        sol = torch.linalg.solve(K[:N0, :N0], torch.cat([r[:N0, None], K[:N0, N0:]], dim=1))
        mu, Sig = K[N0:, :N0] @ sol[:, 0], K[N0:, N0:] - K[N0:, :N0] @ sol[:, 1:]
        assert float(torch.linalg.cond(Sig.detach())) <= 1e6
        L = torch.linalg.cholesky(Sig)
        w = torch.linalg.solve_triangular(L, (r[N0:] - mu)[:, None], upper=False)[:, 0]
        vals.append(-0.5 * (w @ w) - torch.log(torch.diagonal(L)).sum() - 0.5 * (N - N0) * np.log(2 * np.pi))
    _compare("joint", val, p, torch.stack(vals), pc)
