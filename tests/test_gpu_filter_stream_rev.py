# -*- coding: utf-8 -*-
"""GPU checks of the reverse of a streaming forecast and of a streaming absorb: ops.filter_forecast_rev and
ops.filter_absorb_rev (include/celerite2_amd_filter_stream_rev.h, csrc/c2_filter_stream_rev.hip) at every group size,
autograd.filter_forecast[_kernel] / filter_absorb[_kernel], Filter.forecast_kernel / forecast_log_density and
gp.filter_kernel on top of them.

References: the numpy restatement (tests/filter_stream_rev_ref.py, pinned to torch autograd and to exact dense derivatives by
tests/test_filter_stream_rev.py), and the device's own whole-series routes, autograd.predictive_log_density_kernel and
autograd.log_likelihood_kernel.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o|
(inverse_diag_ref.err), with a floor of 1 for an expected array that is all zero (the cotangents are unit normal draws); the
draws are those of tests/test_gpu_filter.py (condition number <= 1e6, asserted there per draw)."""
import numpy as np
import pytest

import filter_ref as F
import filter_rev_ref as R
import filter_stream_rev_ref as Q
from test_gpu_filter import CUTS, HEAD_ROWS, WIDTHS, _odd, batch, dev, host, states_of
from test_gpu_filter_rev import _kernel_case, _shared_case, check

pytestmark = pytest.mark.gpu
FNAMES = ("bstate", "bt", "bc", "ba", "bU")
ANAMES = ("bstate_in", "bt", "bc", "bW", "bd", "bz")
SENT = -7.0


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


def cotangents(seed, B, M, J):
    """bstate (B, SW), bmu, bvar (B, M): unit normal draws."""
    rng = np.random.default_rng(seed)
    return [rng.normal(size=s) for s in ((B, F.state_words(J)), (B, M), (B, M))]


def case(bt, n0, M):
    """Rows n0 .. n0 + M of a batch behind the restatement's state in front of them, on the host."""
    h = {k: np.ascontiguousarray(bt[k][:, n0:n0 + M]) for k in "taUWdz"}
    h.update(state=states_of(bt, n0), c=bt["c"])
    return h


def _row(x, b):
    return x if x.ndim == 1 else x[b]


def restated_forecast(h, bmu, bvar, counts=None):
    out = [Q.forecast_rev(h["state"][b], _row(h["c"], b), _row(h["t"], b), h["U"][b], bmu[b], bvar[b],
                          count=None if counts is None else int(counts[b])) for b in range(h["state"].shape[0])]
    return [np.stack([o[i] for o in out]) for i in range(5)]


def restated_absorb(h, bs, counts=None):
    out = [Q.absorb_rev(h["state"][b], _row(h["c"], b), _row(h["t"], b), h["W"][b], h["d"][b], h["z"][b], bs[b],
                        count=None if counts is None else int(counts[b])) for b in range(h["state"].shape[0])]
    return [np.stack([o[i] for o in out]) for i in range(7)]


def check_outputs(key, names, got, want, J, symmetric=None):
    for name, x, xo in zip(names, got, want):
        if name.startswith("bstate"):
            x = host(x)
            check((key, name, "head"), x[:, :4], xo[:, :4])
            check((key, name, "bF"), x[:, 4:4 + J], xo[:, 4:4 + J])
            check((key, name, "bS"), x[:, 4 + J:], xo[:, 4 + J:])
            S = x[:, 4 + J:].reshape(-1, J, J)
            S = S if symmetric is None else S[symmetric]   # (a series passed through keeps the block it was given)
            assert np.array_equal(S, S.transpose(0, 2, 1)), key   # the symmetric representative, to the bit
        else:
            check((key, name), x, xo)


def call_forecast(ops, d, bmu, bvar, **kw):
    return ops.filter_forecast_rev(d["state"], d["t"], d["c"], d["U"], bmu, bvar, **kw)


def call_absorb(ops, d, bs, **kw):
    return ops.filter_absorb_rev(d["state"], d["t"], d["c"], d["W"], d["d"], d["z"], bs, **kw)


def on_device(h):
    return dict(zip(h, dev(*h.values())))


# ---- group and wave boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", WIDTHS)
def test_group_and_wave_boundaries(ops, J):
    """Every group size (J and the next power of two), partial wavefronts (B = 1, 3, 65, 130) and M on both sides of 16 and
    32, from a state with HEAD_ROWS rows (B = 3 also from the empty one): every output of both reverses, and the ws rows of
    the absorb reverse against the replayed states."""
    import torch

    for B in (1, 3, 65, 130):
        for M in (1, 2, 17, 33):
            for n0 in ((HEAD_ROWS, 0) if B == 3 else (HEAD_ROWS,)):
                key = (J, B, M, n0)
                h = case(batch(J, B, HEAD_ROWS + M, J), n0, M)
                d = on_device(h)
                bs, bmu, bvar = cotangents(1000 * J + 10 * B + M, B, M, J)
                got = call_forecast(ops, d, *dev(bmu, bvar))
                check_outputs((key, "forecast"), FNAMES, got, restated_forecast(h, bmu, bvar), J)
                if n0 == 0:   # ba = bvar, zeros everywhere else
                    assert torch.equal(got[3], dev(bvar)[0]) and not any(bool(x.any()) for i, x in enumerate(got) if i != 3)
                ws = torch.full((B, M, R.workspace_words(J)), SENT, dtype=torch.float64, device="cuda")
                got = call_absorb(ops, d, dev(bs)[0], ws=ws)
                want = restated_absorb(h, bs)
                check_outputs((key, "absorb"), ANAMES, got, want, J)
                check((key, "ws F"), ws[..., :J], want[6][..., :J])
                check((key, "ws S"), ws[..., J:], want[6][..., J:])


# ---- ragged counts, determinism ---------------------------------------------------------------------------------------------
def test_ragged_counts_in_sentinel_filled_outputs(ops):
    """count includes 0 and M: zeros are written beyond count, a sentinel survives nowhere, a count-0 series gets a zero state
    cotangent from the forecast reverse and the identity from the absorb reverse, and the rows taken are the restatement's."""
    import torch

    J, M, n0 = 5, 6, HEAD_ROWS
    counts = np.array([0, 6, 2, 0, 1, 6, 3, 5, 0, 4], dtype=np.int32)
    B = len(counts)
    h = case(batch(91, B, n0 + M, J), n0, M)
    d = on_device(h)
    cnt, = dev(counts)
    bs, bmu, bvar = cotangents(17, B, M, J)
    dbs, dbmu, dbvar = dev(bs, bmu, bvar)
    full = lambda *s: torch.full(s, SENT, dtype=torch.float64, device="cuda")
    taken = torch.from_numpy(np.arange(M)[None, :] < counts[:, None]).cuda()
    none = cnt == 0

    out = [full(B, F.state_words(J)), full(B, M), full(B, J), full(B, M), full(B, M, J)]
    got = call_forecast(ops, d, dbmu, dbvar, count=cnt, out=out)
    assert all(x is o for x, o in zip(got, out))
    check_outputs("ragged forecast", FNAMES, got, restated_forecast(h, bmu, bvar, counts), J)
    for name, x in zip(FNAMES, got):
        assert not bool((x == SENT).any()), name
        if name in ("bt", "ba", "bU"):
            assert not bool(x[~taken].any()), name
    assert not bool(got[0][none].any()) and not bool(got[2][none].any())

    out = [full(B, F.state_words(J)), full(B, M), full(B, J), full(B, M, J), full(B, M), full(B, M)]
    got = call_absorb(ops, d, dbs, count=cnt, out=out)
    assert all(x is o for x, o in zip(got, out))
    check_outputs("ragged absorb", ANAMES, got, restated_absorb(h, bs, counts), J, counts > 0)
    for name, x in zip(ANAMES, got):
        assert not bool((x == SENT).any()), name
        if name in ("bt", "bW", "bd", "bz"):
            assert not bool(x[~taken].any()), name
    assert torch.equal(got[0][none], dbs[none]) and not bool(got[2][none].any())


def test_two_calls_give_identical_bits(ops):
    import torch

    for J, B in ((8, 130), (17, 65)):
        d = on_device(case(batch(99, B, HEAD_ROWS + 17, J), HEAD_ROWS, 17))
        bs, bmu, bvar = dev(*cotangents(29, B, 17, J))
        for x, x2 in zip(call_forecast(ops, d, bmu, bvar), call_forecast(ops, d, bmu, bvar)):
            assert torch.equal(x, x2)
        for x, x2 in zip(call_absorb(ops, d, bs), call_absorb(ops, d, bs)):
            assert torch.equal(x, x2)


# ---- shared t and c, offsets ------------------------------------------------------------------------------------------------
def test_shared_t_and_c_and_odd_offsets(ops):
    """t and c shared by the batch (stride 0) give the bits of the same values repeated per series, bt (B, M) and bc (B, J)
    per series all the same; every array starting at an odd element gives the bits of the aligned call; the autograd layer
    returns the batch sum for the shared arguments."""
    import torch
    from celerite2_amd import autograd as ag

    J, M, B, st0, t1, c1, tB, cB, a, U, V, y = _shared_case(ops)
    cnt, = dev(np.array([9, 0, 4, 9, 1, 7, 2], dtype=np.int32))
    _, d, W, z, flag = ops.filter_append(st0, tB, cB, a, U, V, y)
    assert int(flag.abs().sum()) == 0
    bs, bmu, bvar = dev(*cotangents(31, B, M, J))
    o = _odd
    sent = lambda x: torch.full_like(x, SENT)

    base = ops.filter_forecast_rev(st0, tB, cB, U, bmu, bvar, count=cnt)
    shared = ops.filter_forecast_rev(st0, t1, c1, U, bmu, bvar, count=cnt)
    assert tuple(shared[1].shape) == (B, M) and tuple(shared[2].shape) == (B, J)
    odd = ops.filter_forecast_rev(o(st0), o(t1), o(c1), o(U), o(bmu), o(bvar), count=o(cnt), out=[o(sent(x)) for x in base])
    for name, x, xs, xb in zip(FNAMES, odd, shared, base):
        assert torch.equal(xs, xb) and torch.equal(x, xb), name

    base = ops.filter_absorb_rev(st0, tB, cB, W, d, z, bs, count=cnt)
    shared = ops.filter_absorb_rev(st0, t1, c1, W, d, z, bs, count=cnt)
    assert tuple(shared[1].shape) == (B, M) and tuple(shared[2].shape) == (B, J)
    odd = ops.filter_absorb_rev(o(st0), o(t1), o(c1), o(W), o(d), o(z), o(bs), count=o(cnt),
                                ws=o(torch.empty((B, M, J + J * J), dtype=torch.float64, device="cuda")),
                                out=[o(sent(x)) for x in base])
    for name, x, xs, xb in zip(ANAMES, odd, shared, base):
        assert torch.equal(xs, xb) and torch.equal(x, xb), name

    # the autograd layer: the batch sum for shared t and c, the state cotangent of the forecast
    ts, cs_, ss = t1.clone().requires_grad_(), c1.clone().requires_grad_(), st0.clone().requires_grad_()
    mu, var = ag.filter_forecast(ss, ts, cs_, a, U)
    gs, gt, gc = torch.autograd.grad((mu * bmu).sum() + (var * bvar).sum(), (ss, ts, cs_))
    full = ops.filter_forecast_rev(st0, t1, c1, U, bmu, bvar)
    assert tuple(gt.shape) == (M,) and tuple(gc.shape) == (J,)
    assert torch.equal(gs, full[0]) and torch.equal(gt, full[1].sum(0)) and torch.equal(gc, full[2].sum(0))
    mu_o, var_o = ops.filter_forecast(st0, t1, c1, a, U)
    assert torch.equal(mu, mu_o) and torch.equal(var, var_o)
    ts, cs_ = t1.clone().requires_grad_(), c1.clone().requires_grad_()
    out = ag.filter_absorb(st0, ts, cs_, W, d, z)
    gt, gc = torch.autograd.grad((out * bs).sum(), (ts, cs_))
    full = ops.filter_absorb_rev(st0, t1, c1, W, d, z, bs)
    assert torch.equal(out, ops.filter_absorb(st0, t1, c1, W, d, z))
    assert torch.equal(gt, full[1].sum(0)) and torch.equal(gc, full[2].sum(0))


def test_empty_state_far_below_t_last(ops):
    """n == 0 under a stale t_last of +1e6 and times near -1e4: no NaN anywhere, everything equal to the run under
    t_last = 0, the forecast reverse gives ba = bvar and zeros, and nothing flows into the empty state from the absorb."""
    import torch

    for J in (2, 8):
        bt = batch(95, 3, 4, J)
        t, c, U, W, d, z = dev(bt["t"] - 1e4, bt["c"], bt["U"], bt["W"], bt["d"], bt["z"])
        bs, bmu, bvar = dev(*cotangents(37, 3, 4, J))
        res = []
        for tl in (1e6, 0.0):
            st = ops.filter_init(3, J, "cuda")
            st[:, 0] = tl
            res.append(ops.filter_forecast_rev(st, t, c, U, bmu, bvar) + ops.filter_absorb_rev(st, t, c, W, d, z, bs))
        for name, x, xo in zip(FNAMES + ANAMES, *res):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, xo), name
        fc, ab = res[0][:5], res[0][5:]
        assert torch.equal(fc[3], bvar) and not any(bool(x.any()) for i, x in enumerate(fc) if i != 3)
        assert not bool(ab[0][:, 0].any()) and not bool(ab[0][:, 4:].any())


def test_nan_state_is_local(ops):
    """A series with a NaN state between good ones in one wavefront: the good ones' bits are those of the run without it."""
    import torch

    J, M, n0, B = 3, 6, HEAD_ROWS, 16   # G = 4: all 16 series in one wavefront
    d = on_device(case(batch(97, B, n0 + M, J), n0, M))
    bs, bmu, bvar = dev(*cotangents(23, B, M, J))
    good = call_forecast(ops, d, bmu, bvar) + call_absorb(ops, d, bs)
    bad = dict(d, state=d["state"].clone())
    bad["state"][5] = float("nan")
    bad["state"][9, 4:] = float("nan")
    got = call_forecast(ops, bad, bmu, bvar) + call_absorb(ops, bad, bs)
    ok = torch.ones(B, dtype=torch.bool, device="cuda")
    ok[[5, 9]] = False
    for name, x, xg in zip(FNAMES + ANAMES, got, good):
        assert torch.equal(x[ok], xg[ok]), name
    assert bool(torch.isnan(got[0][5]).any()) and bool(torch.isnan(got[5][9]).any())


# ---- a batch beyond 65535 series ---------------------------------------------------------------------------------------------
def test_large_batch(ops):
    """B = 70000 at J = 2, M = 3: seven distinct series tiled, every series of both reverses against the restatement (the two
    entry points are not in the census of tests/large_batch_cases.py)."""
    import torch

    J, M, n0, K, B = 2, 3, HEAD_ROWS, 7, 70000
    h = case(batch(93, K, n0 + M, J, distinct=K), n0, M)
    bs, bmu, bvar = cotangents(41, K, M, J)
    tile = lambda x: np.ascontiguousarray(np.tile(x, (B // K,) + (1,) * (x.ndim - 1)))
    d = on_device({k: tile(v) for k, v in h.items()})
    dbs, dbmu, dbvar = dev(tile(bs), tile(bmu), tile(bvar))
    for names, got, want in ((FNAMES, call_forecast(ops, d, dbmu, dbvar), restated_forecast(h, bmu, bvar)),
                             (ANAMES, call_absorb(ops, d, dbs), restated_absorb(h, bs))):
        for name, x, xo in zip(names, got, want):
            assert torch.equal(x.view((B // K, K) + x.shape[1:]), x[:K].expand((B // K, K) + x.shape[1:])), name   # every tile
            check(("large", name), x[:K], xo)


# ---- chains -----------------------------------------------------------------------------------------------------------------
N0 = 120   # rows of the head of the 150-row series of _kernel_case


def _fed(flt, t, y, yerr, hi):
    for lo, h in zip(CUTS, [c for c in CUTS[1:] if c < hi] + [hi]):
        upd = flt.append(t[:, lo:h], y[:, lo:h], yerr=yerr[:, lo:h])
        assert int(upd.flag.abs().sum()) == 0
    return flt


def _compare(key, val, p, val_o, po):
    import torch

    g = torch.autograd.grad(val.sum(), list(p.values()))
    g_o = torch.autograd.grad(val_o.sum(), list(po.values()))
    check((key, "value"), val, host(val_o))
    for k, x, xo in zip(p, g, g_o):
        check((key, "grad", k), x.reshape(1), host(xo).reshape(1))


def test_forecast_log_density_trains_like_the_held_out_density():
    """A Filter under an SHO + real kernel of tensor parameters, a jitter and a mean, fed the head in six appends: the
    forecast_log_density of the tail and its gradient in all seven parameters are those of
    autograd.predictive_log_density_kernel(head -> tail).  Filter.forecast stays detached."""
    from celerite2_amd import autograd as ag
    from celerite2_amd.stream import Filter

    B, N, t, yerr, y, params, kernel = _kernel_case()
    p = params()
    flt = _fed(Filter.empty(kernel(p), B, mean=p["mean"], jitter=p["jitter"]), t, y, yerr, N0)
    val = flt.forecast_log_density(t[:, N0:], y[:, N0:], yerr=yerr[:, N0:])
    assert tuple(val.shape) == (B,) and val.requires_grad
    po = params()
    val_o = ag.predictive_log_density_kernel(kernel(po), t[:, :N0], y[:, :N0], t[:, N0:], y[:, N0:], yerr=yerr[:, :N0],
                                             jitter=po["jitter"], mean=po["mean"], yerr_new=yerr[:, N0:])
    _compare("tail", val, p, val_o, po)
    mu, var = flt.forecast(t[:, N0:])
    mu_g, var_g = flt.forecast_kernel(t[:, N0:])
    assert not mu.requires_grad and not var.requires_grad and mu_g.requires_grad and var_g.requires_grad
    check("forecast mu", mu_g, host(mu))
    check("forecast var", var_g, host(var))
    with pytest.raises(ValueError, match="before the last absorbed time"):
        flt.forecast_log_density(t[:, N0 - 2:N0 + 1], y[:, N0 - 2:N0 + 1], yerr=yerr[:, N0 - 2:N0 + 1])
    with pytest.raises(ValueError, match="required"):
        flt.forecast_log_density(t[:, N0:], y[:, N0:])


def test_forecast_log_density_of_the_next_row_is_its_append():
    """forecast_log_density of the next row alone is that row's -(1/2) (z^2 / d + log d + log 2 pi) from `append`, value and
    gradient; with a count, the rows not taken drop out; on a plain kernel the same value without a graph."""
    import torch
    from celerite2_amd import terms
    from celerite2_amd.stream import Filter

    B, N, t, yerr, y, params, kernel = _kernel_case()
    nxt = slice(N0, N0 + 1)
    p = params()
    flt = _fed(Filter.empty(kernel(p), B, mean=p["mean"], jitter=p["jitter"]), t, y, yerr, N0)
    val = flt.forecast_log_density(t[:, nxt], y[:, nxt], yerr=yerr[:, nxt])
    po = params()
    flo = _fed(Filter.empty(kernel(po), B, mean=po["mean"], jitter=po["jitter"]), t, y, yerr, N0)
    upd = flo.append(t[:, nxt], y[:, nxt], yerr=yerr[:, nxt])
    val_o = -0.5 * (upd.innovation ** 2 / upd.variance + torch.log(upd.variance) + np.log(2 * np.pi))[:, 0]
    cnt, = dev(np.array([3, 0, 1, 2], dtype=np.int32))
    three = slice(N0, N0 + 3)
    part = flt.forecast_log_density(t[:, three], y[:, three], yerr=yerr[:, three], count=cnt)
    assert float(part[1].detach()) == 0.0
    check("count 1", part[2:3], host(val[2:3]))
    whole = flt.forecast_log_density(t[:, three], y[:, three], yerr=yerr[:, three])
    assert torch.equal(part[0], whole[0])
    assert all(bool(torch.isfinite(x).all()) for x in torch.autograd.grad(part.sum(), list(p.values()), retain_graph=True))
    _compare("next row", val, p, val_o, po)

    plain = Filter.empty(terms.SHOTerm(S0=1.2, w0=1.1, Q=2.5) + terms.RealTerm(a=0.8, c=0.3), B, mean=0.3)
    e2 = torch.sqrt(yerr ** 2 + 0.15 ** 2)   # (the jitter of _kernel_case, in quadrature)
    _fed(plain, t, y, e2, N0)
    v = plain.forecast_log_density(t[:, three], y[:, three], yerr=e2[:, three])
    assert not v.requires_grad
    check("plain", v, host(whole))


def test_gp_filter_kernel_is_the_whole_series():
    """gp.filter_kernel(y): its log_likelihood and gradient in all seven parameters are those of
    autograd.log_likelihood_kernel; built on the head with the tail appended behind it, those of the whole series; gp.filter
    still refuses the kernel."""
    from celerite2_amd import autograd as ag, gp as G

    B, N, t, yerr, y, params, kernel = _kernel_case()
    p, po = params(), params()
    gp = G.GaussianProcess(kernel(p), t, diag=yerr ** 2, mean=p["mean"])
    flt = gp.filter_kernel(y, jitter=p["jitter"])
    assert flt.differentiable and flt.state.requires_grad and bool((flt.n == N).all())
    ll_o = ag.log_likelihood_kernel(kernel(po), t, y, yerr=yerr, jitter=po["jitter"], mean=po["mean"])
    _compare("whole", flt.log_likelihood, p, ll_o, po)
    with pytest.raises(ValueError, match="tensor hyper-parameters"):
        gp.filter(y)

    p, po = params(), params()
    head = G.GaussianProcess(kernel(p), t[:, :N0].contiguous(), diag=yerr[:, :N0].contiguous() ** 2, mean=p["mean"])
    flt = head.filter_kernel(y[:, :N0].contiguous(), jitter=p["jitter"])
    upd = flt.append(t[:, N0:], y[:, N0:], yerr=yerr[:, N0:])
    assert int(upd.flag.abs().sum()) == 0
    ll_o = ag.log_likelihood_kernel(kernel(po), t, y, yerr=yerr, jitter=po["jitter"], mean=po["mean"])
    _compare("head + tail", flt.log_likelihood, p, ll_o, po)
