# -*- coding: utf-8 -*-
"""GPU checks of the reverse of a streaming append: ops.filter_append_rev (include/celerite2_amd_filter_rev.h,
csrc/c2_filter_rev.hip) at every group size, autograd.filter_append[_kernel] and a stream.Filter with tensor hyper-parameters
on top of it.

References: the numpy restatement (tests/filter_rev_ref.py, pinned to torch autograd and to exact dense derivatives by
tests/test_filter_rev.py), and the device's own whole-series gradients, autograd.log_likelihood and
autograd.log_likelihood_kernel.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o|
(inverse_diag_ref.err); the draws are those of tests/test_gpu_filter.py (condition number <= 1e6, asserted there per draw)."""
import numpy as np
import pytest

import filter_ref as F
import filter_rev_ref as R
from test_gpu_filter import CUTS, HEAD_ROWS, WIDTHS, _odd, batch, dev, host, rows, states_of

pytestmark = pytest.mark.gpu
NAMES = ("bstate_in", "bt", "bc", "ba", "bU", "bV", "by")


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


def check(key, x, xo, floor=None):
    """The standing criterion; an expected array that is all zero (what flows into an empty state) has no scale of its own
    and takes that of the incoming cotangents, unit normal draws: 1."""
    x, xo = (host(x) if hasattr(x, "cpu") else x), np.asarray(xo)
    if floor is None and not xo.any():
        floor = 1.0
    e = F.err(x, xo, floor)
    assert e <= 1.0, (key, e)


def cotangents(seed, B, M, J):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=s) for s in ((B, F.state_words(J)), (B, M), (B, M, J), (B, M))]


def forward(ops, bt, n0, M, count=None):
    """The append of rows n0 .. n0 + M on the device from the restatement's state behind row n0 - 1: what the reverse reads."""
    st0, c = dev(states_of(bt, n0), bt["c"])
    t, a, U, V, y = rows(bt, n0, n0 + M)
    _, d, W, z, flag = ops.filter_append(st0, t, c, a, U, V, y, count=count)
    return dict(state=st0, t=t, c=c, U=U, W=W, d=d, z=z, flag=flag, a=a, V=V, y=y)


def restated(fw, cots, counts=None):
    """R.append_rev per series on the device's own W, d, z -> the seven outputs and ws, stacked over the batch."""
    h = {k: host(fw[k]) for k in ("state", "t", "c", "U", "W", "d", "z", "flag")}
    B = h["state"].shape[0]
    out = []
    for b in range(B):
        t = h["t"] if h["t"].ndim == 1 else h["t"][b]
        c = h["c"] if h["c"].ndim == 1 else h["c"][b]
        out.append(R.append_rev(h["state"][b], c, t, h["U"][b], h["W"][b], h["d"][b], h["z"][b], int(h["flag"][b]),
                                *(x[b] for x in cots), count=None if counts is None else int(counts[b])))
    return [np.stack([o[i] for o in out]) for i in range(8)]


def call(ops, fw, cots, **kw):
    return ops.filter_append_rev(fw["state"], fw["t"], fw["c"], fw["U"], fw["W"], fw["d"], fw["z"], fw["flag"], *cots, **kw)


def check_outputs(key, got, want, J, reversed_=None):
    for name, x, xo in zip(NAMES, got, want):
        if name == "bstate_in":
            x = host(x)
            check((key, "head"), x[:, :4], xo[:, :4])
            check((key, "bF"), x[:, 4:4 + J], xo[:, 4:4 + J])
            check((key, "bS"), x[:, 4 + J:], xo[:, 4 + J:])
            S = x[:, 4 + J:].reshape(-1, J, J)
            S = S if reversed_ is None else S[reversed_]   # (a series passed through keeps the block it was given)
            assert np.array_equal(S, S.transpose(0, 2, 1)), key   # the symmetric representative, to the bit
        else:
            check((key, name), x, xo)


# ---- group and wave boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", WIDTHS)
def test_group_and_wave_boundaries(ops, J):
    """Every group size (J and the next power of two), partial wavefronts (B = 1, 3, 65, 130) and M on both sides of 16 and
    32, from a state with HEAD_ROWS rows (B = 3 also from the empty one): all seven outputs, and the ws rows against the
    replayed states."""
    import torch

    for B in (1, 3, 65, 130):
        for M in (1, 2, 17, 33):
            for n0 in ((HEAD_ROWS, 0) if B == 3 else (HEAD_ROWS,)):
                key = (J, B, M, n0)
                bt = batch(J, B, HEAD_ROWS + M, J)
                fw = forward(ops, bt, n0, M)
                assert int(fw["flag"].abs().sum()) == 0, key
                cots = cotangents(1000 * J + 10 * B + M, B, M, J)
                ws = torch.full((B, M, R.workspace_words(J)), -7.0, dtype=torch.float64, device="cuda")
                got = call(ops, fw, dev(*cots), ws=ws)
                want = restated(fw, cots)
                check_outputs(key, got, want, J)
                check((key, "ws F"), ws[..., :J], want[7][..., :J])
                check((key, "ws S"), ws[..., J:], want[7][..., J:])


# ---- the chain of calls against the whole-series gradient -----------------------------------------------------------------
def test_chain_through_autograd_is_the_whole_series_gradient():
    """150 rows appended as 1, 1, 5, 16, 17 and the rest through autograd.filter_append, the loss the log-likelihood of the last
    state: the gradients in t, c, a, U, V, y are those of autograd.log_likelihood of the whole series."""
    import torch
    from celerite2_amd import autograd as ag, ops

    B, N, J = 5, 150, 8
    bt = batch(48, B, N, J, gap=True)
    ins = [x.requires_grad_() for x in dev(*(bt[k] for k in "tcaUVy"))]
    t, c, a, U, V, y = ins
    st = ops.filter_init(B, J, "cuda")
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        st, d, W, z, flag = ag.filter_append(st, t[:, lo:hi], c, a[:, lo:hi], U[:, lo:hi], V[:, lo:hi], y[:, lo:hi])
        assert int(flag.abs().sum()) == 0 and not flag.requires_grad
    ll = -0.5 * (st[:, 3] + st[:, 2] + st[:, 1] * np.log(2 * np.pi))
    g = torch.autograd.grad(ll.sum(), ins)
    ins_o = [x.detach().clone().requires_grad_() for x in ins]
    ll_o = ag.log_likelihood(*ins_o)
    g_o = torch.autograd.grad(ll_o.sum(), ins_o)
    check("ll", ll, host(ll_o))
    for k, x, xo in zip("tcaUVy", g, g_o):
        check(("grad", k), x, host(xo))


def _kernel_case():
    import torch
    from celerite2_amd import terms

    rng = np.random.default_rng(78)
    B, N = 4, 150
    t = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    yerr = rng.uniform(0.2, 0.5, (B, N))
    y = rng.normal(size=(B, N)) + 0.3
    td, ed, yd = dev(t, yerr, y)

    def params():
        vals = dict(S0=1.2, w0=1.1, Q=2.5, a=0.8, c=0.3, jitter=0.15, mean=0.3)
        return {k: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for k, v in vals.items()}

    def kernel(p):
        return terms.SHOTerm(S0=p["S0"], w0=p["w0"], Q=p["Q"], regime="under") + terms.RealTerm(a=p["a"], c=p["c"])

    return B, N, td, ed, yd, params, kernel


def test_filter_with_tensor_kernel_trains_like_the_whole_series():
    """The chain through stream.Filter under an SHO + real kernel of tensor parameters, a jitter and a mean: log-likelihood and
    its gradient in every parameter are those of autograd.log_likelihood_kernel of the whole series; after detach() behind
    chunk 3 the gradient is that of the later chunks alone, from a filter rebuilt at that state."""
    import torch
    from celerite2_amd import autograd as ag
    from celerite2_amd.stream import Filter

    B, N, t, yerr, y, params, kernel = _kernel_case()
    p = params()
    flt = Filter.empty(kernel(p), B, mean=p["mean"], jitter=p["jitter"])
    assert flt.differentiable
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        upd = flt.append(t[:, lo:hi], y[:, lo:hi], yerr=yerr[:, lo:hi])
        assert int(upd.flag.abs().sum()) == 0 and upd.innovation.requires_grad and upd.variance.requires_grad
    ll = flt.log_likelihood
    g = torch.autograd.grad(ll.sum(), list(p.values()))
    po = params()
    ll_o = ag.log_likelihood_kernel(kernel(po), t, y, yerr=yerr, jitter=po["jitter"], mean=po["mean"])
    g_o = torch.autograd.grad(ll_o.sum(), list(po.values()))
    check("ll", ll, host(ll_o))
    for k, x, xo in zip(p, g, g_o):
        check(("grad", k), x.reshape(1), host(xo).reshape(1))
    mu, var = flt.forecast(t[:, -1:] + 1.0)
    assert not mu.requires_grad and not var.requires_grad and bool(torch.isfinite(mu).all())

    # truncated back-propagation: detach behind chunk 3
    p = params()
    flt = Filter.empty(kernel(p), B, mean=p["mean"], jitter=p["jitter"])
    for lo, hi in zip(CUTS[:3], CUTS[1:4]):
        flt.append(t[:, lo:hi], y[:, lo:hi], yerr=yerr[:, lo:hi])
    assert flt.state.requires_grad
    assert flt.detach() is flt and not flt.state.requires_grad
    mid = flt.state.clone()
    for lo, hi in zip(CUTS[3:-1], CUTS[4:]):
        flt.append(t[:, lo:hi], y[:, lo:hi], yerr=yerr[:, lo:hi])
    g_cut = torch.autograd.grad(flt.log_likelihood.sum(), list(p.values()))
    po = params()
    rebuilt = Filter(kernel(po), mid, mean=po["mean"], jitter=po["jitter"])
    for lo, hi in zip(CUTS[3:-1], CUTS[4:]):
        rebuilt.append(t[:, lo:hi], y[:, lo:hi], yerr=yerr[:, lo:hi])
    g_late = torch.autograd.grad(rebuilt.log_likelihood.sum(), list(po.values()))
    for k, x, xo, xf in zip(p, g_cut, g_late, g):
        check(("cut", k), x.reshape(1), host(xo).reshape(1))
        assert abs(float(x) - float(xf)) > 1e-6 * abs(float(xf)), k   # (and not the gradient of the whole chain)


def test_convolution_is_refused():
    """A TermConvolution around a kernel of tensor parameters: refused by the Filter and by filter_append_kernel."""
    import torch
    from celerite2_amd import autograd as ag, ops, terms
    from celerite2_amd.stream import Filter

    B, N, t, yerr, y, params, kernel = _kernel_case()
    p = params()
    conv = terms.TermConvolution(kernel(p), 0.02)   # (a convolution is always the outer term)
    state = ops.filter_init(B, 3, "cuda")
    with pytest.raises(ValueError, match="TermConvolution"):
        Filter(conv, state)
    with pytest.raises(ValueError, match="TermConvolution"):
        ag.filter_append_kernel(conv, state, t[:, :4], y[:, :4], yerr=yerr[:, :4])
    with pytest.raises(TypeError, match="no tensor parameter"):
        ag.filter_append_kernel(terms.RealTerm(a=0.8, c=0.3), ops.filter_init(B, 1, "cuda"), t[:, :4], y[:, :4], yerr=yerr[:, :4])


def test_plain_filter_is_unchanged_and_in_place(ops):
    """A Filter on a kernel of plain numbers: the state advances in its own storage, nothing carries a graph, and the bits are
    those of ops.filter_append on the same rows."""
    import torch
    from celerite2_amd import terms
    from celerite2_amd.stream import Filter

    B, N, t, yerr, y, _, _ = _kernel_case()
    kernel = terms.SHOTerm(S0=1.2, w0=1.1, Q=2.5) + terms.RealTerm(a=0.8, c=0.3)
    flt = Filter.empty(kernel, B, mean=0.3)
    assert not flt.differentiable
    ptr = flt.state.data_ptr()
    st = ops.filter_init(B, kernel.width, "cuda")
    for lo, hi in zip(CUTS[:4], CUTS[1:5]):
        tm, ym, em = t[:, lo:hi].contiguous(), y[:, lo:hi].contiguous(), yerr[:, lo:hi].contiguous()
        upd = flt.append(tm, ym, yerr=em)
        c, a, U, V = kernel.get_celerite_matrices(tm, em**2)
        st, d, W, z, flag = ops.filter_append(st, tm, c, a, U, V, (ym - 0.3).contiguous())
        assert flt.state.data_ptr() == ptr and not flt.state.requires_grad
        assert torch.equal(flt.state, st) and torch.equal(upd.variance, d) and torch.equal(upd.innovation, z)
    with pytest.raises(ValueError, match="jitter"):
        Filter.empty(kernel, B, jitter=0.1)


# ---- ragged counts, failures, determinism ---------------------------------------------------------------------------------
def test_ragged_counts_in_sentinel_filled_outputs(ops):
    """count includes 0 and M: zeros are written beyond count, a sentinel survives nowhere, a count-0 series gets the identity
    on its state cotangent, and the rows taken are the restatement's."""
    import torch

    J, M, n0 = 5, 6, HEAD_ROWS
    counts = np.array([0, 6, 2, 0, 1, 6, 3, 5, 0, 4], dtype=np.int32)
    B = len(counts)
    bt = batch(91, B, n0 + M, J)
    cnt, = dev(counts)
    fw = forward(ops, bt, n0, M, count=cnt)
    assert int(fw["flag"].abs().sum()) == 0
    cots = cotangents(17, B, M, J)
    dc = dev(*cots)
    sent = -7.0
    out = [torch.full(s, sent, dtype=torch.float64, device="cuda")
           for s in ((B, F.state_words(J)), (B, M), (B, J), (B, M), (B, M, J), (B, M, J), (B, M))]
    got = call(ops, fw, dc, count=cnt, out=out)
    assert all(x is o for x, o in zip(got, out))
    want = restated(fw, cots, counts)
    check_outputs("ragged", got, want, J, counts > 0)
    taken = torch.from_numpy(np.arange(M)[None, :] < counts[:, None]).cuda()
    for name, x in zip(NAMES, got):
        assert not bool((x == sent).any()), name
        if x.dim() >= 2 and x.shape[1] == M and name != "bstate_in":
            assert not bool(x[~taken].any()), name
    none = cnt == 0
    assert torch.equal(got[0][none], dc[0][none]) and not bool(got[2][none].any())


def test_failed_series_is_passed_through_and_local(ops):
    """A failing series between two good ones in one wavefront: the identity on its state cotangent, zeros in everything
    else of it, and its neighbours bit-equal to their run without the failure."""
    import torch

    J, M, n0, B = 3, 6, HEAD_ROWS, 16   # G = 4: all 16 series in one wavefront
    bt = batch(97, B, n0 + M, J)
    st0, c = dev(states_of(bt, n0), bt["c"])
    t, a, U, V, y = rows(bt, n0, n0 + M)
    cots = dev(*cotangents(23, B, M, J))

    def run(a):
        _, d, W, z, flag = ops.filter_append(st0, t, c, a, U, V, y)
        fw = dict(state=st0, t=t, c=c, U=U, W=W, d=d, z=z, flag=flag)
        return flag, call(ops, fw, cots)

    flag, good = run(a)
    assert int(flag.abs().sum()) == 0
    bad_a = a.clone()
    bad_a[5, 2] = -1.0
    bad_a[9, 0] = -1.0
    flag, got = run(bad_a)
    assert int(flag[5]) == 3 and int(flag[9]) == 1
    ok = torch.ones(B, dtype=torch.bool, device="cuda")
    ok[[5, 9]] = False
    for name, x, xg in zip(NAMES, got, good):
        assert torch.equal(x[ok], xg[ok]), name
        if name == "bstate_in":
            assert torch.equal(x[~ok], cots[0][~ok])
        else:
            assert not bool(x[~ok].any()), name


def test_two_calls_give_identical_bits(ops):
    import torch

    for J, B in ((8, 130), (17, 65)):
        bt = batch(99, B, HEAD_ROWS + 17, J)
        fw = forward(ops, bt, HEAD_ROWS, 17)
        cots = dev(*cotangents(29, B, 17, J))
        for x, x2 in zip(call(ops, fw, cots), call(ops, fw, cots)):
            assert torch.equal(x, x2)


# ---- shared t and c, offsets ------------------------------------------------------------------------------------------------
def _shared_case(ops):
    J, M, n0, B = 5, 9, HEAD_ROWS, 7
    from test_gpu_filter import reference

    cs = reference(3100, n0 + M, J)
    scale = 1.0 + np.arange(B)
    A, Y = cs["a"][None, :] + 0.01 * scale[:, None], cs["y"][None, :] * scale[:, None]
    tile = lambda x: np.ascontiguousarray(np.broadcast_to(x, (B,) + x.shape))
    heads = [F.append(F.empty(J), cs["c"], cs["t"][:n0], A[b, :n0], cs["U"][:n0], cs["V"][:n0], Y[b, :n0]) for b in range(B)]
    assert all(h[4] == 0 for h in heads)
    st0, t1, c1, tB, cB = dev(np.stack([h[0] for h in heads]), cs["t"][n0:], cs["c"], tile(cs["t"][n0:]), tile(cs["c"]))
    a, U, V, y = dev(A[:, n0:], tile(cs["U"][n0:]), tile(cs["V"][n0:]), Y[:, n0:])
    return J, M, B, st0, t1, c1, tB, cB, a, U, V, y


def test_shared_t_and_c_and_odd_offsets(ops):
    """t and c shared by the batch (stride 0) give the bits of the same values repeated per series, bt (B, M) and bc (B, J)
    per series all the same; every array starting at an odd element gives the bits of the aligned call; the autograd layer
    returns the batch sum for the shared arguments."""
    import torch
    from celerite2_amd import autograd as ag

    J, M, B, st0, t1, c1, tB, cB, a, U, V, y = _shared_case(ops)
    cnt, = dev(np.array([9, 0, 4, 9, 1, 7, 2], dtype=np.int32))
    _, d, W, z, flag = ops.filter_append(st0, tB, cB, a, U, V, y, count=cnt)
    assert int(flag.abs().sum()) == 0
    d, W, z = (torch.nan_to_num(x) for x in (d, W, z))   # (rows beyond count were never written)
    cots = dev(*cotangents(31, B, M, J))
    base = ops.filter_append_rev(st0, tB, cB, U, W, d, z, flag, *cots, count=cnt)
    shared = ops.filter_append_rev(st0, t1, c1, U, W, d, z, flag, *cots, count=cnt)
    assert tuple(shared[1].shape) == (B, M) and tuple(shared[2].shape) == (B, J)
    for name, x, xb in zip(NAMES, shared, base):
        assert torch.equal(x, xb), name
    o = _odd
    sent = lambda x: torch.full_like(x, -7.0)
    odd = ops.filter_append_rev(o(st0), o(t1), o(c1), o(U), o(W), o(d), o(z), o(flag), *(o(x) for x in cots), count=o(cnt),
                                ws=o(torch.empty((B, M, J + J * J), dtype=torch.float64, device="cuda")),
                                out=[o(sent(x)) for x in base])
    for name, x, xb in zip(NAMES, odd, base):
        assert torch.equal(x, xb), name
    # bd, bW, bz are optional: None is zeros
    zeros = [cots[0]] + [torch.zeros_like(x) for x in cots[1:]]
    for x, xb in zip(ops.filter_append_rev(st0, t1, c1, U, W, d, z, flag, cots[0], count=cnt),
                     ops.filter_append_rev(st0, t1, c1, U, W, d, z, flag, *zeros, count=cnt)):
        assert torch.equal(x, xb)
    # the autograd layer: the batch sum for shared t and c
    ts, cs_ = t1.clone().requires_grad_(), c1.clone().requires_grad_()
    out = ag.filter_append(st0, ts, cs_, a, U, V, y)
    loss = sum((x * b).sum() for x, b in zip(out[:4], (cots[0], cots[1], cots[2], cots[3])))
    gt, gc = torch.autograd.grad(loss, (ts, cs_))
    full = ops.filter_append_rev(st0, t1, c1, U, out[2].detach(), out[1].detach(), out[3].detach(), out[4], *cots)
    assert tuple(gt.shape) == (M,) and tuple(gc.shape) == (J,)
    assert torch.equal(gt, full[1].sum(0)) and torch.equal(gc, full[2].sum(0))


def test_empty_state_far_below_t_last(ops):
    """n == 0 under a stale t_last of +1e6 and times near -1e4: no NaN anywhere, bc and bt equal to those under t_last = 0,
    and nothing flows into the empty state."""
    import torch

    for J in (2, 8):
        bt = batch(95, 3, 4, J)
        t, c, a, U, V, y = dev(bt["t"] - 1e4, bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
        cots = dev(*cotangents(37, 3, 4, J))
        res = []
        for tl in (1e6, 0.0):
            st = ops.filter_init(3, J, "cuda")
            st[:, 0] = tl
            _, d, W, z, flag = ops.filter_append(st, t, c, a, U, V, y)
            assert int(flag.abs().sum()) == 0
            res.append(ops.filter_append_rev(st, t, c, U, W, d, z, flag, *cots))
        for name, x, xo in zip(NAMES, *res):
            assert bool(torch.isfinite(x).all()) and torch.equal(x, xo), name
        assert not bool(res[0][0][:, 0].any()) and not bool(res[0][0][:, 4:].any())
