# -*- coding: utf-8 -*-
"""CPU checks of the reverse of a streaming forecast and of a streaming absorb: the numpy restatements
(tests/filter_stream_rev_ref.py, what the GPU tests compare the kernels with) against torch autograd of torch float64
restatements of filter_ref.forecast and filter_ref.absorb, the forecast reverse behind a chain of appends against the exact
dense derivative of sum log N(tail | head), ragged counts, the empty state under a stale t_last, and the header and argument
validation of include/celerite2_amd_filter_stream_rev.h through the loaded library.

Criterion everywhere: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (inverse_diag_ref.err); an expected array
that is all zero has a floor of 1 (the cotangents are unit normal draws).  The draws are those of tests/test_filter_rev.py
(kappa = max a / d <= 100, asserted there per draw)."""
import ctypes

import numpy as np
import pytest
import torch

import filter_ref as F
import filter_rev_ref as R
import filter_stream_rev_ref as Q
from test_filter_rev import CUTS, WIDTHS, _blocks, _case, _torch_dense, chain_case

assert WIDTHS == [1, 2, 3, 5, 8, 16, 32]
MS = (1, 2, 17)


def _err(x, xo):
    xo = np.asarray(xo, dtype=float)
    return F.err(x, xo, None if xo.any() else 1.0)


def _check(key, x, xo):
    e = _err(x, xo)
    assert e <= 1.0, (key, e)


def _grads(loss, ins):
    """torch.autograd.grad with zeros where nothing depends on an input (the F, S, t_last of an empty state)."""
    return [np.zeros(tuple(i.shape)) if g is None else g.numpy() for g, i in zip(torch.autograd.grad(loss, ins, allow_unused=True), ins)]


def _tensors(cs, keys):
    return [torch.tensor(cs[k], dtype=torch.float64, requires_grad=True) for k in keys]


# ---- the restatements against torch autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("J", WIDTHS)
def test_forecast_restatement_is_autograd_of_the_forecast(J):
    """Random cotangents on mu and var, from an empty and a non-empty state, M = 1, 2, 17: every output, the S block compared
    as the symmetric representative and symmetric to the bit."""
    for nonempty in (False, True):
        for M in MS:
            cs = _case(J, M, nonempty, 100 + 10 * J + M)
            rng = np.random.default_rng(11 * J + M)
            bmu, bvar = rng.normal(size=M), rng.normal(size=M)
            ins = _tensors(cs, ("state", "c", "t", "a", "U"))
            mu, var = Q.torch_forecast(*ins)
            g = _grads((mu * torch.tensor(bmu)).sum() + (var * torch.tensor(bvar)).sum(), ins)
            got = Q.forecast_rev(cs["state"], cs["c"], cs["t"], cs["U"], bmu, bvar)
            gs = R.symmetrise(g[0], J)
            S = got[0][R.HEAD + J:].reshape(J, J)
            assert np.array_equal(S, S.T)
            assert not got[0][1:R.HEAD].any()
            for name, sl in _blocks(J):
                _check((J, M, nonempty, "bstate " + name), got[0][sl], gs[sl])
            for name, x, xo in zip(("bt", "bc", "ba", "bU"), got[1:], (g[2], g[1], g[3], g[4])):
                _check((J, M, nonempty, name), x, xo)
            if not nonempty:   # ba = bvar, zeros everywhere else
                assert np.array_equal(got[3], bvar) and not any(np.any(x) for i, x in enumerate(got) if i != 3)


@pytest.mark.parametrize("J", WIDTHS)
def test_absorb_restatement_is_autograd_of_the_absorb(J):
    """A random cotangent on the state left (all four head words, a non-symmetric S block), from an empty and a non-empty
    entry state, M = 1, 2, 17."""
    for nonempty in (False, True):
        for M in MS:
            cs = _case(J, M, nonempty, 100 + 10 * J + M)
            assert np.array_equal(F.absorb(cs["state"], cs["c"], cs["t"], cs["W"], cs["d"], cs["z"])[:2], cs["out"][:2])
            bs = np.random.default_rng(13 * J + M).normal(size=F.state_words(J))
            ins = _tensors(cs, ("state", "c", "t", "W", "d", "z"))
            g = _grads((Q.torch_absorb(*ins) * torch.tensor(bs)).sum(), ins)
            got = Q.absorb_rev(cs["state"], cs["c"], cs["t"], cs["W"], cs["d"], cs["z"], bs)
            gs = R.symmetrise(g[0], J)
            S = got[0][R.HEAD + J:].reshape(J, J)
            assert np.array_equal(S, S.T)
            for name, sl in _blocks(J):
                _check((J, M, nonempty, "bstate_in " + name), got[0][sl], gs[sl])
            for name, x, xo in zip(("bt", "bc", "bW", "bd", "bz"), got[1:6], (g[2], g[1], g[3], g[4], g[5])):
                _check((J, M, nonempty, name), x, xo)


def test_ragged_counts():
    """count = M is no count; count = k is the reverse of the first k rows, zeros behind; count = 0 gives a zero state
    cotangent from the forecast reverse and the identity from the absorb reverse."""
    J, M, k = 5, 17, 6
    cs = _case(J, M, True, 31)
    rng = np.random.default_rng(3)
    bs, bmu, bvar = rng.normal(size=F.state_words(J)), rng.normal(size=M), rng.normal(size=M)
    fargs = (cs["state"], cs["c"], cs["t"], cs["U"], bmu, bvar)
    for x, xo in zip(Q.forecast_rev(*fargs, count=M), Q.forecast_rev(*fargs)):
        assert np.array_equal(x, xo)
    part = Q.forecast_rev(*fargs, count=k)
    ref = Q.forecast_rev(cs["state"], cs["c"], cs["t"][:k], cs["U"][:k], bmu[:k], bvar[:k])
    assert np.array_equal(part[0], ref[0]) and np.array_equal(part[2], ref[2])
    for i in (1, 3, 4):
        assert np.array_equal(part[i][:k], ref[i]) and not part[i][k:].any(), i
    assert not any(x.any() for x in Q.forecast_rev(*fargs, count=0))

    aargs = (cs["state"], cs["c"], cs["t"], cs["W"], cs["d"], cs["z"], bs)
    for x, xo in zip(Q.absorb_rev(*aargs, count=M), Q.absorb_rev(*aargs)):
        assert np.array_equal(x, xo, equal_nan=True)
    part = Q.absorb_rev(*aargs, count=k)
    ref = Q.absorb_rev(cs["state"], cs["c"], cs["t"][:k], cs["W"][:k], cs["d"][:k], cs["z"][:k], bs)
    assert np.array_equal(part[0], ref[0]) and np.array_equal(part[2], ref[2])
    for i in (1, 3, 4, 5):
        assert np.array_equal(part[i][:k], ref[i]) and not part[i][k:].any(), i
    none = Q.absorb_rev(*aargs, count=0)
    assert np.array_equal(none[0], bs) and not any(x.any() for x in none[1:6])


def test_empty_state_ignores_t_last():
    """n == 0: p := 0 whatever t_last holds -- no NaN anywhere, and the same result as under t_last = 0."""
    J, M = 4, 5
    cs = _case(J, M, False, 11)
    rng = np.random.default_rng(9)
    bs, bmu, bvar = rng.normal(size=F.state_words(J)), rng.normal(size=M), rng.normal(size=M)
    stale = cs["state"].copy()
    stale[0] = 1e6
    t = cs["t"] - 1e4
    got = Q.forecast_rev(stale, cs["c"], t, cs["U"], bmu, bvar)
    ref = Q.forecast_rev(cs["state"], cs["c"], t, cs["U"], bmu, bvar)
    assert all(np.all(np.isfinite(x)) for x in got)
    assert all(np.array_equal(x, xo) for x, xo in zip(got, ref))
    assert np.array_equal(got[3], bvar) and not any(np.any(x) for i, x in enumerate(got) if i != 3)
    got = Q.absorb_rev(stale, cs["c"], t, cs["W"], cs["d"], cs["z"], bs)
    ref = Q.absorb_rev(cs["state"], cs["c"], t, cs["W"], cs["d"], cs["z"], bs)
    assert all(np.all(np.isfinite(x)) for x in got[:6])
    assert all(np.array_equal(x, xo) for x, xo in zip(got[:6], ref[:6]))
    assert got[0][0] == 0.0 and not got[0][R.HEAD:].any()


# ---- the forecast behind a chain of calls against dense conditioning -----------------------------------------------------
N0 = 120   # rows of the head; the tail is the 30 rows behind it


def _dense_tail_density(cs):
    """sum_m log N(y_m | mu_m, var_m) over the tail, each row conditioned on the head alone, and its exact gradient in
    t, c, a, U, V, y -- dense algebra in torch float64."""
    ins = _tensors(cs, "tcaUVy")
    K = _torch_dense(*ins[:5])
    y = ins[5]
    sol = torch.linalg.solve(K[:N0, :N0], torch.cat([y[:N0, None], K[:N0, N0:]], dim=1))
    mu = K[N0:, :N0] @ sol[:, 0]
    var = torch.diagonal(K)[N0:] - torch.einsum("mn,nm->m", K[N0:, :N0], sol[:, 1:])
    L = (-0.5 * ((y[N0:] - mu) ** 2 / var + torch.log(var) + np.log(2 * np.pi))).sum()
    return float(L.detach()), dict(zip("tcaUVy", (x.numpy() for x in torch.autograd.grad(L, ins))))


def _density_cotangents(y, mu, var):
    r = y - mu
    return -0.5 * (r * r / var + np.log(var) + np.log(2 * np.pi)), r / var, 0.5 * (r * r / (var * var) - 1.0 / var)


def test_forecast_behind_appends_is_the_dense_derivative():
    """150 rows: the head appended in six calls, the tail forecast from the state behind it.  The gradient of
    sum log N(tail | head) in t, c, a, U, V and y -- the forecast reverse at the tail, its state cotangent carried back
    through the appends by filter_rev_ref -- is the dense one."""
    cs = chain_case()
    N, J = 150, 8
    L_o, g_o = _dense_tail_density(cs)
    st, calls = F.empty(J), []
    cuts = [x for x in CUTS if x < N0] + [N0]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out, d, W, z, flag = F.append(st, cs["c"], *(cs[k][lo:hi] for k in "taUVy"))
        assert flag == 0
        calls.append((lo, hi, st, d, W, z))
        st = out
    mu, var = F.forecast(st, cs["c"], cs["t"][N0:], cs["a"][N0:], cs["U"][N0:])
    dens, bmu, bvar = _density_cotangents(cs["y"][N0:], mu, var)
    assert abs(dens.sum() - L_o) <= 1e-10 * abs(L_o)
    g = dict(t=np.zeros(N), c=np.zeros(J), a=np.zeros(N), U=np.zeros((N, J)), V=np.zeros((N, J)), y=np.zeros(N))
    bs, bt, bc, ba, bU = Q.forecast_rev(st, cs["c"], cs["t"][N0:], cs["U"][N0:], bmu, bvar)
    g["c"] += bc
    g["t"][N0:], g["a"][N0:], g["U"][N0:], g["y"][N0:] = bt, ba, bU, -bmu
    for lo, hi, s0, d, W, z in reversed(calls):
        bs, bt, bc, ba, bU, bV, by, _ = R.append_rev(s0, cs["c"], cs["t"][lo:hi], cs["U"][lo:hi], W, d, z, 0, bs)
        g["c"] += bc
        for k, x in zip("taUVy", (bt, ba, bU, bV, by)):
            g[k][lo:hi] += x
    assert bs[0] == 0.0 and not bs[R.HEAD:].any()   # nothing flows into the empty state
    for k in "tcaUVy":
        _check(k, g[k], g_o[k])


def test_forecast_behind_an_absorb_composes():
    """The same head absorbed from its factors in two calls: the state is the appended one, and the forecast reverse followed
    by the absorb reverse is torch autograd of the composed torch restatements, in t, c, W, d, z of the head and t, a, U of
    the tail."""
    cs = chain_case()
    J, cut = 8, 47
    d, W = F.factor(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
    z = F.solve_lower(cs["t"], cs["c"], cs["U"], W, cs["y"])
    head = dict(c=cs["c"], t=cs["t"][:N0], W=W[:N0], d=d[:N0], z=z[:N0])
    s1 = F.absorb(F.empty(J), cs["c"], head["t"][:cut], head["W"][:cut], head["d"][:cut], head["z"][:cut])
    s2 = F.absorb(s1, cs["c"], head["t"][cut:], head["W"][cut:], head["d"][cut:], head["z"][cut:])
    s_app = F.append(F.empty(J), cs["c"], *(cs[k][:N0] for k in "taUVy"))[0]
    _check("state", s2[2:], s_app[2:])
    mu, var = F.forecast(s2, cs["c"], cs["t"][N0:], cs["a"][N0:], cs["U"][N0:])
    _, bmu, bvar = _density_cotangents(cs["y"][N0:], mu, var)

    ins = _tensors(head, ("c", "t", "W", "d", "z")) + _tensors(dict(t=cs["t"][N0:], a=cs["a"][N0:], U=cs["U"][N0:]), "taU")
    c_, t_, W_, d_, z_, tt, at, Ut = ins
    e = torch.tensor(F.empty(J))
    st = Q.torch_absorb(Q.torch_absorb(e, c_, t_[:cut], W_[:cut], d_[:cut], z_[:cut]), c_, t_[cut:], W_[cut:], d_[cut:], z_[cut:])
    mu_t, var_t = Q.torch_forecast(st, c_, tt, at, Ut)
    yt = torch.tensor(cs["y"][N0:])
    g = _grads((-0.5 * ((yt - mu_t) ** 2 / var_t + torch.log(var_t))).sum(), ins)

    bs, btt, bc, bat, bUt = Q.forecast_rev(s2, cs["c"], cs["t"][N0:], cs["U"][N0:], bmu, bvar)
    b1, bt2, bc2, bW2, bd2, bz2, _ = Q.absorb_rev(s1, cs["c"], head["t"][cut:], head["W"][cut:], head["d"][cut:], head["z"][cut:], bs)
    b0, bt1, bc1, bW1, bd1, bz1, _ = Q.absorb_rev(F.empty(J), cs["c"], head["t"][:cut], head["W"][:cut], head["d"][:cut],
                                                 head["z"][:cut], b1)
    assert b0[0] == 0.0 and not b0[R.HEAD:].any()
    got = (bc + bc1 + bc2, np.concatenate([bt1, bt2]), np.concatenate([bW1, bW2]), np.concatenate([bd1, bd2]),
           np.concatenate([bz1, bz2]), btt, bat, bUt)
    for name, x, xo in zip(("c", "t", "W", "d", "z", "t tail", "a tail", "U tail"), got, g):
        _check(name, x, xo)


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib


def test_header_symbols_exported(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import autograd

    for name in ("filter_forecast", "filter_absorb", "filter_forecast_kernel", "filter_absorb_kernel"):
        assert name in autograd.__all__ and callable(getattr(autograd, name))


def test_abi_argument_errors(lib):
    """Both entry points reject non-positive sizes and null pointers (C2_ERR_INVALID) and widths above C2_FAST_WIDTH
    (C2_ERR_UNSUPPORTED) before anything touches the device.  count is nullable."""
    L = lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first
    INVALID, UNSUPPORTED = lib.C2_ERR_INVALID, lib.C2_ERR_UNSUPPORTED

    def forecast(B, M, J, p, count=null):
        # p: state, t, c, U, bmu, bvar, bstate, bt, bc, ba, bU
        return L.c2_filter_forecast_rev(i64(B), i64(M), i64(J), p[0], p[1], i64(0), p[2], i64(0), p[3], count, *p[4:], null)

    def absorb(B, M, J, p, count=null):
        # p: state_in, t, c, W, d, z, bstate_out, ws, bstate_in, bt, bc, bW, bd, bz
        return L.c2_filter_absorb_rev(i64(B), i64(M), i64(J), p[0], p[1], i64(0), p[2], i64(0), p[3], p[4], p[5], count, *p[6:],
                                      null)

    for rev, nptr in ((forecast, 11), (absorb, 14)):
        full = [one] * nptr
        assert rev(1, 4, 2, [null] * nptr) == INVALID
        for k in range(nptr):   # each pointer in turn
            assert rev(1, 4, 2, full[:k] + [null] + full[k + 1:]) == INVALID, (rev.__name__, k)
            assert rev(1, 4, 2, full[:k] + [null] + full[k + 1:], one) == INVALID, (rev.__name__, k)
        assert rev(0, 4, 2, full) == INVALID
        assert rev(1, 0, 2, full) == INVALID
        assert rev(1, 4, 0, full) == INVALID
        assert rev(-1, 4, 2, full) == INVALID
        assert rev(1, 4, 33, full) == UNSUPPORTED
        assert rev(1, 4, 33, [null] * nptr) == UNSUPPORTED
        assert rev(1, 2**31, 2, full) == UNSUPPORTED   # count is int32
