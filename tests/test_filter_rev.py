# -*- coding: utf-8 -*-
"""CPU checks of the reverse of a streaming append: the numpy restatement (tests/filter_rev_ref.py, what the GPU tests
compare the kernel with) against torch autograd of a torch float64 restatement of the append, the state cotangent carried
through a chain of calls against the exact dense derivative of the whole-series log-likelihood, ragged and failed series,
and the header and argument validation of include/celerite2_amd_filter_rev.h through the loaded library.

Criterion everywhere: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (inverse_diag_ref.err); an expected array
that is all zero takes the largest incoming cotangent as its floor.  Every draw has kappa = max a / d <= 100, asserted per
draw, so the 0.4 eps kappa^2 floor of DESIGN section 6 (4e-13) stays under the criterion."""
import ctypes

import numpy as np
import pytest
import torch

import filter_ref as F
import filter_rev_ref as R

WIDTHS = [1, 2, 3, 5, 8, 16, 32]
N0 = 9   # rows behind a non-empty entry state


def _err(x, xo, scale):
    xo = np.asarray(xo, dtype=float)
    floor = float(np.max(np.abs(xo)))
    return F.err(x, xo, floor if floor > 0.0 else scale)


def _case(J, M, nonempty, seed):
    """A draw of N0 * nonempty + M rows, the entry state in front of the last M, the append of those and kappa."""
    n0 = N0 if nonempty else 0
    cs = F.draw(seed, n0 + M, J)
    st = F.empty(J)
    kappa = 0.0
    if n0:
        st, d, _, _, flag = F.append(st, cs["c"], *(cs[k][:n0] for k in "taUVy"))
        assert flag == 0
        kappa = float(np.max(cs["a"][:n0] / d))
    rows = {k: cs[k][n0:] for k in "taUVy"}
    out, d, W, z, flag = F.append(st, cs["c"], *(rows[k] for k in "taUVy"))
    assert flag == 0
    kappa = max(kappa, float(np.max(rows["a"] / d)))
    assert kappa <= 100.0, (J, M, nonempty, kappa)
    return dict(c=cs["c"], state=st, out=out, d=d, W=W, z=z, **rows)


def _blocks(J):
    return (("head", slice(0, R.HEAD)), ("F", slice(R.HEAD, R.HEAD + J)), ("S", slice(R.HEAD + J, None)))


@pytest.mark.parametrize("J", WIDTHS)
def test_restatement_is_autograd_of_the_append(J):
    """Random cotangents on every output (all four head words of the state, a non-symmetric S block) from an empty and a
    non-empty entry state, M = 1, 2, 17."""
    for nonempty in (False, True):
        for M in (1, 2, 17):
            cs = _case(J, M, nonempty, 100 + 10 * J + M)
            rng = np.random.default_rng(7 * J + M)
            bs, bd, bW, bz = (rng.normal(size=s) for s in (F.state_words(J), M, (M, J), M))
            scale = max(np.abs(x).max() for x in (bs, bd, bW, bz))
            ins = [torch.tensor(cs[k], dtype=torch.float64, requires_grad=True) for k in ("state", "c", "t", "a", "U", "V", "y")]
            outs = R.torch_append(*ins)
            loss = sum((o * torch.tensor(b)).sum() for o, b in zip(outs, (bs, bd, bW, bz)))
            g = [np.zeros(tuple(i.shape)) if x is None else x.numpy()   # (nothing depends on the F, S, t_last of an empty state)
                 for x, i in zip(torch.autograd.grad(loss, ins, allow_unused=True), ins)]
            got = R.append_rev(cs["state"], cs["c"], cs["t"], cs["U"], cs["W"], cs["d"], cs["z"], 0, bs, bd, bW, bz)
            gs = R.symmetrise(g[0], J)
            S = got[0][R.HEAD + J:].reshape(J, J)
            assert np.array_equal(S, S.T)
            for name, sl in _blocks(J):
                e = _err(got[0][sl], gs[sl], scale)
                assert e <= 1.0, (J, M, nonempty, "bstate_in " + name, e)
            for name, x, xo in zip(("bt", "bc", "ba", "bU", "bV", "by"), got[1:7], (g[2], g[1], g[3], g[4], g[5], g[6])):
                e = _err(x, xo, scale)
                assert e <= 1.0, (J, M, nonempty, name, e)


def _torch_dense(t, c, a, U, V):
    dt = torch.abs(t[:, None] - t[None, :])
    K = torch.tril(torch.einsum("nj,mj,nmj->nm", U, V, torch.exp(-c[None, None, :] * dt[:, :, None])), -1)
    return K + K.T + torch.diag(a)


CUTS = [0, 1, 2, 7, 23, 40, 150]   # 1, 1, 5, 16, 17 rows and the rest


def chain_case(seed=21, N=150, J=8):
    cs = F.draw(seed, N, J)
    ins = [torch.tensor(cs[k], dtype=torch.float64, requires_grad=True) for k in "tcaUVy"]
    K = _torch_dense(*ins[:5])
    y = ins[5]
    ll = -0.5 * (y @ torch.linalg.solve(K, y) + torch.linalg.slogdet(K)[1] + N * np.log(2 * np.pi))
    cs["grads"] = dict(zip("tcaUVy", (x.numpy() for x in torch.autograd.grad(ll, ins))))
    cs["ll"] = float(ll.detach())
    return cs


def ll_cotangent(J):
    """The cotangent of the last state under the loss log-likelihood = -(1/2) ([3] + [2] + n log 2 pi)."""
    b = np.zeros(F.state_words(J))
    b[1], b[2], b[3] = -0.5 * np.log(2 * np.pi), -0.5, -0.5
    return b


def test_chain_is_the_dense_derivative():
    """150 rows appended as 1, 1, 5, 16, 17 and the rest; the state cotangent carried backwards through the six calls gives
    the exact dense derivative of the whole-series log-likelihood in t, c, a, U, V, y."""
    cs = chain_case()
    N, J = 150, 8
    st, calls = F.empty(J), []
    for lo, hi in zip(CUTS[:-1], CUTS[1:]):
        out, d, W, z, flag = F.append(st, cs["c"], *(cs[k][lo:hi] for k in "taUVy"))
        assert flag == 0 and float(np.max(cs["a"][lo:hi] / d)) <= 100.0
        calls.append((lo, hi, st, d, W, z))
        st = out
    assert abs(F.log_likelihood(st) - cs["ll"]) <= 1e-10 * abs(cs["ll"])
    bs = ll_cotangent(J)
    g = dict(t=np.zeros(N), c=np.zeros(J), a=np.zeros(N), U=np.zeros((N, J)), V=np.zeros((N, J)), y=np.zeros(N))
    for lo, hi, s0, d, W, z in reversed(calls):
        bs, bt, bc, ba, bU, bV, by, _ = R.append_rev(s0, cs["c"], cs["t"][lo:hi], cs["U"][lo:hi], W, d, z, 0, bs)
        g["c"] += bc
        for k, x in zip("taUVy", (bt, ba, bU, bV, by)):
            g[k][lo:hi] += x
    assert bs[0] == 0.0 and not bs[R.HEAD:].any()   # nothing flows into the empty state
    for k in "tcaUVy":
        e = F.err(g[k], cs["grads"][k])
        assert e <= 1.0, (k, e)


def test_ragged_counts():
    """count = M is no count; count = k is the reverse of the first k rows, zeros behind; count = 0 is the identity."""
    J, M = 5, 17
    cs = _case(J, M, True, 31)
    rng = np.random.default_rng(3)
    bs, bd, bW, bz = (rng.normal(size=s) for s in (F.state_words(J), M, (M, J), M))
    args = (cs["state"], cs["c"], cs["t"], cs["U"], cs["W"], cs["d"], cs["z"], 0, bs, bd, bW, bz)
    full = R.append_rev(*args)
    for x, xo in zip(R.append_rev(*args, count=M), full):
        assert np.array_equal(x, xo, equal_nan=True)
    k = 6
    part = R.append_rev(*args, count=k)
    ref = R.append_rev(cs["state"], cs["c"], cs["t"][:k], cs["U"][:k], cs["W"][:k], cs["d"][:k], cs["z"][:k], 0, bs, bd[:k],
                       bW[:k], bz[:k])
    assert np.array_equal(part[0], ref[0]) and np.array_equal(part[2], ref[2])
    for i in (1, 3, 4, 5, 6):
        assert np.array_equal(part[i][:k], ref[i]) and not part[i][k:].any(), i
    none = R.append_rev(*args, count=0)
    assert np.array_equal(none[0], bs) and not any(x.any() for x in none[1:7])


def test_failed_series_is_passed_through():
    """A series whose forward call failed: the identity on the state cotangent (not symmetrised), zeros elsewhere, and the
    series beside it in a batch are what they are alone."""
    J, M = 4, 5
    rng = np.random.default_rng(5)
    series = [_case(J, M, True, 40 + b) for b in range(3)]
    cots = [[rng.normal(size=s) for s in (F.state_words(J), M, (M, J), M)] for _ in range(3)]
    a = series[1]["a"].copy()
    a[2] = -1.0
    s1, d, W, z, flag = F.append(series[1]["state"], series[1]["c"], series[1]["t"], a, series[1]["U"], series[1]["V"],
                                 series[1]["y"])
    assert flag == 3 and np.array_equal(s1, series[1]["state"])
    series[1].update(d=d, W=W, z=z)
    flags = [0, flag, 0]
    got = [R.append_rev(cs["state"], cs["c"], cs["t"], cs["U"], cs["W"], cs["d"], cs["z"], f, *cot)
           for cs, f, cot in zip(series, flags, cots)]
    assert np.array_equal(got[1][0], cots[1][0]) and not any(x.any() for x in got[1][1:7])
    for b in (0, 2):
        assert all(np.all(np.isfinite(x)) for x in got[b][:7]) and got[b][4].any()


def test_empty_state_ignores_t_last():
    """n == 0: p := 0 whatever t_last holds -- no NaN in bc, bt, and the same result as under t_last = 0."""
    J, M = 4, 5
    cs = _case(J, M, False, 11)
    rng = np.random.default_rng(9)
    cot = [rng.normal(size=s) for s in (F.state_words(J), M, (M, J), M)]
    stale = cs["state"].copy()
    stale[0] = 1e6
    t = cs["t"] - 1e4
    got = R.append_rev(stale, cs["c"], t, cs["U"], cs["W"], cs["d"], cs["z"], 0, *cot)
    ref = R.append_rev(cs["state"], cs["c"], t, cs["U"], cs["W"], cs["d"], cs["z"], 0, *cot)
    assert all(np.all(np.isfinite(x)) for x in got[:7])
    for x, xo in zip(got[:7], ref[:7]):
        assert np.array_equal(x, xo)
    assert got[0][0] == 0.0 and not got[0][R.HEAD:].any()


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib


def test_header_symbols_exported(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    for J, words in ((1, 2), (8, 72), (32, 1056), (0, 0), (33, 0), (-1, 0)):
        assert lib.load().c2_filter_rev_workspace_words(J) == words, J
        if words:
            assert R.workspace_words(J) == words


def test_abi_argument_errors(lib):
    """The entry point rejects non-positive sizes and null pointers (C2_ERR_INVALID) and widths above C2_FAST_WIDTH
    (C2_ERR_UNSUPPORTED) before anything touches the device.  count, bd, bW and bz are nullable."""
    L = lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first
    INVALID, UNSUPPORTED = lib.C2_ERR_INVALID, lib.C2_ERR_UNSUPPORTED

    def rev(B, M, J, p, opt=(null, null, null, null)):
        # p: state_in, t, c, U, W, d, z, flag, bstate_out, ws, bstate_in, bt, bc, ba, bU, bV, by;  opt: count, bd, bW, bz
        return L.c2_filter_append_rev(i64(B), i64(M), i64(J), p[0], p[1], i64(0), p[2], i64(0), p[3], p[4], p[5], p[6], opt[0],
                                      p[7], p[8], opt[1], opt[2], opt[3], p[9], p[10], p[11], p[12], p[13], p[14], p[15],
                                      p[16], null)

    nptr = 17
    full = [one] * nptr
    assert rev(1, 4, 2, [null] * nptr) == INVALID
    for k in range(nptr):   # each pointer in turn
        assert rev(1, 4, 2, full[:k] + [null] + full[k + 1:]) == INVALID, k
        assert rev(1, 4, 2, full[:k] + [null] + full[k + 1:], (one,) * 4) == INVALID, k
    assert rev(0, 4, 2, full) == INVALID
    assert rev(1, 0, 2, full) == INVALID
    assert rev(1, 4, 0, full) == INVALID
    assert rev(1, 4, 33, full) == UNSUPPORTED
    assert rev(1, 4, 33, [null] * nptr) == UNSUPPORTED
    assert rev(1, 2**31, 2, full) == UNSUPPORTED   # count is int32
