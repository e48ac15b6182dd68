# -*- coding: utf-8 -*-
"""CPU checks of the streaming updates: the numpy restatement of the three modes (tests/filter_ref.py, what the GPU tests
compare the kernel with) against the reference's recursions over the whole series and against dense algebra, and the argument
validation of the four entry points of include/celerite2_amd_filter.h through the loaded library.

Criterion everywhere: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (inverse_diag_ref.err).  Every draw has a
condition number <= 1e6, asserted per draw."""
import ctypes

import numpy as np
import pytest

import filter_ref as F

# (seed, N, J, gap in time, noise range in units of k(0))
DRAWS = [(1, 40, 1, False, (0.05, 0.5)), (2, 40, 2, False, (0.05, 0.5)), (3, 70, 3, False, (0.05, 0.5)),
         (4, 70, 8, True, (0.05, 0.5)), (5, 150, 8, False, (1e-3, 10.0)), (6, 97, 16, False, (0.05, 0.5)),
         (7, 97, 32, False, (0.05, 0.5)), (8, 150, 5, True, (1e-3, 1e-2))]


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed, N, J, gap, noise in DRAWS:
        cs = F.draw(seed, N, J, gap=gap, noise=noise)
        cs["K"] = F.dense(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
        cond = np.linalg.cond(cs["K"])
        assert cond <= 1e6, (seed, cond)   # a bad draw fails here instead of loosening anything below
        cs["d"], cs["W"] = F.factor(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
        cs["z"] = F.solve_lower(cs["t"], cs["c"], cs["U"], cs["W"], cs["y"])
        cs["N"], cs["J"] = N, J
        out.append(("draw%d_N%d_J%d%s" % (seed, N, J, "_gap" if gap else ""), cs))
    return out


def _chunked(cs, cuts):
    st, parts = F.empty(cs["J"]), []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        st, d, W, z, flag = F.append(st, cs["c"], *(cs[k][lo:hi] for k in "taUVy"))
        assert flag == 0
        parts.append((d, W, z))
    return st, [np.concatenate([p[i] for p in parts]) for i in range(3)]


def test_chunked_append_is_factor_and_solve_lower(cases):
    """Appending 1, 1, 5, ... rows from the empty state gives the d, W, z of the whole series, and the count n."""
    for name, cs in cases:
        N = cs["N"]
        st, (d, W, z) = _chunked(cs, [0, 1, 2, 7, N // 2, N - 3, N])
        for x, xo in ((d, cs["d"]), (W, cs["W"]), (z, cs["z"])):
            assert F.err(x, xo) <= 1.0, (name, F.err(x, xo))
        assert st[0] == cs["t"][-1] and st[1] == N, name
        S = st[F.HEAD + cs["J"]:].reshape(cs["J"], cs["J"])
        assert np.array_equal(S, S.T), name


def test_log_likelihood_is_the_dense_one(cases):
    for name, cs in cases:
        N, K, y = cs["N"], cs["K"], cs["y"]
        st, _ = _chunked(cs, [0, 3, N])
        ll_o = -0.5 * (y @ np.linalg.solve(K, y) + np.linalg.slogdet(K)[1] + N * np.log(2 * np.pi))
        assert abs(F.log_likelihood(st) - ll_o) <= 1e-10 * abs(ll_o), name


def test_absorb_is_the_closed_form(cases):
    """Absorbing the first n0 rows of a factorisation gives the closed-form state; appending the rest of the series from
    either gives the rest of the factorisation and the state of the chunked append."""
    for name, cs in cases:
        N, J = cs["N"], cs["J"]
        n0 = N // 2 + 1
        s_abs = F.absorb(F.empty(J), cs["c"], cs["t"][:n0], cs["W"][:n0], cs["d"][:n0], cs["z"][:n0])
        s_cf = F.closed_form(cs["t"], cs["c"], cs["W"], cs["d"], cs["z"], n0)
        assert s_abs[0] == s_cf[0] and s_abs[1] == s_cf[1], name
        assert F.err(s_abs[2:4], s_cf[2:4]) <= 1.0, name
        assert F.err(s_abs[F.HEAD:F.HEAD + J], s_cf[F.HEAD:F.HEAD + J]) <= 1.0, name
        assert F.err(s_abs[F.HEAD + J:], s_cf[F.HEAD + J:]) <= 1.0, name
        full, _ = _chunked(cs, [0, N])
        for s0 in (s_abs, s_cf):
            s1, d, W, z, flag = F.append(s0, cs["c"], *(cs[k][n0:] for k in "taUVy"))
            assert flag == 0
            for x, xo in ((d, cs["d"][n0:]), (W, cs["W"][n0:]), (z, cs["z"][n0:]), (s1[F.HEAD + J:], full[F.HEAD + J:]),
                          (s1[F.HEAD:F.HEAD + J], full[F.HEAD:F.HEAD + J])):
                assert F.err(x, xo) <= 1.0, (name, F.err(x, xo))


def test_forecast_is_dense_conditioning(cases):
    """From the state behind row n0 - 1, every later row's forecast is its dense conditional on the first n0 rows."""
    for name, cs in cases:
        N, J, K, y = cs["N"], cs["J"], cs["K"], cs["y"]
        n0 = N // 2 + 1
        st = F.closed_form(cs["t"], cs["c"], cs["W"], cs["d"], cs["z"], n0)
        mu, var = F.forecast(st, cs["c"], cs["t"][n0:], cs["a"][n0:], cs["U"][n0:])
        mu_o, var_o = F.dense_forecast(K, y, n0)
        floor = max(np.abs(mu_o).max(), np.abs(y).max())
        assert F.err(mu, mu_o, floor) <= 1.0, (name, F.err(mu, mu_o, floor))
        assert F.err(var, var_o) <= 1.0, (name, F.err(var, var_o))
        # the noise-free process at the same times: a = k(0) in place of k(0) + diag
        var_f = F.forecast(st, cs["c"], cs["t"][n0:], np.full(N - n0, cs["k0"]), cs["U"][n0:])[1]
        assert F.err(var_f, var_o - cs["diag"][n0:], cs["k0"]) <= 1.0, name


def test_empty_state_ignores_t_last():
    """n == 0: p := 0 whatever t_last holds -- a first time far below it must not turn 0 * exp(+big) into NaN."""
    cs = F.draw(11, 5, 4)
    st = F.empty(4)
    st[0] = 1e6
    s1, d, W, z, flag = F.append(st, cs["c"], cs["t"] - 1e4, cs["a"], cs["U"], cs["V"], cs["y"])
    d_o, W_o = F.factor(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
    assert flag == 0 and np.all(np.isfinite(s1)) and F.err(d, d_o) <= 1.0 and F.err(W, W_o) <= 1.0


def test_failure_leaves_the_state():
    cs = F.draw(12, 9, 4)
    s0, *_ = F.append(F.empty(4), cs["c"], *(cs[k][:4] for k in "taUVy"))
    a = cs["a"][4:].copy()
    a[2] = -1.0
    s1, d, W, z, flag = F.append(s0, cs["c"], cs["t"][4:], a, cs["U"][4:], cs["V"][4:], cs["y"][4:])
    assert flag == 3 and np.array_equal(s1, s0)
    assert np.all(np.isfinite(d[:3])) and d[2] <= 0 and np.all(np.isfinite(z[:2])) and np.all(np.isnan(z[2:]))


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib


def test_header_symbols_exported(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    for J, words in ((1, 6), (8, 76), (32, 1060), (0, 0), (33, 0), (-1, 0)):
        assert lib.load().c2_filter_state_words(J) == words, J
        if words:
            assert F.state_words(J) == words


def test_abi_argument_errors(lib):
    """The three device entry points reject non-positive sizes and null pointers (C2_ERR_INVALID) and widths above
    C2_FAST_WIDTH (C2_ERR_UNSUPPORTED) before anything touches the device.  `count` is nullable, and a count out of range
    is the caller's responsibility."""
    L = lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first
    INVALID, UNSUPPORTED = lib.C2_ERR_INVALID, lib.C2_ERR_UNSUPPORTED

    def append(B, M, J, p):   # p: state_in, state_out, t, c, a, U, V, y, d, W, z, flag
        return L.c2_filter_append(i64(B), i64(M), i64(J), p[0], p[1], p[2], i64(0), p[3], i64(0), p[4], p[5], p[6], p[7], null,
                                  p[8], p[9], p[10], p[11], null)

    def absorb(B, M, J, p):   # p: state_in, state_out, t, c, W, d, z
        return L.c2_filter_absorb(i64(B), i64(M), i64(J), p[0], p[1], p[2], i64(0), p[3], i64(0), p[4], p[5], p[6], null, null)

    def forecast(B, M, J, p):   # p: state, t, c, a, U, mu, var
        return L.c2_filter_forecast(i64(B), i64(M), i64(J), p[0], p[1], i64(0), p[2], i64(0), p[3], p[4], null, p[5], p[6], null)

    for call, nptr in ((append, 12), (absorb, 7), (forecast, 7)):
        full = [one] * nptr
        assert call(1, 4, 2, [null] * nptr) == INVALID
        for k in range(nptr):   # each pointer in turn
            assert call(1, 4, 2, full[:k] + [null] + full[k + 1:]) == INVALID, (call.__name__, k)
        assert call(0, 4, 2, full) == INVALID
        assert call(1, 0, 2, full) == INVALID
        assert call(1, 4, 0, full) == INVALID
        assert call(1, 4, 33, full) == UNSUPPORTED
        assert call(1, 4, 33, [null] * nptr) == UNSUPPORTED
        assert call(1, 2**31, 2, full) == UNSUPPORTED   # count is int32
