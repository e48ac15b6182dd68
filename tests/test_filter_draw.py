# -*- coding: utf-8 -*-
"""CPU checks of the forecast sample paths: the numpy restatement (tests/filter_draw_ref.py, what the GPU tests compare the
kernel with) against dense conditioning -- mu_c + cholesky(Sigma_c) @ eps -- and the header, the export lists and the argument
validation of include/celerite2_amd_filter_draw.h through the loaded library.

Criterion everywhere: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (inverse_diag_ref.err).  Every conditional
covariance has a condition number <= 1e6, asserted per case."""
import ctypes

import numpy as np
import pytest

import filter_draw_ref as D
import filter_ref as F

# (seed, N, J, gap in time, noise range in units of k(0))
DRAWS = [(21, 40, 1, False, (0.05, 0.5)), (22, 40, 2, True, (0.05, 0.5)), (23, 70, 3, False, (0.05, 0.5)),
         (24, 70, 5, True, (1e-3, 1e-2)), (25, 150, 8, False, (1e-3, 10.0)), (26, 97, 16, False, (0.05, 0.5)),
         (27, 97, 17, True, (0.05, 0.5)), (28, 150, 32, False, (0.05, 0.5))]
KDRAWS = 3


def _state(cs, n0):
    """The state behind row n0 - 1 (the empty one for n0 == 0)."""
    st = F.empty(cs["J"])
    if n0:
        st, *_, flag = F.append(st, cs["c"], *(cs[k][:n0] for k in "taUVy"))
        assert flag == 0
    return st


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed, N, J, gap, noise in DRAWS:
        cs = F.draw(seed, N, J, gap=gap, noise=noise)
        cs["N"], cs["J"] = N, J
        cs["eps"] = np.random.default_rng(seed).normal(size=(N, KDRAWS))
        out.append(("draw%d_N%d_J%d%s" % (seed, N, J, "_gap" if gap else ""), cs))
    return out


def test_draw_is_dense_conditioning(cases):
    """From the state behind row n0 - 1, the paths at the later rows are mu_c + cholesky(Sigma_c) @ eps, with noise (would-be
    observations) and latent (a = k(0) at the query rows), for n0 in {0, 1, N - 1, about N / 2}."""
    worst = 0.0
    for name, cs in cases:
        N, y = cs["N"], cs["y"]
        for n0 in (0, 1, N - 1, N // 2 + 1):
            st = _state(cs, n0)
            for latent in (False, True):
                a = cs["a"].copy()
                if latent:
                    a[n0:] = cs["k0"]
                K = F.dense(cs["t"], cs["c"], a, cs["U"], cs["V"])
                mu, Sig = D.dense_conditional(K, y, n0)
                cond = np.linalg.cond(Sig)
                assert cond <= 1e6, (name, n0, latent, cond)   # a bad draw fails here instead of loosening anything below
                eps = cs["eps"][n0:]
                ref = mu[:, None] + np.linalg.cholesky(Sig) @ eps
                paths, d, flag = D.draw_paths(st, cs["c"], cs["t"][n0:], a[n0:], cs["U"][n0:], cs["V"][n0:], eps)
                assert flag == 0, (name, n0, latent)
                e = F.err(paths, ref)
                worst = max(worst, e)
                assert e <= 1.0, (name, n0, latent, e)
                # d is the append's: neither depends on y
                d_o = F.append(st, cs["c"], cs["t"][n0:], a[n0:], cs["U"][n0:], cs["V"][n0:], y[n0:])[1]
                assert np.array_equal(d, d_o), (name, n0, latent)
    print("worst violation ratio %.2e" % worst)


def test_round_trip_of_an_append(cases):
    """eps = z / sqrt(d) of a real append gives its y back."""
    for name, cs in cases:
        n0 = cs["N"] // 2
        st = _state(cs, n0)
        rows = [cs[k][n0:] for k in "taUV"]
        _, d, _, z, flag = F.append(st, cs["c"], *rows, cs["y"][n0:])
        assert flag == 0
        paths, d2, flag = D.draw_paths(st, cs["c"], *rows, (z / np.sqrt(d))[:, None])
        assert flag == 0 and np.array_equal(d, d2)
        floor = np.abs(cs["y"]).max()
        assert F.err(paths[:, 0], cs["y"][n0:], floor) <= 1.0, (name, F.err(paths[:, 0], cs["y"][n0:], floor))


def test_zero_normals_give_the_forecast_mean(cases):
    """eps = 0: every row's path value is filter_ref.forecast's mean, and the first row's d is its variance."""
    for name, cs in cases:
        n0 = cs["N"] // 2
        st = _state(cs, n0)
        rows = [cs[k][n0:] for k in "taUV"]
        paths, d, flag = D.draw_paths(st, cs["c"], *rows, np.zeros((cs["N"] - n0, 2)))
        mu, var = F.forecast(st, cs["c"], rows[0], rows[1], rows[2])
        floor = max(np.abs(mu).max(), np.abs(cs["y"]).max())
        assert flag == 0 and F.err(paths[:, 0], mu, floor) <= 1.0 and np.array_equal(paths[:, 0], paths[:, 1]), name
        assert F.err(d[:1], var[:1]) <= 1.0, name


def test_empty_state_gives_a_prior_draw():
    """n == 0 under a stale t_last = 1e6: p := 0, and the paths are cholesky(K) @ eps."""
    cs = F.draw(31, 12, 4)
    st = F.empty(4)
    st[0] = 1e6
    eps = np.random.default_rng(31).normal(size=(12, 5))
    paths, d, flag = D.draw_paths(st, cs["c"], cs["t"] - 1e4, cs["a"], cs["U"], cs["V"], eps)
    K = F.dense(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
    assert np.linalg.cond(K) <= 1e6
    assert flag == 0 and F.err(paths, np.linalg.cholesky(K) @ eps) <= 1.0
    assert F.err(d, F.factor(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])[0]) <= 1.0


def test_failing_row():
    """flag, the rows before the failing one, its d, and nothing behind it."""
    cs = F.draw(32, 9, 4)
    st = _state(dict(cs, J=4), 4)
    a = cs["a"][4:].copy()
    a[2] = -1.0
    eps = np.random.default_rng(32).normal(size=(5, 3))
    paths, d, flag = D.draw_paths(st, cs["c"], cs["t"][4:], a, cs["U"][4:], cs["V"][4:], eps)
    good = D.draw_paths(st, cs["c"], cs["t"][4:], cs["a"][4:], cs["U"][4:], cs["V"][4:], eps)
    assert flag == 3 and d[2] <= 0 and np.all(np.isnan(d[3:])) and np.all(np.isnan(paths[2:]))
    assert np.array_equal(paths[:2], good[0][:2]) and np.array_equal(d[:2], good[1][:2])


def test_joint_log_density_is_the_dense_one(cases):
    """-(1/2) sum (z^2 / d + log d + log 2 pi) over the rows of an append from the state behind row n0 - 1 is the log density
    of the multivariate normal N(mu_c, Sigma_c) at those rows."""
    for name, cs in cases:
        N, y = cs["N"], cs["y"]
        K = F.dense(cs["t"], cs["c"], cs["a"], cs["U"], cs["V"])
        for n0 in (0, 1, N - 1, N // 2 + 1):
            _, d, _, z, flag = F.append(_state(cs, n0), cs["c"], *(cs[k][n0:] for k in "taUVy"))
            assert flag == 0
            mu, Sig = D.dense_conditional(K, y, n0)
            r = y[n0:] - mu
            ref = -0.5 * (r @ np.linalg.solve(Sig, r) + np.linalg.slogdet(Sig)[1] + (N - n0) * np.log(2 * np.pi))
            assert abs(D.joint_log_density(d, z) - ref) <= 1e-10 * abs(ref), (name, n0)


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib


def test_header_symbols_exported(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    for J in (0, 33, -1):
        assert lib.load().c2_filter_draw_chunk(J) == 0
    for J in range(1, 33):
        assert lib.load().c2_filter_draw_chunk(J) >= 1


def test_abi_argument_errors(lib):
    """c2_filter_draw rejects non-positive sizes and null pointers (C2_ERR_INVALID) and what it does not support
    (C2_ERR_UNSUPPORTED) before anything touches the device.  `count` is nullable."""
    L = lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first
    INVALID, UNSUPPORTED = lib.C2_ERR_INVALID, lib.C2_ERR_UNSUPPORTED

    def draw(B, M, J, K, p):   # p: state, t, c, a, U, V, eps, paths, d, flag
        return L.c2_filter_draw(i64(B), i64(M), i64(J), i64(K), p[0], p[1], i64(0), p[2], i64(0), p[3], p[4], p[5], p[6], null,
                                p[7], p[8], p[9], null)

    full = [one] * 10
    assert draw(1, 4, 2, 3, [null] * 10) == INVALID
    for k in range(10):   # each pointer in turn
        assert draw(1, 4, 2, 3, full[:k] + [null] + full[k + 1:]) == INVALID, k
    assert draw(0, 4, 2, 3, full) == INVALID
    assert draw(1, 0, 2, 3, full) == INVALID
    assert draw(1, 4, 0, 3, full) == INVALID
    assert draw(1, 4, 2, 0, full) == INVALID
    assert draw(1, 4, 33, 3, full) == UNSUPPORTED
    assert draw(1, 4, 33, 3, [null] * 10) == UNSUPPORTED
    assert draw(1, 2**31, 2, 3, full) == UNSUPPORTED   # count is int32
    assert draw(1, 4, 2, 2**31, full) == UNSUPPORTED
