# -*- coding: utf-8 -*-
"""The periodogram under correlated noise on the CPU: the numpy restatement of the whitened-sinusoid sweep
(tests/periodogram_ref.py, what csrc/c2_periodogram.hip implements) against dense algebra, the torch finish
(celerite2_amd/periodogram.py) on the restated products against dense generalized least squares per frequency, against the
classical floating-mean periodogram in the white-noise limit and on an injected signal, and the binding of the third public
header (include/celerite2_amd_periodogram.h), which needs no device.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import ctypes

import numpy as np
import pytest
import torch

import periodogram_ref as R

WIDTHS = [1, 2, 3, 5, 8, 16, 32]
LENGTHS = [1, 2, 17, 33, 150]
WORST = {}


def check(key, x, xo, what=None):
    """The standing criterion on the finite entries; the NaN positions of x and xo must be the same."""
    x, xo = np.asarray(x, dtype=float), np.asarray(xo, dtype=float)
    assert x.shape == xo.shape, (what, key, x.shape, xo.shape)
    assert np.array_equal(np.isnan(x), np.isnan(xo)), (what, key)
    m = ~np.isnan(xo)
    e = R.err(x[m], xo[m]) if m.any() and np.any(xo[m]) else (0.0 if not np.any(x[m]) else np.inf)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert e <= 1.0, (what, key, e)
    return e


def finish_of(D, T, normalization="standard", **kw):
    from celerite2_amd import periodogram as pg

    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    return pg.finish(S0, torch.from_numpy(np.asarray(T))[None], len(D["t"]), normalization, **kw)


@pytest.mark.parametrize("J", WIDTHS)
def test_restatement_against_dense(J):
    """T from the restated sweep, single-series and batched, against C^T K^-1 [C | S | Y0] from np.linalg.solve on the dense
    matrix, on every length; the nuisance columns rotate over P0 = 1, 0, 3, and t_ref is off zero on every other case."""
    for i, N in enumerate(LENGTHS):
        P0 = (1, 0, 3)[(i + J) % 3]
        D = R.case(100 * J + i, N, J, P0)
        t_ref = 0.0 if i % 2 else float(D["t"][N // 2]) + 0.125
        K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
        want = R.dense_products(K, D["t"], D["Y0"], D["freq"], t_ref)
        args = [D[x] for x in ("t", "c", "U", "W", "d", "Z0", "freq")]
        got = R.whitened_sinusoids(*args, t_ref)
        assert got.shape == (65, 5 + 2 * P0)
        check("restatement vs dense", got, want, (J, N, P0))
        gotb = R.whitened_sinusoids_batched(*[np.stack([a, a]) for a in args], t_ref)
        assert gotb.shape == (2, 65, 5 + 2 * P0) and np.array_equal(gotb[0], gotb[1])
        check("batched restatement vs dense", gotb[0], want, (J, N, P0))
        check("batched vs single restatement", gotb[0], got, (J, N, P0))


@pytest.mark.parametrize("N,J", [(150, 8), (33, 3), (17, 1), (150, 32)])
def test_finish_against_dense(N, J):
    """The torch finish on the restated products against two dense generalized-least-squares fits per frequency, 65
    frequencies and a constant column: dchi2 in all three normalisations, the amplitudes and chi2 of the null fit."""
    D = R.case(7 * N + J, N, J, 1)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, chi2_0 = R.dense_periodogram(K, D["t"], D["A0"], D["y"], D["freq"])
    T = R.whitened_sinusoids(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0", "freq")])
    for nm, want in (("standard", dchi2 / chi2_0), ("chi2", dchi2), ("log_likelihood", 0.5 * dchi2)):
        fit = finish_of(D, T, nm)
        assert tuple(fit.power.shape) == (1, 65) and tuple(fit.amplitude.shape) == (1, 65, 2) and tuple(fit.chi2_null.shape) == (1,)
        check("finish power vs dense", fit.power[0].numpy(), want, (N, J, nm))
        check("finish amplitude vs dense", fit.amplitude[0].numpy(), amp, (N, J, nm))
        check("finish chi2_null vs dense", fit.chi2_null.numpy(), [chi2_0], (N, J, nm))
    p = finish_of(D, T).power[0].numpy()
    assert np.all(p >= 0.0) and np.all(p <= 1.0)


@pytest.mark.parametrize("P0", [0, 3])
def test_finish_other_column_counts(P0):
    """No nuisance column (the G00 terms vanish) and three of them, against the dense fits."""
    D = R.case(40 + P0, 60, 4, P0)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, chi2_0 = R.dense_periodogram(K, D["t"], D["A0"], D["y"], D["freq"])
    fit = finish_of(D, R.whitened_sinusoids(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0", "freq")]), "chi2")
    check("finish power vs dense", fit.power[0].numpy(), dchi2, P0)
    check("finish amplitude vs dense", fit.amplitude[0].numpy(), amp, P0)
    check("finish chi2_null vs dense", fit.chi2_null.numpy(), [chi2_0], P0)


@pytest.mark.parametrize("N", [1, 2])
def test_rank_deficient_lengths(N):
    """One and two points beside a constant column: the raw products are what dense algebra gives, the power and the
    amplitudes are NaN at every frequency, chi2 of the null fit stays, and nothing raises."""
    D = R.case(11 + N, N, 3, 1, F=7)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    T = R.whitened_sinusoids(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0", "freq")])
    check("restatement vs dense", T, R.dense_products(K, D["t"], D["Y0"], D["freq"]), N)
    for nm in ("standard", "chi2", "log_likelihood"):
        fit = finish_of(D, T, nm)
        assert bool(torch.isnan(fit.power).all()) and bool(torch.isnan(fit.amplitude).all())
        assert bool(torch.isfinite(fit.chi2_null).all())


def test_nan_rules():
    """w = 0 beside a constant column is NaN and leaves the other frequencies alone; a repeated nuisance column or a series
    that is not `ok` is NaN throughout and leaves its neighbours their bits."""
    from celerite2_amd import periodogram as pg

    D = R.case(5, 33, 3, 2)
    freq = np.concatenate([[0.0], D["freq"][:6]])
    args = [D[x] for x in ("t", "c", "U", "W", "d")]
    T = R.whitened_sinusoids(*args, D["Z0"], freq)
    fit = finish_of(D, T)
    assert bool(torch.isnan(fit.power[0, 0])) and bool(torch.isnan(fit.amplitude[0, 0]).all())
    assert bool(torch.isfinite(fit.power[0, 1:]).all()) and bool(torch.isfinite(fit.amplitude[0, 1:]).all())
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    check("finish power vs dense", fit.power[0, 1:].numpy(), np.divide(*R.dense_periodogram(K, D["t"], D["A0"], D["y"], freq[1:])[::2]))
    Y2 = D["Y0"].copy()
    Y2[:, 1] = Y2[:, 0]                      # rank 1
    Z2 = R.sweep(D["t"], D["c"], D["U"], D["W"], Y2)[0]
    T2 = R.whitened_sinusoids(*args, Z2, freq)
    S0 = torch.from_numpy(np.stack([R.null_products(Z, D["d"]) for Z in (D["Z0"], Z2, D["Z0"])]))
    TT = torch.from_numpy(np.stack([T, T2, T]))
    got = pg.finish(S0, TT, 33, ok=torch.tensor([True, True, False]))
    for b in (1, 2):
        assert bool(torch.isnan(got.power[b]).all()) and bool(torch.isnan(got.amplitude[b]).all()) and bool(torch.isnan(got.chi2_null[b]))
    for x, xo in zip(got, fit):
        assert np.array_equal(x[0].numpy(), xo[0].numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="normalization"):
        pg.finish(S0, TT, 33, "psd")
    with pytest.raises(ValueError, match=r"^Invalid shape: T "):
        pg.finish(S0, TT[..., :-1], 33)


def test_white_noise_limit():
    """U = V = 0 (so W = 0 and d = the diagonal): the "standard" power is the classical floating-mean periodogram, written
    from weighted sums -- the one known answer that shares no code with the sweep."""
    rng = np.random.default_rng(3)
    N, J = 80, 2
    t = np.sort(rng.uniform(0.0, 20.0, N))
    sigma2 = rng.uniform(0.05, 0.5, N)
    y = 0.7 + 0.4 * np.sin(2.1 * t + 0.3) + np.sqrt(sigma2) * rng.normal(size=N)
    freq = R.grid(t)
    D = dict(t=t, d=sigma2, Z0=np.stack([np.ones(N), y], axis=1))
    for t_ref in (0.0, 7.5):
        T = R.whitened_sinusoids(t, np.array([0.3, 1.1]), np.zeros((N, J)), np.zeros((N, J)), sigma2, D["Z0"], freq, t_ref)
        check("white-noise limit vs classical", finish_of(D, T).power[0].numpy(), R.classical_gls(t, y, sigma2, freq, t_ref), t_ref)


def test_injected_signal():
    """A sinusoid at a grid frequency added to a draw: the power peaks there, and the fitted (alpha, beta) are dense GLS's."""
    D = R.case(21, 150, 4, 1)
    k = 23
    y = D["y"] + 3.0 * np.cos(D["freq"][k] * D["t"] - 0.8)
    Y0 = np.concatenate([D["A0"], y[:, None]], axis=1)
    D["Z0"] = R.sweep(D["t"], D["c"], D["U"], D["W"], Y0)[0]
    fit = finish_of(D, R.whitened_sinusoids(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0", "freq")]))
    assert int(torch.argmax(fit.power[0])) == k
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, chi2_0 = R.dense_periodogram(K, D["t"], D["A0"], y, D["freq"])
    check("finish power vs dense", fit.power[0].numpy(), dchi2 / chi2_0, "injected")
    check("finish amplitude vs dense", fit.amplitude[0].numpy(), amp, "injected")
    assert abs(np.hypot(*fit.amplitude[0, k].numpy()) - 3.0) < 1.0      # (the injected amplitude, to the noise)


# ---- the binding of the third header -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def sin_args(B=1, N=4, J=2, Q0=1, F=3, p=None, T=None, t_ref=0.0):
    return [B, N, J, Q0, F, p, 0, p, 0, p, p, p, p, p, 0, t_ref, T, None]


def test_periodogram_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib

    fn = lib.c2_whitened_sinusoids
    assert len(fn.argtypes) == 18 and fn.restype is ctypes.c_int
    assert fn.argtypes[:5] == (ctypes.c_int64,) * 5 and fn.argtypes[5] is _lib.Pointer and fn.argtypes[14] is ctypes.c_int64
    assert fn.argtypes[15] is ctypes.c_double and fn.argtypes[16] is _lib.Pointer


def test_bad_sinusoid_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_whitened_sinusoids(*sin_args()[:-1])
    with pytest.raises(refused):
        lib.c2_whitened_sinusoids(*sin_args(), None)
    with pytest.raises(refused):
        lib.c2_whitened_sinusoids(*sin_args(B=1.0))
    with pytest.raises(refused):
        lib.c2_whitened_sinusoids(*sin_args(t_ref="0"))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_whitened_sinusoids(*sin_args(p=text))


def test_sinusoid_argument_errors(lib):
    """Sizes, null pointers, J = 33 and Q0 = 9 are refused before anything is launched: no device is needed."""
    from celerite2_amd import _lib

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    for bad in (dict(B=0), dict(N=0), dict(J=0), dict(Q0=0), dict(F=0), dict(N=-1), dict(F=-3)):
        assert lib.c2_whitened_sinusoids(*sin_args(p=p, T=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_whitened_sinusoids(*sin_args(p=p, T=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_sinusoids(*sin_args(p=None, T=p)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_sinusoids(*sin_args(J=33, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_sinusoids(*sin_args(Q0=9, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    # 2^31 blocks or more: 64 frequencies a block up to J = 16, 32 at J = 32
    assert lib.c2_whitened_sinusoids(*sin_args(B=2 ** 31, F=64, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_sinusoids(*sin_args(B=2 ** 25, F=64 * 64, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_sinusoids(*sin_args(B=2 ** 25, F=64 * 32, J=32, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED


def test_ops_shape_errors_name_the_argument():
    """ops.whitened_sinusoids describes its arguments with the shared specs (CPU tensors: the dtype / device check comes first,
    so the helper is called directly)."""
    from celerite2_amd import ops

    dims = dict(B=2, N=5, J=2, Q=3, F=4, K=9)
    ops._shapes(dims, [("Z0", torch.zeros(2, 5, 3), "BNQ"), ("freq", torch.zeros(4), "F|BF"), ("freq", torch.zeros(2, 4), "F|BF"),
                       ("out", torch.zeros(2, 4, 9), "BFK")])
    with pytest.raises(ValueError, match=r"^Invalid shape: Z0 "):
        ops._shapes(dims, [("Z0", torch.zeros(5, 3), "BNQ")])
    with pytest.raises(ValueError, match=r"^Invalid shape: freq "):
        ops._shapes(dims, [("freq", torch.zeros(3, 4), "F|BF")])
    with pytest.raises(ValueError, match=r"^Invalid shape: out "):
        ops._shapes(dims, [("out", torch.zeros(2, 4, 7), "BFK")])
    with pytest.raises(ValueError, match="GPU"):
        ops.whitened_sinusoids(torch.zeros(5), torch.zeros(2), torch.zeros(2, 5, 2), torch.zeros(2, 5, 2), torch.zeros(2, 5),
                               torch.zeros(2, 5, 3), torch.zeros(4))


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
