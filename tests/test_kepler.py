# -*- coding: utf-8 -*-
"""The Keplerian search under correlated noise on the CPU: the solver of Kepler's equation as the kernel states it
(tests/kepler_ref.py, what csrc/c2_kepler.hip implements) against a bracketed extended-precision solution, the exact
reduction of the mean anomaly against math.remainder, the numpy restatement of the whitened-Keplerian sweep against dense
algebra, the torch finish (celerite2_amd/kepler.py) on the restated products against two dense generalized-least-squares
fits per trial and on an injected orbit, the grid, the domain and the profile, and the binding of the fifth public header
(include/celerite2_amd_kepler.h), which needs no device.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import kepler_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
ECCS = [0.0, 1e-12, 1e-8, 0.3, 0.7, 0.9, 0.95, 0.99]
SWEEP_ARGS = ("t", "c", "U", "W", "d", "Z0", "trials")
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


def anomaly_grid():
    """r on 20 001 points of [-pi (1 + 1e-7), pi (1 + 1e-7)] and the special values."""
    top = np.pi * (1.0 + 1e-7)
    special = [0.0, 1e-300, -1e-300, 1e-12, -1e-12, 1e-6, -1e-6, 1e-3, -1e-3, np.pi, -np.pi]
    return np.concatenate([np.linspace(-top, top, 20001), special])


# ---- the solver ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", ECCS)
def test_solver_against_bracketed_solution(e):
    """The lane's fixed sequence against bisection in extended precision.  |E - E*| (1 - e cos E*) <= 16 ulp: the residual
    E - e sin E - r cannot be evaluated in double to better than about 1.5 ulp (|E| + |r| + e), and a converged double
    solver measures 3.2 on this grid.  The columns lie within 32 ulp sqrt(1 - e^2) / (1 - e cos E*)^2 + 8 ulp of the converged
    ones (d nu / d M times the bound on M, plus the rounding of the column's own arithmetic)."""
    r = anomaly_grid()
    E, cnu, snu = R.solve(r, e)
    Ec = R.converged(r, e)
    Co, So = R.columns_converged(r, e)
    w = (1.0 - np.longdouble(e) * np.cos(Ec))
    worst = float(np.max(np.abs(E - Ec) * w)) / ULP
    WORST["solver |E - E*| (1 - e cos E*) / ulp, e = %g" % e] = worst
    assert worst <= 16.0, (e, worst)
    bound = 32.0 * ULP * math.sqrt(1.0 - e * e) / w ** 2 + 8.0 * ULP
    for name, got, want in (("cos nu", cnu, Co), ("sin nu", snu, So)):
        ratio = float(np.max(np.abs(got - want) / bound))
        WORST["solver %s error / bound, e = %g" % (name, e)] = ratio
        assert ratio <= 1.0, (e, name, ratio)
    assert np.all(np.abs(cnu) <= 1.0 + 4 * ULP) and np.all(np.abs(snu) <= 1.0 + 4 * ULP)


@pytest.mark.parametrize("e", ECCS)
def test_columns_are_even_and_odd(e):
    """cos nu is exactly even in r and sin nu exactly odd: the equation is solved for |r| and the sign restored."""
    r = anomaly_grid()
    _, c1, s1 = R.solve(r, e)
    _, c2, s2 = R.solve(-r, e)
    assert np.array_equal(c1, c2) and np.array_equal(s1, -s2)


def test_circular_limit():
    """At e = 0 the columns are cos r and sin r to 2 ulp, and E = r."""
    r = anomaly_grid()
    E, cnu, snu = R.solve(r, 0.0)
    assert np.array_equal(E, r)
    assert np.max(np.abs(cnu - np.cos(r))) <= 2 * ULP and np.max(np.abs(snu - np.sin(r))) <= 2 * ULP


# ---- the reduction ---------------------------------------------------------------------------------------------------------
def test_reduce_is_the_exact_remainder():
    """r = fma(-q, TWO_PI, x) through exact rationals: it is representable (the fma rounds nothing away), it is
    math.remainder(x, TWO_PI) except on ties at +-pi, |r| <= pi (1 + 2^-50), for |x| up to 1e7; and the array form used by
    the restated sweep gives the same bits.
    The bound pi (1 + 2^-50) is asserted on the drawn values and on whole turns.  It does NOT hold on values constructed
    next to a half turn of a large q (measured: x = 3494038.508618071, q = 556094, |r| = pi + 2.7e-11): fl(x * INV_2PI)
    carries a relative error of up to 2^-52 (INV_2PI's and the product's), so q may fall on the other side of the half
    turn and |r| <= pi (1 + (|q| + 1) 2^-51).  Those values are held to that bound, which is what the header states."""
    from fractions import Fraction

    rng = np.random.default_rng(0)
    drawn = np.concatenate([rng.uniform(-1e7, 1e7, 6000), rng.uniform(-100.0, 100.0, 3000), rng.uniform(-4.0, 4.0, 1000),
                            np.rint(rng.uniform(-1e6, 1e6, 1500)) * R.TWO_PI,                # whole turns
                            [0.0, -0.0, np.pi, -np.pi, 1e7, -1e7, 1e-300, R.TWO_PI, 0.5 * R.TWO_PI, 1.5 * R.TWO_PI]])
    halves = (np.rint(rng.uniform(-1e6, 1e6, 1500)) + 0.5) * R.TWO_PI                        # half turns: next to the ties
    x = np.concatenate([drawn, halves])
    got = np.array([R.reduce(v) for v in x])
    for i, (v, r) in enumerate(zip(x, got)):
        q = float(np.rint(v * R.INV_2PI))
        assert Fraction(r) == Fraction(float(v)) - Fraction(q) * Fraction(R.TWO_PI), v       # exactly representable
        top = math.pi * (1.0 + 2.0 ** -50) if i < len(drawn) else math.pi * (1.0 + (abs(q) + 1.0) * 2.0 ** -51)
        assert abs(r) <= top, (v, r)
        m = math.remainder(float(v), R.TWO_PI)
        if r != m:                                                                            # only the other side of a tie
            assert i >= len(drawn) - 10, (v, r, m)                                            # (never on a drawn value)
            assert abs(abs(r) - 0.5 * R.TWO_PI) <= 4e-9 and abs(Fraction(r) - Fraction(m)) == Fraction(R.TWO_PI), (v, r, m)
    assert np.array_equal(R.reduce_array(x), got)
    assert np.array_equal(np.signbit(R.reduce_array(x)[got != 0]), np.signbit(got[got != 0]))


# ---- the sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 3, 8])
def test_restatement_against_dense(J):
    """T from the restated sweep, single-series and batched, against [C | S]^T K^-1 [C | S | Y0] from np.linalg.solve on
    the dense matrix with the columns built the independent way (extended-precision reduction, bisection)."""
    for i, N in enumerate((1, 2, 9, 33)):
        for Q0 in (1, 3):
            D = R.case(100 * J + 10 * i + Q0, N, J, Q0 - 1, K=33, e_max=0.9)
            K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
            want = R.dense_products(K, D["t"], D["Y0"], D["trials"])
            args = [D[x] for x in SWEEP_ARGS]
            got = R.whitened_keplerians(*args)
            assert got.shape == (33, 3 + 2 * Q0)
            check("restatement vs dense", got, want, (J, N, Q0))
            gotb = R.whitened_keplerians_batched(*[np.stack([a, a]) for a in args])
            assert gotb.shape == (2, 33, 3 + 2 * Q0) and np.array_equal(gotb[0], gotb[1])
            check("batched vs single restatement", gotb[0], got, (J, N, Q0))


# ---- the finish ------------------------------------------------------------------------------------------------------------
def finish_of(D, T, **kw):
    from celerite2_amd import kepler as kp

    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    return kp.finish(S0, torch.from_numpy(np.asarray(T))[None], len(D["t"]), trials=torch.from_numpy(D["trials"]), **kw)


@pytest.mark.parametrize("P0", [0, 1, 3])
def test_finish_against_dense(P0):
    """The torch finish on the restated products against two dense generalized-least-squares fits per trial ([A0] and
    [A0 | cos nu | sin nu]): the power in all three normalisations, the amplitude and chi2 of the null fit."""
    from celerite2_amd import kepler as kp

    D = R.case(40 + P0, 120, 4, P0, K=40, e_max=0.9)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, chi2_0 = R.dense_keplerian(K, D["t"], D["A0"], D["y"], D["trials"])
    T = R.whitened_keplerians(*[D[x] for x in SWEEP_ARGS])
    for nm, ref in (("standard", dchi2 / chi2_0), ("chi2", dchi2), ("log_likelihood", 0.5 * dchi2)):
        fit = finish_of(D, T, normalization=nm)
        assert isinstance(fit, kp.KeplerianSearch) and fit._fields == ("power", "amplitude", "semi_amplitude", "omega", "chi2_null")
        assert tuple(fit.power.shape) == (1, 40) and tuple(fit.amplitude.shape) == (1, 40, 2) and tuple(fit.chi2_null.shape) == (1,)
        check("finish power vs dense", fit.power[0].numpy(), ref, (P0, nm))
        check("finish amplitude vs dense", fit.amplitude[0].numpy(), amp, (P0, nm))
        check("finish semi_amplitude vs dense", fit.semi_amplitude[0].numpy(), np.hypot(amp[:, 0], amp[:, 1]), (P0, nm))
        check("finish omega vs dense", fit.omega[0].numpy(), np.arctan2(-amp[:, 1], amp[:, 0]), (P0, nm))
        check("finish chi2_null vs dense", fit.chi2_null.numpy(), [chi2_0], (P0, nm))


@pytest.mark.parametrize("P0", [1, 3])
def test_injected_orbit_is_recovered(P0):
    """Noise-free y = A0 beta0 + K cos(nu + omega) at each trial in turn: the fit at that trial returns (K, omega) to the
    criterion (the constant K e cos omega it leaves out lies in the span of A0's constant column)."""
    D = R.case(60 + P0, 120, 4, P0, K=40, e_max=0.9)
    C, S = R.columns(D["t"], D["trials"])
    rng = np.random.default_rng(1)
    beta0 = rng.normal(size=P0)
    for k in (0, 7, 22, 39):
        semi, omega = rng.uniform(0.5, 3.0), rng.uniform(-3.0, 3.0)
        y = D["A0"] @ beta0 + semi * (np.cos(omega) * C[:, k] - np.sin(omega) * S[:, k])
        Y0 = np.concatenate([D["A0"], y[:, None]], axis=1)
        E = dict(D, Z0=R.sweep(D["t"], D["c"], D["U"], D["W"], Y0)[0])
        fit = finish_of(E, R.whitened_keplerians(*[E[x] for x in SWEEP_ARGS]), normalization="chi2")
        check("injected semi-amplitude", [float(fit.semi_amplitude[0, k])], [semi], (P0, k))
        check("injected omega", [float(fit.omega[0, k])], [omega], (P0, k))
        assert int(torch.argmax(fit.power[0])) == k


def test_finish_masks_the_domain_and_names_bad_shapes():
    from celerite2_amd import kepler as kp

    D = R.case(5, 33, 3, 2, K=20, e_max=0.9)
    args = [D[x] for x in SWEEP_ARGS[:-1]]
    good = finish_of(D, R.whitened_keplerians(*args, D["trials"]))
    assert all(bool(torch.isfinite(x).all()) for x in good)
    for name, (col, value) in {"e < 0": (1, -0.1), "e > 0.99": (1, 0.995), "w = 0": (0, 0.0), "w < 0": (0, -1.0),
                               "tp = inf": (2, np.inf)}.items():
        E = dict(D, trials=D["trials"].copy())
        E["trials"][7, col] = value
        with np.errstate(all="ignore"):
            T = R.whitened_keplerians(*args, E["trials"])
        keep = np.arange(20) != 7
        got = finish_of(E, T)
        for x, xo in zip(got[:4], good[:4]):
            assert bool(torch.isnan(x[0, 7]).all()), name
            assert np.array_equal(x[0].numpy()[keep], xo[0].numpy()[keep]), name
        assert torch.equal(got.chi2_null, good.chi2_null)
    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    T = torch.zeros((1, 20, 9), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"^Invalid shape: T "):
        kp.finish(S0, T[..., :-1], 33)
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        kp.finish(S0, T, 33, trials=torch.from_numpy(D["trials"][:-1]))
    with pytest.raises(ValueError, match="normalization"):
        kp.finish(S0, T, 33, normalization="psd")


# ---- the smaller pieces ----------------------------------------------------------------------------------------------------
def test_trial_grid():
    from celerite2_amd import kepler as kp

    freq, ecc = [0.5, 2.0, 3.0], [0.0, 0.4]
    g = kp.trial_grid(freq, ecc, 4, t0=10.0)
    assert g.dtype == torch.float64 and tuple(g.shape) == (3 * 2 * 4, 3)
    assert bool(kp.in_domain(g).all())
    k = 0
    for w in freq:                                         # frequency-major, then eccentricity, then periastron
        for e in ecc:
            for m in range(4):
                assert float(g[k, 0]) == w and float(g[k, 1]) == e
                assert float(g[k, 2]) == 10.0 + m * ((2.0 * math.pi / w) / 4), (k, m)
                k += 1
    assert torch.equal(kp.trial_grid(torch.tensor(freq, dtype=torch.float64), torch.tensor(ecc, dtype=torch.float64), 4, t0=10.0), g)
    assert tuple(kp.trial_grid([1.0], [0.1], 1).shape) == (1, 3)
    with pytest.raises(ValueError):
        kp.trial_grid([1.0], [0.1], 0)


def test_in_domain():
    from celerite2_amd import kepler as kp

    assert kp.MAX_ECC == 0.99
    header = open(os.path.join(ROOT, "include", "celerite2_amd_kepler.h")).read()
    assert float(re.search(r"#define\s+C2_KEPLER_MAX_ECC\s+(\S+)", header).group(1)) == kp.MAX_ECC == R.MAX_ECC
    nan, inf = float("nan"), float("inf")
    trials = torch.tensor([[1.0, 0.0, 0.0], [1.0, 0.99, 5.0], [1.0, float(np.nextafter(0.99, 1.0)), 0.0], [1.0, -0.0, 0.0],
                           [0.0, 0.1, 0.0], [-1.0, 0.1, 0.0], [1.0, -1e-300, 0.0], [nan, 0.1, 0.0], [1.0, nan, 0.0],
                           [1.0, 0.1, nan], [1.0, 0.1, inf], [1e-300, 0.5, -2.45e6], [inf, 0.5, 0.0]], dtype=torch.float64)
    want = [True, True, False, True, False, False, False, False, False, False, False, True, True]
    assert kp.in_domain(trials).tolist() == want
    assert kp.in_domain(torch.stack([trials, trials])).tolist() == [want, want]


def test_profile():
    from celerite2_amd import kepler as kp

    nan = float("nan")
    power = torch.tensor([[0.1, 0.3, nan, 0.2, nan, nan, 0.5, 0.5, nan, 0.0, nan, nan],
                          [nan, nan, nan, nan, nan, 0.7, 0.2, 0.1, 0.9, 0.4, 0.3, 0.2]], dtype=torch.float64)
    best, idx = kp.profile(power, 4)
    assert tuple(best.shape) == (2, 4) and tuple(idx.shape) == (2, 4)
    assert np.array_equal(best.numpy(), [[0.3, 0.2, 0.5, 0.0], [nan, 0.7, 0.9, 0.4]], equal_nan=True)
    assert idx[0].tolist()[:2] == [1, 3] and idx[0, 2].item() in (6, 7) and idx[0, 3].item() == 9
    assert idx[1].tolist() == [0, 5, 8, 9]
    fit = kp.KeplerianSearch(power, None, None, None, None)
    assert all(torch.equal(x, y) or bool(torch.isnan(x).any()) for x, y in zip(kp.profile(fit, 4), (best, idx)))
    assert torch.equal(kp.profile(fit, 4)[1], idx)
    one, at = kp.profile(power, 1)
    assert one[:, 0].tolist() == [0.5, 0.9] and at[1, 0].item() == 8
    with pytest.raises(ValueError, match=r"^Invalid shape: power "):
        kp.profile(power, 5)


# ---- the binding of the fifth header -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def kp_args(B=1, N=4, J=2, Q0=1, K=3, p=None, T=None):
    return [B, N, J, Q0, K, p, 0, p, 0, p, p, p, p, p, 0, T, None]


def test_kepler_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib

    fn = lib.c2_whitened_keplerians
    assert len(fn.argtypes) == 17 and fn.restype is ctypes.c_int
    assert fn.argtypes[:5] == (ctypes.c_int64,) * 5 and fn.argtypes[5] is _lib.Pointer and fn.argtypes[6] is ctypes.c_int64
    assert fn.argtypes[13] is _lib.Pointer and fn.argtypes[14] is ctypes.c_int64 and fn.argtypes[15] is _lib.Pointer
    # the constants of the header's rule are the ones the restatement uses
    text = open(_lib.header_path("kepler")).read()
    assert float.fromhex(re.search(r"TWO_PI = fl\(2 pi\) = (\S+);", text).group(1)) == R.TWO_PI
    assert float.fromhex(re.search(r"INV_2PI = fl\(1 / fl\(2 pi\)\) = (\S+);", text).group(1)) == R.INV_2PI


def test_bad_kepler_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_whitened_keplerians(*kp_args()[:-1])
    with pytest.raises(refused):
        lib.c2_whitened_keplerians(*kp_args(), None)
    with pytest.raises(refused):
        lib.c2_whitened_keplerians(*kp_args(B=1.0))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_whitened_keplerians(*kp_args(p=text))


def test_kepler_argument_errors(lib):
    """Sizes, null pointers, J = 33 and Q0 = 9 are refused before anything is launched: no device is needed."""
    from celerite2_amd import _lib

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    for bad in (dict(B=0), dict(N=0), dict(J=0), dict(Q0=0), dict(K=0), dict(N=-1), dict(K=-3)):
        assert lib.c2_whitened_keplerians(*kp_args(p=p, T=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_whitened_keplerians(*kp_args(p=p, T=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_keplerians(*kp_args(p=None, T=p)) == _lib.C2_ERR_INVALID
    neg = kp_args(p=p, T=p)
    neg[14] = -3
    assert lib.c2_whitened_keplerians(*neg) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_keplerians(*kp_args(J=33, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_keplerians(*kp_args(Q0=9, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    # 2^31 blocks or more: 64 trials a block up to J = 16, 32 above
    assert lib.c2_whitened_keplerians(*kp_args(B=2 ** 31, K=64, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_keplerians(*kp_args(B=2 ** 25, K=64 * 64, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_keplerians(*kp_args(B=2 ** 25, K=32 * 64, J=32, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED


def test_python_argument_errors():
    """ops.whitened_keplerians and gp.keplerian_search raise ValueError before C is entered (CPU tensors: the dtype / device
    check of the op comes first, so its shape specs are exercised through the helper)."""
    from celerite2_amd import gp as G, ops

    dims = dict(B=2, N=5, J=2, Q=3, K=6, F=3, R=9)
    ops._shapes(dims, [("Z0", torch.zeros(2, 5, 3), "BNQ"), ("trials", torch.zeros(6, 3), "KF|BKF"),
                       ("trials", torch.zeros(2, 6, 3), "KF|BKF"), ("out", torch.zeros(2, 6, 9), "BKR")])
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops._shapes(dims, [("trials", torch.zeros(3, 6, 3), "KF|BKF")])
    with pytest.raises(ValueError, match=r"^Invalid shape: out "):
        ops._shapes(dims, [("out", torch.zeros(2, 6, 8), "BKR")])
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    ins = [z(5), z(2), z(2, 5, 2), z(2, 5, 2), z(2, 5), z(2, 5, 3)]
    with pytest.raises(ValueError, match="GPU"):
        ops.whitened_keplerians(*ins, z(6, 3))
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops.whitened_keplerians(*ins, z(6, 4))
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops.whitened_keplerians(*ins, z(18))
    with pytest.raises(ValueError, match=r"^Invalid shape: Z0 "):
        ops.whitened_keplerians(*ins[:5], z(5, 3), z(6, 3))
    # the front end on a stand-in for a computed GP: trials, A and the normalisation are refused before anything is solved
    import types
    gp = types.SimpleNamespace(_need=lambda: None, _check_vector=lambda y: None, _diag=z(2, 5), mean=0.0, _t=z(5))
    gp._whitened_columns = lambda y, A: G.GaussianProcess._whitened_columns(gp, y, A)
    gp.keplerian_search = lambda *a, **k: G.GaussianProcess.keplerian_search(gp, *a, **k)
    for bad in (z(6, 4), z(3, 6, 3), z(18), z(0, 3), [[1.0, 0.0, 0.1]]):
        with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
            G.GaussianProcess.keplerian_search(gp, z(2, 5), bad)
    with pytest.raises(ValueError, match="A must be"):
        G.GaussianProcess.keplerian_search(gp, z(2, 5), z(6, 3), A="ones")
    with pytest.raises(ValueError, match=r"^Invalid shape: A "):
        G.GaussianProcess.keplerian_search(gp, z(2, 5), z(6, 3), A=z(4, 2))
    with pytest.raises(ValueError, match="normalization"):
        G.GaussianProcess.keplerian_search(gp, z(2, 5), z(6, 3), normalization="psd")
    with pytest.raises(ValueError, match="max_trials"):
        G.GaussianProcess.keplerian_periodogram(gp, z(2, 5), [1.0, 2.0], [0.0, 0.5], 4, max_trials=7)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst, %s: %.3g" % (k, WORST[k]))
