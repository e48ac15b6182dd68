# -*- coding: utf-8 -*-
"""The multi-harmonic periodogram under correlated noise on the CPU: the numpy restatement of the whitened-harmonics sweep
(tests/harmonics_ref.py, what csrc/c2_harmonics.hip implements) against dense algebra, the torch finish
(celerite2_amd/harmonics.py) on the restated products against dense generalized least squares per frequency, the nesting of
the models, an injected two-harmonic signal, the NaN rules, and the binding of the eighth public header
(include/celerite2_amd_harmonics.h), which needs no device.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import ctypes
import re

import numpy as np
import pytest
import torch

import harmonics_ref as R
import periodogram_ref as PR

WIDTHS = [1, 2, 3, 5, 8, 16, 32]
LENGTHS = [1, 2, 17, 33, 150]
TERMS = [1, 2, 3, 4]
SWEEP = ("t", "c", "U", "W", "d", "Z0", "freq")
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


def finish_of(D, T, H, normalization="standard", **kw):
    from celerite2_amd import harmonics as hm

    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    return hm.finish(S0, torch.from_numpy(np.asarray(T))[None], len(D["t"]), H, normalization, **kw)


@pytest.mark.parametrize("J", WIDTHS)
@pytest.mark.parametrize("H", TERMS)
def test_restatement_against_dense(H, J):
    """T from the restated sweep, single-series and batched, against the products from np.linalg.solve on the dense matrix,
    on every length; the nuisance columns rotate over P0 = 1, 0, 3, and t_ref is off zero on every other case.  At H = 1
    the restatement is periodogram_ref's, to the bit."""
    for i, N in enumerate(LENGTHS):
        P0 = (1, 0, 3)[(i + J) % 3]
        D = R.case(100 * J + i, N, J, P0, F=9)
        t_ref = 0.0 if i % 2 else float(D["t"][N // 2]) + 0.125
        K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
        want = R.dense_products(K, D["t"], D["Y0"], D["freq"], H, t_ref)
        args = [D[x] for x in SWEEP]
        got = R.whitened_harmonics(*args, H, t_ref)
        assert got.shape == (9, R.width(H, P0 + 1))
        check("restatement vs dense", got, want, (H, J, N, P0))
        gotb = R.whitened_harmonics_batched(*[np.stack([a, a]) for a in args], H, t_ref)
        assert gotb.shape == (2, 9, R.width(H, P0 + 1)) and np.array_equal(gotb[0], gotb[1])
        check("batched restatement vs dense", gotb[0], want, (H, J, N, P0))
        check("batched vs single restatement", gotb[0], got, (H, J, N, P0))
        if H == 1:
            assert np.array_equal(got, PR.whitened_sinusoids(*args, t_ref))


# (N, J, P0, lowest and highest frequency in cycles over the baseline)
FINISH_CASES = [(120, 3, 3, 1, 25), (120, 8, 1, 1, 12), (150, 32, 3, 1, 25), (33, 8, 2, 1, 6), (33, 2, 1, 1, 4), (17, 4, 1, 1, 2)]


@pytest.mark.parametrize("N,J,P0,lo,hi", FINISH_CASES)
@pytest.mark.parametrize("H", [2, 3, 4])
def test_finish_against_dense(H, N, J, P0, lo, hi):
    """The torch finish on the restated products against two dense generalized-least-squares fits per frequency, 40
    frequencies: dchi2 in all three normalisations, the amplitudes and chi2 of the null fit."""
    D = R.case(7 * N + J, N, J, P0)
    D["freq"] = R.grid(D["t"], 40, lo, hi)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, chi2_0 = R.dense_harmonics(K, D["t"], D["A0"], D["y"], D["freq"], H)
    T = R.whitened_harmonics(*[D[x] for x in SWEEP], H)
    for nm, want in (("standard", dchi2 / chi2_0), ("chi2", dchi2), ("log_likelihood", 0.5 * dchi2)):
        fit = finish_of(D, T, H, nm)
        assert tuple(fit.power.shape) == (1, 40) and tuple(fit.amplitude.shape) == (1, 40, 2 * H) and tuple(fit.chi2_null.shape) == (1,)
        check("finish power vs dense", fit.power[0].numpy(), want, (H, N, J, nm))
        check("finish amplitude vs dense", fit.amplitude[0].numpy(), amp, (H, N, J, nm))
        check("finish chi2_null vs dense", fit.chi2_null.numpy(), [chi2_0], (H, N, J, nm))
    p = finish_of(D, T, H).power[0].numpy()
    assert np.all(p >= 0.0) and np.all(p <= 1.0)


@pytest.mark.parametrize("P0", [0, 1, 3])
def test_one_term_is_the_periodogram(P0):
    """finish(nterms=1) against periodogram.finish on the same S0, T: within the criterion, the same NaN positions (w = 0
    is among the frequencies)."""
    from celerite2_amd import periodogram as pg

    D = R.case(60 + P0, 60, 4, P0)
    freq = np.concatenate([[0.0], D["freq"][:20]])
    T = PR.whitened_sinusoids(*[D[x] for x in SWEEP[:-1]], freq)
    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    for nm in ("standard", "chi2", "log_likelihood"):
        one = finish_of(D, T, 1, nm)
        ref = pg.finish(S0, torch.from_numpy(T)[None], 60, nm)
        assert bool(torch.isnan(ref.power[0, 0])) and bool(torch.isfinite(ref.power[0, 1:]).all())   # (w = 0: the sine is zero)
        for name, x, xo in zip(one._fields, one, ref):
            check("finish(nterms=1) vs periodogram.finish", x.numpy(), xo.numpy(), (P0, nm, name))


def test_nested_models():
    """dchi2 at H is at least dchi2 at H - 1 at every frequency, up to the criterion's floor."""
    D = R.case(31, 120, 4, 2)
    D["freq"] = R.grid(D["t"], 40, 1.0, 12.0)
    prev = None
    for H in TERMS:
        p = finish_of(D, R.whitened_harmonics(*[D[x] for x in SWEEP], H), H, "chi2").power[0].numpy()
        assert np.all(np.isfinite(p))
        if prev is not None:
            assert np.all(p >= prev - (1e-10 * np.abs(prev) + 1e-12 * np.abs(prev).max())), H
        prev = p


def test_injected_two_harmonic_signal():
    """A signal with a fundamental and a strong second harmonic at a grid frequency, added to a draw: at the true frequency
    the H = 2 power exceeds the H = 1 power, the H = 2 amplitudes are dense GLS's, and `waveform` of the fit reproduces the
    injected periodic part to the noise: the draw's own scatter is of order one and the fit averages N = 150 points into
    four amplitudes, so each is known to a few tenths; an rms misfit below 0.5 of a signal of rms 2.5 is asked."""
    from celerite2_amd import harmonics as hm

    D = R.case(21, 150, 4, 1)
    D["freq"] = R.grid(D["t"], 40, 1.0, 20.0)
    k = 17
    w = D["freq"][k]
    signal = 2.0 * np.cos(w * D["t"] - 0.8) + 3.0 * np.sin(2.0 * w * D["t"] + 0.3)
    y = D["y"] + signal
    D["Z0"] = PR.sweep(D["t"], D["c"], D["U"], D["W"], np.concatenate([D["A0"], y[:, None]], axis=1))[0]
    one = finish_of(D, R.whitened_harmonics(*[D[x] for x in SWEEP], 1), 1)
    two = finish_of(D, R.whitened_harmonics(*[D[x] for x in SWEEP], 2), 2)
    assert float(two.power[0, k]) > float(one.power[0, k])
    assert int(torch.argmax(two.power[0])) == k
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, chi2_0 = R.dense_harmonics(K, D["t"], D["A0"], y, D["freq"], 2)
    check("finish power vs dense", two.power[0].numpy(), dchi2 / chi2_0, "injected")
    check("finish amplitude vs dense", two.amplitude[0].numpy(), amp, "injected")
    wave = hm.waveform(two.amplitude, torch.from_numpy(D["freq"]), torch.from_numpy(D["t"]))
    assert tuple(wave.shape) == (1, 40, 150)
    check("waveform vs numpy", wave[0, k].numpy(), R.waveform(amp[k], w, D["t"]), "injected")
    rms = float(np.sqrt(np.mean((wave[0, k].numpy() - signal) ** 2)))
    print("waveform rms misfit: %.3g of a signal of rms %.3g" % (rms, np.sqrt(np.mean(signal ** 2))))
    assert rms < 0.5
    # t_ref, per-series times, and the shape checks
    tb = torch.from_numpy(np.stack([D["t"], D["t"] + 1.0]))
    ab = torch.cat([two.amplitude, two.amplitude])
    wb = hm.waveform(ab, torch.from_numpy(D["freq"]), tb, t_ref=0.5)
    check("waveform vs numpy", wb[1, k].numpy(), R.waveform(amp[k], w, D["t"] + 1.0, 0.5), "batched, t_ref")
    with pytest.raises(ValueError, match="Invalid shape: amplitude"):
        hm.waveform(ab[..., :3], torch.from_numpy(D["freq"]), tb)
    with pytest.raises(ValueError, match="Invalid shape: freq"):
        hm.waveform(ab, torch.from_numpy(D["freq"][:7]), tb)
    with pytest.raises(ValueError, match="Invalid shape: t"):
        hm.waveform(ab, torch.from_numpy(D["freq"]), tb[:1].expand(3, 150))


def test_nan_rules():
    """w = 0 beside a constant column is NaN and leaves the other frequencies alone; on an evenly spaced grid a frequency
    whose second harmonic aliases onto the constant is NaN at that frequency only; N < P0 + 2 H + 1 is NaN everywhere; a
    series that is not `ok` is NaN throughout and leaves its neighbours their bits."""
    from celerite2_amd import harmonics as hm

    D = R.case(5, 33, 3, 2)
    freq = np.concatenate([[0.0], R.grid(D["t"], 6, 1.0, 4.0)])
    args = [D[x] for x in SWEEP[:-2]]
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    for H in (2, 3):
        T = R.whitened_harmonics(*args, D["Z0"], freq, H)
        fit = finish_of(D, T, H)
        assert bool(torch.isnan(fit.power[0, 0])) and bool(torch.isnan(fit.amplitude[0, 0]).all())
        assert bool(torch.isfinite(fit.power[0, 1:]).all()) and bool(torch.isfinite(fit.amplitude[0, 1:]).all())
        dchi2, _, chi2_0 = R.dense_harmonics(K, D["t"], D["A0"], D["y"], freq[1:], H)
        check("finish power vs dense", fit.power[0, 1:].numpy(), dchi2 / chi2_0, ("w = 0 aside", H))
    # an even grid of unit spacing: at w = pi the second harmonic is cos(2 pi n) = 1, the constant column
    E = R.case(6, 32, 2, 1)
    E["t"] = np.arange(32.0)
    E["d"], E["W"] = PR.factor(E["t"], E["c"], E["a"], E["U"], E["V"])
    E["Z0"] = PR.sweep(E["t"], E["c"], E["U"], E["W"], E["Y0"])[0]
    fe = np.array([0.4, np.pi, 1.1, 2.0])
    fit = finish_of(E, R.whitened_harmonics(*[E[x] for x in SWEEP[:-1]], fe, 2), 2)
    assert [bool(x) for x in torch.isnan(fit.power[0])] == [False, True, False, False]
    assert [bool(x) for x in torch.isnan(fit.amplitude[0]).all(dim=-1)] == [False, True, False, False]
    assert bool(torch.isfinite(finish_of(E, R.whitened_harmonics(*[E[x] for x in SWEEP[:-1]], fe, 1), 1).power[0, 1]))
    # too few points: N = 6 < P0 + 2 H + 1 = 7 at H = 2 with two nuisance columns; N = 7 is enough
    for N, nan in ((6, True), (7, False)):
        S = R.case(8, N, 2, 2, F=5)
        fit = finish_of(S, R.whitened_harmonics(*[S[x] for x in SWEEP], 2), 2)
        assert bool(torch.isnan(fit.power).all()) == nan and bool(torch.isnan(fit.amplitude).all()) == nan
        assert bool(torch.isfinite(fit.chi2_null).all())
    # ok= masks a series; a repeated nuisance column is NaN throughout
    T = R.whitened_harmonics(*args, D["Z0"], freq, 2)
    fit = finish_of(D, T, 2)
    Y2 = D["Y0"].copy()
    Y2[:, 1] = Y2[:, 0]                      # rank 1
    Z2 = PR.sweep(D["t"], D["c"], D["U"], D["W"], Y2)[0]
    T2 = R.whitened_harmonics(*args, Z2, freq, 2)
    S0 = torch.from_numpy(np.stack([R.null_products(Z, D["d"]) for Z in (D["Z0"], Z2, D["Z0"])]))
    TT = torch.from_numpy(np.stack([T, T2, T]))
    got = hm.finish(S0, TT, 33, 2, ok=torch.tensor([True, True, False]))
    for b in (1, 2):
        assert bool(torch.isnan(got.power[b]).all()) and bool(torch.isnan(got.amplitude[b]).all()) and bool(torch.isnan(got.chi2_null[b]))
    for x, xo in zip(got, fit):
        assert np.array_equal(x[0].numpy(), xo[0].numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="normalization"):
        hm.finish(S0, TT, 33, 2, "psd")
    with pytest.raises(ValueError, match=r"^Invalid shape: T "):
        hm.finish(S0, TT[..., :-1], 33, 2)
    with pytest.raises(ValueError, match="nterms"):
        hm.finish(S0, TT, 33, 0)


# ---- the binding of the eighth header ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def har_args(B=1, N=4, J=2, Q0=1, F=3, H=2, p=None, T=None, t_ref=0.0):
    return [B, N, J, Q0, F, H, p, 0, p, 0, p, p, p, p, p, 0, t_ref, T, None]


def test_harmonics_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib, ops

    text = open(_lib.header_path("harmonics")).read()
    fn = lib.c2_whitened_harmonics
    assert len(fn.argtypes) == 19 and fn.restype is ctypes.c_int
    assert fn.argtypes[:6] == (ctypes.c_int64,) * 6 and fn.argtypes[6] is _lib.Pointer and fn.argtypes[15] is ctypes.c_int64
    assert fn.argtypes[16] is ctypes.c_double and fn.argtypes[17] is _lib.Pointer
    assert int(re.search(r"^#define\s+C2_HARMONICS_MAX\s+(\d+)", text, flags=re.M).group(1)) == ops.HARMONICS_MAX == 4
    # the pinned tables of the searches are as they were
    assert set(ops._TRIAL_TABLE) == {"periodogram", "transit", "keplerian", "shape"}


def test_bad_harmonic_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_whitened_harmonics(*har_args()[:-1])
    with pytest.raises(refused):
        lib.c2_whitened_harmonics(*har_args(), None)
    with pytest.raises(refused):
        lib.c2_whitened_harmonics(*har_args(H=2.0))
    with pytest.raises(refused):
        lib.c2_whitened_harmonics(*har_args(t_ref="0"))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_whitened_harmonics(*har_args(p=text))


def test_harmonic_argument_errors(lib):
    """Sizes, null pointers, H = 0, H = 5, J = 33 and Q0 = 9 are refused before anything is launched: no device is needed."""
    from celerite2_amd import _lib

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    for H in (1, 2, 3, 4):
        for bad in (dict(B=0), dict(N=0), dict(J=0), dict(Q0=0), dict(F=0), dict(N=-1), dict(F=-3)):
            assert lib.c2_whitened_harmonics(*har_args(H=H, p=p, T=p, **bad)) == _lib.C2_ERR_INVALID, (H, bad)
        assert lib.c2_whitened_harmonics(*har_args(H=H, p=p, T=None)) == _lib.C2_ERR_INVALID
        assert lib.c2_whitened_harmonics(*har_args(H=H, p=None, T=p)) == _lib.C2_ERR_INVALID
        assert lib.c2_whitened_harmonics(*har_args(H=H, J=33, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
        assert lib.c2_whitened_harmonics(*har_args(H=H, Q0=9, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    for H in (0, -1):
        assert lib.c2_whitened_harmonics(*har_args(H=H, p=p, T=p)) == _lib.C2_ERR_INVALID
    for H in (5, 64):
        assert lib.c2_whitened_harmonics(*har_args(H=H, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    # 2^31 blocks or more: 32 trials a block at H = 2 up to J = 16, 16 at H = 3, 4; 16 and 8 at J = 32
    assert lib.c2_whitened_harmonics(*har_args(B=2 ** 31, F=32, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_harmonics(*har_args(B=2 ** 25, F=64 * 32, H=2, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_harmonics(*har_args(B=2 ** 25, F=64 * 16, H=3, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_harmonics(*har_args(B=2 ** 25, F=64 * 16, H=2, J=32, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_harmonics(*har_args(B=2 ** 25, F=64 * 8, H=4, J=32, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED


def test_ops_errors_name_the_argument():
    """ops.whitened_harmonics refuses nterms outside 1 .. 4 by name, before anything else, and describes its arguments with
    the shared specs (CPU tensors: the dtype / device check comes first)."""
    from celerite2_amd import ops

    z = [torch.zeros(5), torch.zeros(2), torch.zeros(2, 5, 2), torch.zeros(2, 5, 2), torch.zeros(2, 5), torch.zeros(2, 5, 3), torch.zeros(4)]
    for bad in (0, 5, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="nterms"):
            ops.whitened_harmonics(*z, bad)
    with pytest.raises(ValueError, match="GPU"):
        ops.whitened_harmonics(*z, 2)


def test_worst_case_report():
    from celerite2_amd import harmonics  # noqa: F401  (the report belongs to the module under test)

    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
