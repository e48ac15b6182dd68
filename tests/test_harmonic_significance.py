# -*- coding: utf-8 -*-
"""False-alarm probabilities of the multi-harmonic periodogram on the CPU: the many-series finish
(celerite2_amd/harmonics.py, null_statistics) on the restated products (tests/harmonic_significance_ref.py) against two dense
generalized-least-squares fits per frequency and draw of y_r = L D^1/2 n_r formed densely, against harmonics.finish at one
draw, against significance.null_statistics at one term, the NaN rules, and the binding of the ninth public header
(include/celerite2_amd_harmonic_trials.h), which needs no device.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import harmonic_significance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMALIZATIONS = ("standard", "chi2", "log_likelihood")
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


def tn(a):
    return torch.from_numpy(np.ascontiguousarray(a))[None]


def products(D, H, normals):
    """What null_statistics reads for the case D and the draws of `normals` (N, R), each with a leading batch axis of one:
    (y (N, R) formed densely, S0, T, G0Y, s_yy, P)."""
    y, s_yy, G0Y, alpha = R.null_draws(D, normals)
    T = R.HR.whitened_harmonics(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0")], D["freq"], H)
    P = R.projections(D["t"], alpha, D["freq"], H)
    return y, tn(R.HR.null_products(D["Z0"], D["d"])), tn(T), tn(G0Y), tn(s_yy), tn(P)


# ---- the identities against dense algebra ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 40])
@pytest.mark.parametrize("P0", [0, 1, 3])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_restated_projection_against_dense(H, P0, N):
    """P = col^T alpha, and with alpha = (K + D)^-1 y it is the entry gty of the restated sweep's T; both against
    np.linalg.solve on the dense matrix."""
    D = R.case(7 + H + 10 * P0 + N, N, 3, P0, 6, H)
    Kd = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    alpha = np.linalg.solve(Kd, D["y"])[:, None]
    P = R.projections(D["t"], alpha, D["freq"], H)
    assert P.shape == (6, 2 * H, 1)
    col = R.HR.columns(D["t"], D["freq"], H)                                # (NC, N, F)
    check("restated P vs dense col^T alpha", P[..., 0], np.einsum("cnf,n->fc", col, alpha[:, 0]), (H, P0, N))
    want = R.HR.dense_products(Kd, D["t"], D["Y0"], D["freq"], H)
    Q0, HEAD = P0 + 1, H * (2 * H + 1)
    gty = np.stack([want[:, HEAD + i * Q0 + P0] for i in range(2 * H)], axis=1)
    check("restated P vs dense gty", P[..., 0], gty, (H, P0, N))


@pytest.mark.parametrize("N", [17, 40])
@pytest.mark.parametrize("P0", [0, 1, 3])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_null_statistics_against_dense(H, P0, N):
    """For given normals the draws y_r = L D^1/2 n_r are formed densely and fitted densely, twice per frequency; the fused
    route never forms them.  F = 6 frequencies, R = 5 draws; N = 17 leaves 17 - 3 - 8 = 6 degrees of freedom at the least."""
    from celerite2_amd import harmonics as hm

    D = R.case(100 * H + 10 * P0 + N, N, 3, P0, 6, H)
    normals = np.random.default_rng(H + P0 + N).normal(size=(N, 5))
    y, S0, T, G0Y, s_yy, P = products(D, H, normals)
    dchi2, chi2_0 = R.dense_statistics(D, y, H)
    for nm in NORMALIZATIONS:
        got = hm.null_statistics(S0, T, G0Y, s_yy, P, N, H, normalization=nm)
        assert tuple(got.shape) == (1, 6, 5) and bool(torch.isfinite(got).all())
        check("null_statistics vs dense fits of y_r", got[0].numpy(), R.normalized(dchi2, chi2_0[None, :], nm), (H, P0, N, nm))
    # the kernel's lines, restated, on the same factors
    fac = hm.null_factors(S0, T, N, H)
    V, c0 = hm.null_draws(fac, G0Y, s_yy)
    D2 = R.null_chi2(P[0].numpy(), fac.Lm[0].numpy(), None if fac.Xt is None else fac.Xt[0].numpy(), None if V is None else V[0].numpy())
    check("restated kernel lines vs dense fits of y_r", D2, dchi2, (H, P0, N))
    check("chi2_0 of the draws vs dense fits", c0[0].numpy(), chi2_0, (H, P0, N))
    assert tuple(fac.Lm.shape) == (1, 6, H * (2 * H + 1)) and (fac.Xt is None) == (P0 == 0)
    assert fac.Xt is None or tuple(fac.Xt.shape) == (1, 6, 2 * H, P0)


# ---- one draw: the existing finish; one term: the existing many-series finish --------------------------------------------
@pytest.mark.parametrize("P0", [0, 1, 3])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_single_draw_is_finish(H, P0):
    """With R = 1 and the series' own products -- g0y, s_yy of S0, gty of T -- null_statistics is finish's power."""
    from celerite2_amd import harmonics as hm

    N, F = 60, 20
    D = R.case(50 + P0 + H, N, 4, P0, F, H)
    Q0, HEAD = P0 + 1, H * (2 * H + 1)
    S0 = tn(R.HR.null_products(D["Z0"], D["d"]))
    T = tn(R.HR.whitened_harmonics(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0")], D["freq"], H))
    P = torch.stack([T[..., HEAD + i * Q0 + P0] for i in range(2 * H)], dim=2)[..., None].contiguous()
    G0Y, s_yy = S0[:, :P0, P0, None], S0[:, P0, P0, None]
    for nm in NORMALIZATIONS:
        got = hm.null_statistics(S0, T, G0Y, s_yy, P, N, H, normalization=nm)
        want = hm.finish(S0, T, N, H, nm).power
        assert bool(torch.isfinite(want).all())
        check("one draw vs finish", got[..., 0].numpy(), want.numpy(), (H, P0, nm))


@pytest.mark.parametrize("P0", [0, 1, 3])
def test_one_term_is_the_periodograms_null_statistics(P0):
    from celerite2_amd import harmonics as hm, significance as sg

    N = 33
    D = R.case(3 + P0, N, 3, P0, 9, 1)
    normals = np.random.default_rng(P0).normal(size=(N, 4))
    _, S0, T, G0Y, s_yy, P = products(D, 1, normals)
    for nm in NORMALIZATIONS:
        got = hm.null_statistics(S0, T, G0Y, s_yy, P, N, 1, normalization=nm)
        want = sg.null_statistics("periodogram", S0, T, G0Y, s_yy, P, N, normalization=nm)
        assert bool(torch.isfinite(want).all())
        check("nterms = 1 vs significance.null_statistics", got.numpy(), want.numpy(), (P0, nm))


def test_factors_are_the_finishs():
    """finish and null_factors read one factorisation: finish's NaN frequencies are null_factors' singular ones, and Lm L^T
    rebuilds M = Gtt - X^T X from T."""
    from celerite2_amd import harmonics as hm

    H, P0, N, F = 3, 2, 40, 7
    D = R.case(11, N, 3, P0, F, H)
    S0 = tn(R.HR.null_products(D["Z0"], D["d"]))
    T = tn(R.HR.whitened_harmonics(*[D[x] for x in ("t", "c", "U", "W", "d", "Z0")], D["freq"], H))
    fac = hm.null_factors(S0, T, N, H)
    fit = hm.finish(S0, T, N, H)
    assert torch.equal(torch.isnan(fit.power), fac.singular) and not bool(fac.singular.any())
    NC = 2 * H
    L = np.zeros((F, NC, NC))
    for i in range(NC):
        for j in range(i + 1):
            L[:, i, j] = fac.Lm[0, :, i * (i + 1) // 2 + j].numpy()
    X = np.transpose(fac.Xt[0].numpy(), (0, 2, 1))                          # (F, P0, NC)
    Gtt = np.zeros((F, NC, NC))
    for i in range(NC):
        for j in range(i, NC):
            Gtt[:, i, j] = Gtt[:, j, i] = T[0, :, R.HR.tri(i, j, NC)].numpy()
    check("Lm Lm^T vs Gtt - X^T X", L @ np.transpose(L, (0, 2, 1)), Gtt - np.transpose(X, (0, 2, 1)) @ X)


# ---- the NaN rules ---------------------------------------------------------------------------------------------------------
def test_nan_rules():
    """w = 0 beside a constant column is NaN at that frequency only; N < P0 + 2 H + 1 is NaN throughout; a series not taken
    is NaN throughout and its neighbour keeps its bits."""
    from celerite2_amd import harmonics as hm

    H, P0, N, F = 2, 1, 33, 8
    D = R.case(5, N, 3, P0, F, H)
    normals = np.random.default_rng(3).normal(size=(N, 4))
    _, S0, T, G0Y, s_yy, P = products(D, H, normals)
    good = hm.null_statistics(S0, T, G0Y, s_yy, P, N, H)
    assert bool(torch.isfinite(good).all())
    E = dict(D)
    E["freq"] = D["freq"].copy()
    E["freq"][4] = 0.0
    _, S0e, Te, _, _, Pe = products(E, H, normals)
    got = hm.null_statistics(S0e, Te, G0Y, s_yy, Pe, N, H)
    keep = np.arange(F) != 4
    assert bool(torch.isnan(got[0, 4]).all()) and np.array_equal(got[0, keep].numpy(), good[0, keep].numpy())
    fac = hm.null_factors(S0e, Te, N, H)
    assert fac.singular[0].tolist() == [f == 4 for f in range(F)] and bool(torch.isnan(fac.Lm[0, 4]).all())
    assert bool(torch.isfinite(fac.Lm[0, keep]).all())
    # no degree of freedom left: N < P0 + 2 H + 1
    short = hm.null_statistics(S0, T, G0Y, s_yy, P, P0 + 2 * H, H)
    assert bool(torch.isnan(short).all())
    assert bool(torch.isfinite(hm.null_statistics(S0, T, G0Y, s_yy, P, P0 + 2 * H + 1, H)).all())
    # a series not taken, and one whose A0 is rank-deficient
    two = lambda a: torch.cat([a, a])
    both = hm.null_statistics(two(S0), two(T), two(G0Y), two(s_yy), two(P), N, H, ok=torch.tensor([True, False]))
    assert bool(torch.isnan(both[1]).all()) and torch.equal(both[0], good[0])
    S0d = two(S0).clone()
    S0d[1, :P0, :P0] = 0.0
    both = hm.null_statistics(S0d, two(T), two(G0Y), two(s_yy), two(P), N, H)
    assert bool(torch.isnan(both[1]).all()) and torch.equal(both[0], good[0])
    assert hm.null_factors(S0d, two(T), N, H).bad.tolist() == [False, True]


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    """harmonics.null_statistics, the two ops and gp.search_significance raise ValueError, naming the argument, before C."""
    import types

    from celerite2_amd import gp as G, harmonics as hm, ops

    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    H, P0, F, Rn = 2, 1, 5, 3
    S0, T = torch.eye(P0 + 1, dtype=torch.float64)[None], z(1, F, H * (2 * H + 1) + 2 * H * (P0 + 1))
    args = (S0, T, z(1, P0, Rn), z(1, Rn), z(1, F, 2 * H, Rn), 40)
    with pytest.raises(ValueError, match="normalization"):
        hm.null_statistics(*args, H, normalization="psd")
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError, match="nterms"):
            hm.null_statistics(*args, bad)
    with pytest.raises(ValueError, match=r"^Invalid shape: P "):
        hm.null_statistics(*args[:4], z(1, F, 2, Rn), 40, H)
    with pytest.raises(ValueError, match=r"^Invalid shape: s_yy, G0Y "):
        hm.null_statistics(*args[:3], z(1, Rn + 1), args[4], 40, H)
    with pytest.raises(ValueError, match=r"^Invalid shape: T "):
        hm.null_statistics(S0, T[..., :-1], *args[2:], H)
    for op in (ops.harmonic_projections, lambda *a: ops.harmonic_null_chi2(*a, z(2, 6, 10))):
        for bad in (0, 5, 2.0, True):
            with pytest.raises(ValueError, match="nterms"):
                op(z(5), z(2, 5, 3), z(6), bad)
        with pytest.raises(ValueError, match=r"^Invalid shape: alpha "):
            op(z(5), z(5, 3), z(6), 2)
        with pytest.raises(ValueError, match=r"^Invalid shape: freq "):
            op(z(5), z(2, 5, 3), z(6, 1, 1), 2)
        with pytest.raises(ValueError, match="GPU"):
            op(z(5), z(2, 5, 3), z(6), 2)
    with pytest.raises(ValueError, match=r"^Invalid shape: Xt, V "):
        ops.harmonic_null_chi2(z(5), z(2, 5, 3), z(6), 2, z(2, 6, 10), z(2, 6, 4, 1), None)
    with pytest.raises(ValueError, match=r"^Invalid shape: V "):
        ops.harmonic_null_chi2(z(5), z(2, 5, 3), z(6), 2, z(2, 6, 10), z(2, 6, 4, 8), z(2, 8, 3))
    dims = dict(B=2, N=5, R=3, K=6, C=4, L=10, P=1)
    ops._shapes(dims, [("Lm", z(2, 6, 10), "BKL"), ("Xt", z(2, 6, 4, 1), "BKCP"), ("V", z(2, 1, 3), "BPR"), ("out", z(2, 6, 3), "BKR")])
    for name, bad, spec in (("Lm", z(2, 6, 9), "BKL"), ("Xt", z(2, 6, 1, 4), "BKCP"), ("V", z(2, 3, 1), "BPR"), ("out", z(2, 3, 6), "BKR")):
        with pytest.raises(ValueError, match=r"^Invalid shape: %s " % name):
            ops._shapes(dims, [(name, bad, spec)])
    gp = types.SimpleNamespace(_need=lambda: None, _check_vector=lambda y: None, _diag=z(2, 5), mean=0.0, _t=z(5))
    call = lambda *a, **k: G.GaussianProcess.search_significance(gp, *a, **k)
    for bad in (0, 5, 2.0, True, None):
        with pytest.raises(ValueError, match="nterms"):
            call("periodogram", z(2, 5), z(6), nterms=bad)
    for kind, trials in (("transit", z(6, 4)), ("keplerian", z(6, 3))):
        with pytest.raises(ValueError, match="nterms"):
            call(kind, z(2, 5), trials, nterms=2)
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        call("periodogram", z(2, 5), z(3, 6), nterms=2)
    with pytest.raises(ValueError, match="normalization"):
        call("periodogram", z(2, 5), z(6), nterms=3, normalization="psd")


# ---- the binding of the ninth header -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def proj_args(B=1, N=4, F=3, H=2, R=2, p=None, P=None, t_ref=0.0):
    return [B, N, F, H, R, p, 0, p, 0, t_ref, p, P, None]


def null_args(B=1, N=4, F=3, H=2, R=2, P0=1, p=None, D=None, Lm="p", Xt="p", V="p"):
    pick = lambda x: p if isinstance(x, str) else x
    return [B, N, F, H, R, P0, p, 0, p, 0, 0.0, p, pick(Lm), pick(Xt), pick(V), D, None]


def test_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib, ops, significance as sg

    text = open(_lib.header_path("harmonic_trials")).read()
    for name, n, ints in (("c2_harmonic_projections", 13, 5), ("c2_harmonic_null_chi2", 17, 6)):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n and fn.restype is ctypes.c_int, name
        assert fn.argtypes[:ints] == (ctypes.c_int64,) * ints and fn.argtypes[ints] is _lib.Pointer, name
        assert fn.argtypes[ints + 1] is fn.argtypes[ints + 3] is ctypes.c_int64 and fn.argtypes[ints + 4] is ctypes.c_double, name
        assert all(a is _lib.Pointer for a in fn.argtypes[ints + 5:]), name
    # the draws a wavefront: one value per H, multiples of 16, the header's
    defs = {int(h): int(v) for h, v in re.findall(r"^#define\s+C2_HARMONIC_DRAWS_(\d+)\s+(\d+)", text, flags=re.M)}
    assert ops.HARMONIC_DRAWS == defs and sorted(defs) == list(range(1, ops.HARMONICS_MAX + 1))
    assert all(v % 16 == 0 and v >= 16 for v in defs.values())
    # the pinned tables of the searches are as they were
    assert sg.KINDS == ("periodogram", "transit", "keplerian")
    assert set(sg.SEARCHES) == set(ops._TRIAL_TABLE) == {"periodogram", "transit", "keplerian", "shape"}
    assert set(ops.TRIAL_KINDS) == set(sg.KINDS)
    # one statement of the harmonic's frequency and of every column rule
    csrc = os.path.join(ROOT, "celerite2_amd", "csrc")
    stated = [src for src in sorted(os.listdir(csrc)) if re.search(r"\bharmonic\s*\(int h\b", open(os.path.join(csrc, src)).read())]
    assert stated == ["c2_trial_columns.hpp"]
    for src in ("c2_harmonics.hip", "c2_harmonic_trials.hip"):
        body = open(os.path.join(csrc, src)).read()
        assert '#include "c2_trial_columns.hpp"' in body and ("pgram::harmonic(" in body or "trial::Harmonics<" in body), src


def test_bad_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    for fn, args in ((lib.c2_harmonic_projections, proj_args), (lib.c2_harmonic_null_chi2, null_args)):
        with pytest.raises(refused):
            fn(*args()[:-1])
        with pytest.raises(refused):
            fn(*args(), None)
        with pytest.raises(refused):
            fn(*args(H=2.0))
        for text in ("t", b"t"):
            with pytest.raises(refused):
                fn(*args(p=text))


def test_argument_errors(lib):
    """Sizes, null pointers, H and P0 beyond their limits and 2^31 blocks are refused before anything is launched: no device
    is needed."""
    from celerite2_amd import _lib, ops

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    INV, UNS = _lib.C2_ERR_INVALID, _lib.C2_ERR_UNSUPPORTED
    proj = lambda **k: lib.c2_harmonic_projections(*proj_args(p=p, P=p, **k))
    null = lambda **k: lib.c2_harmonic_null_chi2(*null_args(p=p, D=p, **k))
    for H in (1, 2, 3, 4):
        for bad in (dict(B=0), dict(N=0), dict(F=0), dict(R=0), dict(N=-1), dict(F=-3)):
            assert proj(H=H, **bad) == INV and null(H=H, **bad) == INV, (H, bad)
        assert lib.c2_harmonic_projections(*proj_args(H=H, p=p, P=None)) == INV
        assert lib.c2_harmonic_projections(*proj_args(H=H, p=None, P=p)) == INV
        assert lib.c2_harmonic_null_chi2(*null_args(H=H, p=p, D=None)) == INV
        assert lib.c2_harmonic_null_chi2(*null_args(H=H, p=None, D=p, Lm=p, Xt=p, V=p)) == INV
        for gone in ("Lm", "Xt", "V"):
            assert null(H=H, **{gone: None}) == INV, (H, gone)
        assert null(H=H, P0=-1) == INV and null(H=H, P0=8) == UNS
        for i in (6, 8):
            neg = proj_args(H=H, p=p, P=p)
            neg[i] = -3
            assert lib.c2_harmonic_projections(*neg) == INV
        for i in (7, 9):
            neg = null_args(H=H, p=p, D=p)
            neg[i] = -3
            assert lib.c2_harmonic_null_chi2(*neg) == INV
        # 2^31 blocks or more: 16 frequencies and C2_HARMONIC_DRAWS_H draws a block
        RB = ops.HARMONIC_DRAWS[H]
        for fn in (proj, null):
            assert fn(H=H, B=2 ** 31, F=16, R=RB) == UNS
            assert fn(H=H, B=2 ** 11, F=16 * 2 ** 10, R=RB * 2 ** 10) == UNS
            assert fn(H=H, B=1, F=16 * 2 ** 31, R=1) == UNS
    for H in (0, -1):
        assert proj(H=H) == INV and null(H=H) == INV
    for H in (5, 64):
        assert proj(H=H) == UNS and null(H=H) == UNS


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst, %s: %.3g" % (k, WORST[k]))
