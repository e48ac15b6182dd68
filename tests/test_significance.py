# -*- coding: utf-8 -*-
"""False-alarm probabilities of the three searches on the CPU: the many-series finish (celerite2_amd/significance.py,
null_statistics) on the restated products (tests/trial_projections_ref.py) against two dense generalized-least-squares fits
per trial and draw of y_r = L D^1/2 n_r formed densely, against the existing `finish` of each search at one draw, the
counting rules of false_alarm_probability and false_alarm_level, `dips_only`, and the binding of the sixth public header
(include/celerite2_amd_trials.h), which needs no device.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import trial_projections_ref as R

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


def fused(kind, D, normals, **kw):
    """null_statistics (K, R) fed the restated products of the case D and the draws of `normals` (N, R)."""
    from celerite2_amd import significance as sg

    y, s_yy, G0Y, alpha = R.null_draws(D, normals)
    trials = D[R.TRIALS_KEY[kind]]
    P = R.projections(kind, D["t"], alpha, trials)
    tn = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]
    S0 = tn(R.PR.null_products(D["Z0"], D["d"]))
    got = sg.null_statistics(kind, S0, tn(R.sweep_products(kind, D)), tn(G0Y), tn(s_yy), tn(P), len(D["t"]),
                             trials=None if kind == "periodogram" else torch.from_numpy(trials), **kw)
    assert tuple(got.shape) == (1, len(trials), normals.shape[1])
    return y, got[0].numpy()


def finish_nan(kind, D):
    """(K,) bool: the trials at which the existing finish of the kind holds NaN for the case's own series."""
    from celerite2_amd import kepler as kp, periodogram as pg, transit as tr

    S0 = torch.from_numpy(R.PR.null_products(D["Z0"], D["d"]))[None]
    T, N = torch.from_numpy(R.sweep_products(kind, D))[None], len(D["t"])
    if kind == "periodogram":
        x = pg.finish(S0, T, N).power
    elif kind == "keplerian":
        x = kp.finish(S0, T, N, trials=torch.from_numpy(D["trials"])).power
    else:
        x = tr.finish(S0, T, N, trials=torch.from_numpy(D["trials"])).delta_chi2
    return torch.isnan(x)[0].numpy()


# ---- the identities against dense algebra ------------------------------------------------------------------------------
@pytest.mark.parametrize("P0", [0, 1, 3])
@pytest.mark.parametrize("J", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 2, 5, 17, 150])
@pytest.mark.parametrize("kind", R.KINDS)
def test_null_statistics_against_dense(kind, N, J, P0):
    """For given normals the draws y_r = L D^1/2 n_r are formed densely and fitted densely, twice per trial; the fused route
    never forms them.  Below N = P0 + 3 (the transit: P0 + 2) no degree of freedom is left and every trial is NaN.  At N = 5
    the fits have one or two degrees of freedom left; the criterion is the standing one all the same."""
    seed = 1000 * R.KINDS.index(kind) + 10 * N + J + 100 * P0
    D = R.case(kind, seed, N, J, P0, K=9)
    normals = np.random.default_rng(seed + 1).normal(size=(N, 3))
    for nm in NORMALIZATIONS:
        y, got = fused(kind, D, normals, normalization=nm)
        if N < P0 + (2 if kind == "transit" else 3):
            assert np.isnan(got).all(), (kind, N, P0)
            continue
        if nm == "standard":
            dchi2, chi2_0, _ = R.dense_statistics(kind, D, y)
        want = R.normalized(dchi2, chi2_0[None, :], nm)
        want = np.where(finish_nan(kind, D)[:, None], np.nan, want)   # (singular trials: where the existing finish has them)
        check("%s: null_statistics vs dense fits of y_r" % kind, got, want, (N, J, P0, nm))


# ---- one draw: the existing finish ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P0", [0, 1, 3])
@pytest.mark.parametrize("kind", R.KINDS)
def test_single_draw_is_the_existing_finish(kind, P0):
    """With R = 1 and the series' own products -- g0y, s_yy of S0, gty of T -- null_statistics is the existing finish."""
    from celerite2_amd import kepler as kp, periodogram as pg, significance as sg, transit as tr

    D = R.case(kind, 50 + P0, 60, 4, P0, K=20)
    Q0, N = P0 + 1, 60
    S0 = torch.from_numpy(R.PR.null_products(D["Z0"], D["d"]))[None]
    T = torch.from_numpy(R.sweep_products(kind, D))[None]
    trials = torch.from_numpy(D[R.TRIALS_KEY[kind]])
    if kind == "transit":
        P = T[:, :, None, 1 + P0, None]
    else:
        P = torch.stack([T[..., 3 + P0], T[..., 3 + Q0 + P0]], dim=2)[..., None]
    G0Y, s_yy = S0[:, :P0, P0, None], S0[:, P0, P0, None]
    for nm in NORMALIZATIONS:
        got = sg.null_statistics(kind, S0, T, G0Y, s_yy, P.contiguous(), N, normalization=nm,
                                 trials=None if kind == "periodogram" else trials)
        if kind == "periodogram":
            want = pg.finish(S0, T, N, nm).power
        elif kind == "keplerian":
            want = kp.finish(S0, T, N, nm, trials=trials).power
        else:
            fit = tr.finish(S0, T, N, trials=trials)
            want = R.normalized(fit.delta_chi2, fit.chi2_null[:, None], nm)
        assert bool(torch.isfinite(want).all())
        check("%s: one draw vs finish" % kind, got[..., 0].numpy(), want.numpy(), (P0, nm))


def test_nan_rules():
    """A singular trial, one outside the domain and a series not taken hold NaN for every draw, and their neighbours' bits
    do not change."""
    from celerite2_amd import significance as sg

    for kind in R.KINDS:
        D = R.case(kind, 5, 33, 3, 2, K=10)
        key = R.TRIALS_KEY[kind]
        normals = np.random.default_rng(3).normal(size=(33, 4))
        _, good = fused(kind, D, normals)
        assert np.isfinite(good).all()
        E = dict(D)
        E[key] = D[key].copy()
        if kind == "periodogram":
            E[key][4] = 0.0                                   # w = 0 beside a constant column: not identifiable
        elif kind == "transit":
            E[key][4, 3] = 0.75 * E[key][4, 2]                # tau > w / 2
        else:
            E[key][4, 1] = 0.995                              # e > 0.99
        _, got = fused(kind, E, normals)
        keep = np.arange(10) != 4
        assert np.isnan(got[4]).all() and np.array_equal(got[keep], good[keep]), kind
        # a series not taken
        y, s_yy, G0Y, alpha = R.null_draws(D, normals)
        tn = lambda a: torch.from_numpy(np.ascontiguousarray(np.stack([a, a])))
        args = (tn(R.PR.null_products(D["Z0"], D["d"])), tn(R.sweep_products(kind, D)), tn(G0Y), tn(s_yy),
                tn(R.projections(kind, D["t"], alpha, D[key])), 33)
        both = sg.null_statistics(kind, *args, ok=torch.tensor([True, False]))
        assert bool(torch.isnan(both[1]).all()) and np.array_equal(both[0].numpy(), good)
    with pytest.raises(ValueError, match="kind"):
        sg.null_statistics("bls", *args)
    with pytest.raises(ValueError, match="normalization"):
        sg.null_statistics("keplerian", *args, normalization="psd")
    with pytest.raises(ValueError, match=r"^Invalid shape: P "):
        sg.null_statistics("keplerian", *args[:4], args[4][:, :, :1], 33)
    with pytest.raises(ValueError, match=r"^Invalid shape: s_yy, G0Y "):
        sg.null_statistics("keplerian", *args[:3], args[3][:, :2], args[4], 33)


def test_dips_only():
    """A trial whose fitted depth is positive counts 0 (not NaN); the others are unchanged.  The sign is the dense fit's."""
    D = R.case("transit", 21, 80, 4, 1, K=24)
    normals = np.random.default_rng(8).normal(size=(80, 6))
    y, full = fused("transit", D, normals, normalization="chi2")
    _, dips = fused("transit", D, normals, normalization="chi2", dips_only=True)
    _, _, sign = R.dense_statistics("transit", D, y)
    assert (sign > 0).any() and (sign < 0).any()
    assert np.array_equal(dips[sign > 0], np.zeros((sign > 0).sum())) and np.array_equal(dips[sign < 0], full[sign < 0])
    from celerite2_amd import significance as sg
    # other kinds ignore it
    E = R.case("periodogram", 2, 40, 2, 1, K=6)
    n = np.random.default_rng(1).normal(size=(40, 2))
    assert np.array_equal(fused("periodogram", E, n)[1], fused("periodogram", E, n, dips_only=True)[1])
    assert sg.KINDS == R.KINDS


# ---- the counting rules ------------------------------------------------------------------------------------------------
def test_false_alarm_probability():
    from celerite2_amd import significance as sg

    rng = np.random.default_rng(0)
    B, K, Rn = 3, 40, 25
    maxima = rng.normal(size=(B, Rn))
    stat = rng.normal(size=(B, K)) * 1.5
    stat[:, :5] = maxima[:, :5]                               # ties count: ">="
    stat[0, 7] = stat[2, 9] = np.nan
    stat[1, 11], stat[1, 12] = np.inf, -np.inf
    fap = sg.false_alarm_probability(torch.from_numpy(stat), torch.from_numpy(maxima)).numpy()
    want = np.array([[(1 + np.sum(maxima[b] >= s)) / (Rn + 1) if not np.isnan(s) else np.nan for s in stat[b]] for b in range(B)])
    assert np.array_equal(fap, want, equal_nan=True)
    ok = ~np.isnan(fap)
    assert np.all(fap[ok] >= 1.0 / (Rn + 1)) and np.all(fap[ok] <= 1.0)
    assert fap[1, 11] == 1.0 / (Rn + 1) and fap[1, 12] == 1.0
    assert np.isnan(fap[0, 7]) and np.isnan(fap[2, 9]) and np.isnan(fap).sum() == 2
    for b in range(B):                                        # non-increasing in the statistic
        o = np.argsort(stat[b][ok[b]])
        assert np.all(np.diff(fap[b][ok[b]][o]) <= 0.0)
    # (B,) statistics, and a draw without a valid trial (a NaN maximum) is never at or above
    one = sg.false_alarm_probability(torch.from_numpy(stat[:, 20]), torch.from_numpy(maxima)).numpy()
    assert np.array_equal(one, want[:, 20])
    holed = maxima.copy()
    holed[:, 3] = np.nan
    got = sg.false_alarm_probability(torch.from_numpy(stat), torch.from_numpy(holed)).numpy()
    want2 = np.array([[(1 + np.sum(holed[b] >= s)) / (Rn + 1) if not np.isnan(s) else np.nan for s in stat[b]] for b in range(B)])
    assert np.array_equal(got, want2, equal_nan=True)
    with pytest.raises(ValueError, match=r"^Invalid shape: statistic "):
        sg.false_alarm_probability(torch.zeros(2, 4, dtype=torch.float64), torch.from_numpy(maxima))


def test_false_alarm_level():
    from celerite2_amd import significance as sg

    rng = np.random.default_rng(1)
    maxima = torch.from_numpy(rng.normal(size=(2, 99)))
    for fap in (0.02, 0.05, 0.1, 0.5, 1.0):
        level = sg.false_alarm_level(maxima, fap)
        assert tuple(level.shape) == (2,)
        at = sg.false_alarm_probability(level, maxima)
        assert bool((at <= fap + 1e-12).all()), (fap, at)
        srt = torch.sort(maxima, dim=1, descending=True)[0]
        assert bool((srt == level[:, None]).any(dim=1).all())                # the level is one of the maxima ...
        smaller = srt[:, int((srt[0] >= level[0]).sum()):][:, :1]             # ... and the next smaller one misses `fap`
        if smaller.numel():
            assert bool((sg.false_alarm_probability(smaller, maxima) > fap).all()), fap
    assert sg.false_alarm_level(maxima, 0.019).tolist() == [math.inf, math.inf]     # 99 draws resolve 2 / 100 at best
    assert torch.equal(sg.false_alarm_level(maxima, 0.02), maxima.max(dim=1)[0])
    with pytest.raises(ValueError):
        sg.false_alarm_level(maxima, 0.0)


# ---- the restatement itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_projection_is_the_sweeps_gty(kind):
    """With alpha = (K + D)^-1 y, the restated projection is the entry gty of the restated sweep's T, both against
    np.linalg.solve on the dense matrix."""
    D = R.case(kind, 9, 40, 3, 2, K=15)
    Kd = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    alpha = np.linalg.solve(Kd, D["y"])[:, None]
    trials = D[R.TRIALS_KEY[kind]]
    P = R.projections(kind, D["t"], alpha, trials)
    T = R.sweep_products(kind, D)
    Q0 = 3
    want = R.REF[kind].dense_products(Kd, D["t"], D["Y0"], trials)
    cols = [1 + 2] if kind == "transit" else [3 + 2, 3 + Q0 + 2]
    for c, col in enumerate(cols):
        check("%s: projection vs dense gty" % kind, P[:, c, 0], want[:, col])
        check("%s: sweep gty vs dense gty" % kind, T[:, col], want[:, col])
    assert P.shape == (15, R.NCOL[kind], 1)


# ---- the binding of the sixth header -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def tp_args(kind=0, B=1, N=4, K=3, R=2, p=None, P=None):
    return [kind, B, N, K, R, p, 0, p, 0, 0.0, p, P, None]


def test_trials_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib, ops, significance as sg

    fn = lib.c2_trial_projections
    assert len(fn.argtypes) == 13 and fn.restype is ctypes.c_int
    assert fn.argtypes[0] is ctypes.c_int and fn.argtypes[1:5] == (ctypes.c_int64,) * 4 and fn.argtypes[9] is ctypes.c_double
    assert all(fn.argtypes[i] is _lib.Pointer for i in (5, 7, 10, 11, 12)) and fn.argtypes[6] is fn.argtypes[8] is ctypes.c_int64
    # the op's tables are the headers': codes, draws a wavefront, doubles a trial, columns, the width of T
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(C2_TRIAL_\w+)\s+(\d+)", open(_lib.header_path("trials")).read(), flags=re.M)}
    shapes_h = open(_lib.header_path("shapes")).read()
    defs.update({k: int(v) for k, v in re.findall(r"^#define\s+(C2_SHAPE_\w+)\s+(\d+)", shapes_h, flags=re.M)})
    assert set(ops.TRIAL_KINDS) == set(R.KINDS) and set(ops._TRIAL_TABLE) == set(sg.SEARCHES) == set(R.KINDS) | {"shape"}
    assert sg.KINDS == R.KINDS
    for kind, name in (("periodogram", "SINUSOID"), ("transit", "TRANSIT"), ("keplerian", "KEPLERIAN")):
        code, words, C, RB = ops.TRIAL_KINDS[kind]
        assert (code, RB) == (defs["C2_TRIAL_" + name], defs["C2_TRIAL_%s_DRAWS" % name]) and RB % 16 == 0
        assert (words, C) == (R.WORDS[kind], R.NCOL[kind])
        assert ops._TRIAL_TABLE[kind][:3] + (ops._TRIAL_TABLE[kind].draws, ops._TRIAL_TABLE[kind].bank) == (code, words, C, RB, False)
    shape = ops._TRIAL_TABLE["shape"]
    assert (shape.code, shape.words, shape.columns, shape.draws, shape.bank) == (None, 4, 1, defs["C2_SHAPE_DRAWS"], True)
    assert ops.SHAPE_DRAWS == defs["C2_SHAPE_DRAWS"] and ops.SHAPE_MAX_NODES == defs["C2_SHAPE_MAX_NODES"]
    # the width of T as the headers state it: 3 + 2 Q0 for a two-column kind, 1 + Q0 for a one-column kind
    headers = {"periodogram": "periodogram", "transit": "transit", "keplerian": "kepler", "shape": "shapes"}
    for kind, kd in ops._TRIAL_TABLE.items():
        assert kd.width == ((3, 2) if kd.columns == 2 else (1, 1)), kind
        h = open(os.path.join(ROOT, "include", "celerite2_amd_%s.h" % headers[kind])).read()
        assert ("3 + 2 Q0" if kd.columns == 2 else "1 + Q0") in h, kind
        assert (sg.SEARCHES[kind].domain is None) == (kind == "periodogram") and sg.SEARCHES[kind].dips == (kd.columns == 1)
    # every source that forms a trial column includes the one statement of the columns, and no other file defines a rule
    csrc = os.path.join(ROOT, "celerite2_amd", "csrc")
    for src in ("c2_periodogram.hip", "c2_transit.hip", "c2_kepler.hip", "c2_shapes.hip", "c2_trial_sweep.hpp", "c2_trial_project.hip"):
        assert '#include "c2_trial_columns.hpp"' in open(os.path.join(csrc, src)).read(), src
    rule = re.compile(r"\bcolumns\s*\(double t\b|struct (Sinusoid|Transit|Keplerian|Shape|Fold)\b|\b(danby|mean_anomaly|phase)\s*\(double\b")
    for src in sorted(os.listdir(csrc)):
        found = rule.search(open(os.path.join(csrc, src)).read())
        assert (found is not None) == (src == "c2_trial_columns.hpp"), (src, found)
    assert not os.path.exists(os.path.join(csrc, "c2_shape_column.hpp")) and not os.path.exists(os.path.join(csrc, "c2_shape_project.hip"))


def test_bad_projection_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_trial_projections(*tp_args()[:-1])
    with pytest.raises(refused):
        lib.c2_trial_projections(*tp_args(), None)
    with pytest.raises(refused):
        lib.c2_trial_projections(*tp_args(B=1.0))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_trial_projections(*tp_args(p=text))


def test_projection_argument_errors(lib):
    """Sizes, null pointers, an unknown kind and 2^31 blocks are refused before anything is launched: no device is needed."""
    from celerite2_amd import _lib, ops

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    for bad in (dict(B=0), dict(N=0), dict(K=0), dict(R=0), dict(N=-1), dict(K=-3), dict(kind=3), dict(kind=-1)):
        assert lib.c2_trial_projections(*tp_args(p=p, P=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_trial_projections(*tp_args(p=p, P=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_trial_projections(*tp_args(p=None, P=p)) == _lib.C2_ERR_INVALID
    for i in (6, 8):
        neg = tp_args(p=p, P=p)
        neg[i] = -3
        assert lib.c2_trial_projections(*neg) == _lib.C2_ERR_INVALID
    for kind in R.KINDS:
        code, _, _, RB = ops.TRIAL_KINDS[kind]
        assert lib.c2_trial_projections(*tp_args(kind=code, B=2 ** 31, K=16, R=RB, p=p, P=p)) == _lib.C2_ERR_UNSUPPORTED
        assert lib.c2_trial_projections(*tp_args(kind=code, B=2 ** 11, K=16 * 2 ** 10, R=RB * 2 ** 10, p=p, P=p)) == _lib.C2_ERR_UNSUPPORTED
        assert lib.c2_trial_projections(*tp_args(kind=code, B=1, K=16 * 2 ** 31, R=1, p=p, P=p)) == _lib.C2_ERR_UNSUPPORTED


def test_python_argument_errors():
    """ops.trial_projections and gp.search_significance raise ValueError before C is entered."""
    import types

    from celerite2_amd import gp as G, ops

    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(ValueError, match="kind"):
        ops.trial_projections("bls", z(5), z(2, 5, 3), z(6, 4))
    with pytest.raises(ValueError, match=r"^Invalid shape: alpha "):
        ops.trial_projections("transit", z(5), z(5, 3), z(6, 4))
    for kind, bad in (("periodogram", z(6, 1, 1)), ("transit", z(6, 3)), ("keplerian", z(6, 4)), ("keplerian", z(18))):
        with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
            ops.trial_projections(kind, z(5), z(2, 5, 3), bad)
    with pytest.raises(ValueError, match="GPU"):
        ops.trial_projections("keplerian", z(5), z(2, 5, 3), z(6, 3))
    dims = dict(B=2, N=5, R=3, K=6, F=3, C=2)
    ops._shapes(dims, [("alpha", z(2, 5, 3), "BNR"), ("trials", z(2, 6, 3), "KF|BKF"), ("out", z(2, 6, 2, 3), "BKCR")])
    with pytest.raises(ValueError, match=r"^Invalid shape: out "):
        ops._shapes(dims, [("out", z(2, 6, 3, 2), "BKCR")])
    gp = types.SimpleNamespace(_need=lambda: None, _check_vector=lambda y: None, _diag=z(2, 5), mean=0.0, _t=z(5))
    call = lambda *a, **k: G.GaussianProcess.search_significance(gp, *a, **k)
    with pytest.raises(ValueError, match="kind"):
        call("bls", z(2, 5), z(6, 4))
    with pytest.raises(ValueError, match="normalization"):
        call("transit", z(2, 5), z(6, 4), normalization="psd")
    for kind, bad in (("periodogram", z(3, 6)), ("periodogram", z(0)), ("transit", z(6, 3)), ("keplerian", z(3, 6, 3)),
                      ("keplerian", z(0, 3)), ("transit", [[1.0, 0.0, 0.1, 0.0]])):
        with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
            call(kind, z(2, 5), bad)
    with pytest.raises(ValueError, match=r"^Invalid shape: normals "):
        call("keplerian", z(2, 5), z(6, 3), normals=z(2, 4, 7))
    with pytest.raises(ValueError, match="draws"):
        call("keplerian", z(2, 5), z(6, 3), draws=0)
    with pytest.raises(ValueError, match="max_trials"):
        call("keplerian", z(2, 5), z(6, 3), max_trials=0)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst, %s: %.3g" % (k, WORST[k]))
