# -*- coding: utf-8 -*-
"""The tabulated-shape search under correlated noise on the CPU: the numpy restatement of the column rule and of the sweep
(tests/shapes_ref.py, what trial::Shape of csrc/c2_trial_columns.hpp and csrc/c2_shapes.hip implement) against dense algebra with the column
built another way, against the transit restatement where the two rules must coincide (bit for bit for the box), the torch
finish and the builders (celerite2_amd/shapes.py), an injected limb-darkened transit, and the binding of the seventh public
header (include/celerite2_amd_shapes.h), which needs no device.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import ctypes
import re

import numpy as np
import pytest
import torch

import shapes_ref as R
import transit_ref as TR

SWEEP_ARGS = ("t", "c", "U", "W", "d", "Z0", "trials", "shapes")
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


def finish_of(D, T, **kw):
    from celerite2_amd import shapes as sh

    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    return sh.finish(S0, torch.from_numpy(np.asarray(T))[None], len(D["t"]), trials=torch.from_numpy(D["trials"]),
                     n_shapes=D["shapes"].shape[0], **kw)


@pytest.mark.parametrize("J", [1, 3, 8])
def test_restatement_against_dense(J):
    """T from the restated sweep, single-series and batched, against b^T K^-1 [b | Y0] from np.linalg.solve on the dense
    matrix with the columns built the independent way (np.interp on an extended-precision fold): every length x P0, folded
    and single events lane by lane, three asymmetric shapes, times offset by 2.45e6; every edge and fold a margin away from
    the samples (midpoint edges), so the two constructions cannot disagree on a decision."""
    for i, N in enumerate((1, 2, 5, 17, 150)):
        for P0 in (0, 1, 3):
            D = R.case(100 * J + 10 * i + P0, N, J, P0, shift=2.45e6, S=(9, 2, 65)[(i + P0) % 3])
            assert float(D["trials"][:, 1].min()) > 2.4e6 and set(D["trials"][:, 3]) == {0.0, 1.0, 2.0}
            if N >= 17:
                n_in, n_out = R.counts(D["t"], D["trials"])
                assert n_in.min() >= 2 and n_out.min() >= 2
            K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
            want = R.dense_products(K, D["t"], D["Y0"], D["trials"], D["shapes"])
            args = [D[x] for x in SWEEP_ARGS]
            got = R.whitened_shapes(*args)
            assert got.shape == (65, 2 + P0)
            check("restatement vs dense", got, want, (J, N, P0))
            gotb = R.whitened_shapes_batched(*[np.stack([a, a]) for a in args[:-1]], args[-1])
            assert np.array_equal(gotb[0], gotb[1])
            check("batched vs single restatement", gotb[0], got, (J, N, P0))
            gotp = R.whitened_shapes_batched(*[np.stack([a, a]) for a in args])          # a per-series bank
            assert np.array_equal(gotp, gotb)


def test_column_rule_against_independent():
    """The rule against the independent construction on the columns themselves: the same zeros, values within the error of
    the times over the node spacing; the left / right orientation on a ramp shape; the rule's explicit edge cases."""
    for seed, N in enumerate((9, 33, 150)):
        t = R.draw(seed, N, 2)["t"]
        for shift in (0.0, 2.45e6):
            ts = t + shift
            for S in (2, 3, 65):
                bank = R.bank(3, S, seed)
                trials = R.trials_for(ts, 65, 3, seed=seed)
                b, bo = R.column(ts, trials, bank), R.column_independent(ts, trials, bank)
                assert b.shape == (N, 65) and np.array_equal(b == 0.0, bo == 0.0)
                # (g = v (S - 1) / w with v a difference of times: its absolute error is that of the times, times (S - 1) / w;
                # a profile with values in [0, 1] and node differences up to 1 turns that into the same error of b)
                tol = 8.0 * np.spacing(np.abs(ts).max()) * (S - 1) / trials[:, 2] + 8 * np.finfo(float).eps
                assert np.all(np.abs(b - bo) <= tol[None, :])
    ramp = np.array([[0.0, 0.25, 0.5, 0.75, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0]])      # shape 0 rises from the leading edge
    one = lambda tn, *trial: float(R.column(np.array([tn]), np.array([trial]), ramp)[0, 0])
    assert one(-1.0, 0.0, 0.0, 2.0, 0.0) == 0.0 and one(1.0, 0.0, 0.0, 2.0, 0.0) == 1.0     # the two (closed) edges
    assert one(-0.5, 0.0, 0.0, 2.0, 0.0) == 0.25 and one(0.5, 0.0, 0.0, 2.0, 0.0) == 0.75    # on nodes 1 and 3
    assert one(0.25, 0.0, 0.0, 2.0, 0.0) == 0.625                                           # between nodes 2 and 3
    assert one(np.nextafter(1.0, 2.0), 0.0, 0.0, 2.0, 0.0) == 0.0 and one(np.nextafter(-1.0, -2.0), 0.0, 0.0, 2.0, 0.0) == 0.0
    assert one(7.25, 0.0, 0.25, 1.0, 0.0) == 0.0 and one(7.25, 1.0, 0.25, 1.0, 0.0) == 0.5    # P == 0: no fold; P = 1: phi = 0
    assert one(7.5, 1.0, 0.0, 1.0, 0.0) == 0.0 and one(6.5, 1.0, 0.0, 1.0, 0.0) == 1.0        # w = P: x / P ties to even (8, 6), phi = -+ P / 2
    assert one(2.45e6 + 3.25, 1.5, 2.45e6 + 0.25, 0.5, 0.0) == 0.5                            # x = 3 exactly: two periods on
    # the index is clamped, never trusted: -1, NS, NaN read shape 0; 0.5 truncates to 0; 1 is shape 1
    for s in (-1.0, 2.0, np.nan, 0.5):
        assert one(0.25, 0.0, 0.0, 2.0, s) == 0.625, s
    assert one(0.25, 0.0, 0.0, 2.0, 1.0) == 1.0
    # NaN or zero widths and NaN epochs are evaluated as written and stay inside the bank
    for trial in ((0.0, 0.0, np.nan, 0.0), (0.0, np.nan, 2.0, 0.0), (np.nan, 0.0, 2.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, -2.0, 0.0)):
        R.column(np.array([-1.0, 0.0, 0.3]), np.array([trial]), ramp)


def test_box_is_the_transit_box_bit_for_bit():
    """With the all-ones S = 2 bank the rule is transit_ref's box (tau = 0) BIT FOR BIT -- the lines up to u are the same --
    including samples placed exactly on both edges and on a fold, w = P, and single events; so is the sweep."""
    ones = np.ones((1, 2))
    t = np.arange(64) * 0.125                                                     # exact arithmetic: samples ON the edges
    tr = np.array([[2.0, 1.0, 0.5, 0.0], [2.0, 1.0, 2.0, 0.0], [0.0, 3.0, 1.0, 0.0], [1.0, 0.5, 0.25, 0.0], [3.0, 0.125, 1.0, 0.0],
                   [0.0, 100.0, 1.0, 0.0], [4.0, 0.0, 4.0, 0.0]])
    b, bo = R.column(t, tr, ones), TR.template(t, tr)
    assert np.array_equal(b, bo)
    x = t[:, None] - tr[None, :, 1]
    assert np.any((np.abs(x[:, 2]) == 0.5) & (b[:, 2] == 1.0))                     # a single event's two edges, closed
    assert np.any(x[:, 2] == 0.5) and np.any(x[:, 2] == -0.5)
    assert np.any(np.abs(x[:, 0] - 2.0 * np.rint(x[:, 0] / 2.0)) == 1.0)             # a sample on the fold of P = 2
    assert np.all(b[:, 1] == 1.0) and np.all(b[:, 6] == 1.0) and np.all(b[:, 5] == 0.0)   # w = P covers everything
    for seed, N in enumerate((17, 150)):
        D = TR.case(seed, N, 3, 1, kinds=("fold-box", "single-box"))
        for shift in (0.0, 2.45e6):
            ts = D["t"] + shift
            trials = TR.trials_for(ts, 65, kinds=("fold-box", "single-box"), seed=seed)
            assert np.array_equal(R.column(ts, trials, ones), TR.template(ts, trials))
        args = [D[x] for x in ("t", "c", "U", "W", "d", "Z0", "trials")]
        assert np.array_equal(R.whitened_shapes(*args, ones), TR.whitened_transits(*args))


def test_significance_with_a_box_bank_is_the_transit_branch_bit_for_bit(monkeypatch):
    """gp.shape_search_significance with the all-ones S = 2 bank (shapes.box()) and gp.search_significance("transit", ...) on
    the same tau = 0 trials and the same normals give the same bits -- statistic, fap and null_maxima, NaN positions
    included -- at every normalization, with and without dips_only, in blocks of trials and draws as well: one loop serves
    both.  On CPU tensors: the ops are replaced by the restatements (the two columns by R.column and TR.template, which the
    test above holds equal; one contraction for both projections, so that no summation order stands between them)."""
    import types

    import trial_projections_ref as PJ
    from celerite2_amd import gp as G, ops, shapes as sh

    B, N, J = 2, 40, 3
    Ds = [TR.case(7 + b, N, J, 1, K=29, kinds=("fold-box", "single-box")) for b in range(B)]
    t = Ds[0]["t"]
    for D in Ds[1:]:                                                              # (one time axis: the trials are shared)
        D["t"] = t
        D["d"], D["W"] = R.factor(t, D["c"], D["a"], D["U"], D["V"])
    trials = np.concatenate([Ds[0]["trials"], [[1.0, 0.5, 2.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 1.0, 0.5, 0.0]]])   # three outside
    assert np.all(trials[:, 3] == 0.0)
    tn = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    stack = lambda k: tn(np.stack([D[k] for D in Ds]))
    npy = lambda x: x.numpy()
    Ls = [PJ.lower(t, D["c"], D["U"], D["W"]) for D in Ds]
    per_series = lambda f, *xs: tn(np.stack([f(b, *[npy(x)[b] for x in xs]) for b in range(B)]))

    def project(col, alpha):                                                       # col (N, K), alpha (N, R) -> (K, 1, R)
        return np.einsum("nk,nr->kr", col.astype(np.longdouble), alpha.astype(np.longdouble)).astype(float)[:, None, :]

    sweep_args = lambda b, Z0: (t, Ds[b]["c"], Ds[b]["U"], Ds[b]["W"], Ds[b]["d"], Z0)
    monkeypatch.setattr(ops, "solve_lower", lambda t_, c, U, W, Y: per_series(lambda b, y: np.linalg.solve(Ls[b], y), Y))
    monkeypatch.setattr(ops, "solve_upper", lambda t_, c, U, W, Y: per_series(lambda b, y: np.linalg.solve(Ls[b].T, y), Y))
    monkeypatch.setattr(ops, "whitened_transits",
                        lambda t_, c, U, W, d, Z0, tr: per_series(lambda b, z: TR.whitened_transits(*sweep_args(b, z), npy(tr)), Z0))
    monkeypatch.setattr(ops, "whitened_shapes",
                        lambda t_, c, U, W, d, Z0, tr, bank: per_series(lambda b, z: R.whitened_shapes(*sweep_args(b, z), npy(tr), npy(bank)), Z0))
    monkeypatch.setattr(ops, "trial_projections",
                        lambda kind, t_, alpha, tr, t_ref=0.0: per_series(lambda b, a: project(TR.template(t, npy(tr)), a), alpha))
    monkeypatch.setattr(ops, "shape_projections",
                        lambda t_, alpha, tr, bank: per_series(lambda b, a: project(R.column(t, npy(tr), npy(bank)), a), alpha))

    gp = types.SimpleNamespace(_need=lambda: None, _check_vector=lambda y: None, mean=0.0, _t=tn(t), _c=stack("c"), _U=stack("U"),
                               _W=stack("W"), _d=stack("d"), _diag=torch.ones((B, N), dtype=torch.float64),
                               _flag=torch.zeros(B, dtype=torch.int32))
    for name in ("_whitened_columns", "_nan_failed", "_shape_args"):
        setattr(gp, name, getattr(G.GaussianProcess, name).__get__(gp))
    y, normals = stack("y"), torch.from_numpy(np.random.default_rng(3).normal(size=(B, N, 12)))
    trials, bank = tn(trials), sh.stack(sh.box())
    assert tuple(bank.shape) == (1, 2) and bool((bank == 1.0).all())
    zeroed = 0
    for nm in ("standard", "chi2", "log_likelihood"):
        for dips in (False, True):
            for blocks in (dict(), dict(max_trials=10, max_draws=5)):
                kw = dict(normalization=nm, dips_only=dips, normals=normals, **blocks)
                a = G.GaussianProcess.search_significance(gp, "transit", y, trials, **kw)
                b = G.GaussianProcess.shape_search_significance(gp, y, trials, bank, **kw)
                for x, xo, what in zip(a, b, a._fields):
                    assert x.shape == xo.shape and np.array_equal(npy(x), npy(xo), equal_nan=True), (nm, dips, blocks, what)
                assert bool(torch.isnan(a.statistic[:, -3:]).all()) and bool(torch.isfinite(a.statistic[:, :-3]).all())
                assert bool(torch.isfinite(a.null_maxima).all()) and bool(((a.fap[:, :-3] > 0) & (a.fap[:, :-3] <= 1)).all())
                zeroed += int((a.statistic == 0).sum()) if dips else 0
                assert dips or not bool((a.statistic == 0).any())
    assert zeroed > 0                                                              # (dips_only did change something)


def test_trapezoid_bank_meets_the_transit_trapezoid():
    """A trapezoid bank with its corners on nodes against transit_ref's trapezoid (tau = ingress w): columns and products."""
    from celerite2_amd import shapes as sh

    for ingress, S in ((0.25, 9), (0.5, 3), (0.125, 65), (0.375, 9)):
        bank = sh.stack(sh.trapezoid(ingress, S)).numpy()
        D = TR.case(int(100 * ingress) + S, 150, 3, 1, kinds=("fold-box", "single-box"))
        D["trials"][:, 3] = ingress * D["trials"][:, 2]
        bo = TR.template(D["t"], D["trials"])
        assert np.any((bo > 0) & (bo < 1))
        tri = D["trials"].copy()
        tri[:, 3] = 0.0
        b = R.column(D["t"], tri, bank)
        check("trapezoid bank vs transit trapezoid, column", b, bo, (ingress, S))
        args = [D[x] for x in ("t", "c", "U", "W", "d", "Z0")]
        check("trapezoid bank vs transit trapezoid, T", R.whitened_shapes(*args, tri, bank), TR.whitened_transits(*args, D["trials"]),
              (ingress, S))
    with pytest.raises(ValueError, match="not an integer"):
        sh.trapezoid(0.3, 9)
    with pytest.raises(ValueError):
        sh.trapezoid(0.6, 11)


@pytest.mark.parametrize("N,J,P0", [(150, 8, 1), (33, 3, 1), (17, 1, 0), (60, 4, 3)])
def test_finish_against_dense(N, J, P0):
    """The torch finish on the restated products against two dense generalized-least-squares fits per trial ([A0] and
    [A0 | b_k], the column built the independent way)."""
    D = R.case(7 * N + J + P0, N, J, P0, S=17)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, amp, aerr, chi2_0 = R.dense_search(K, D["t"], D["A0"], D["y"], D["trials"], D["shapes"])
    fit = finish_of(D, R.whitened_shapes(*[D[x] for x in SWEEP_ARGS]))
    assert type(fit).__name__ == "ShapeSearch" and fit._fields == ("delta_chi2", "amplitude", "amplitude_err", "snr", "chi2_null")
    assert all(tuple(x.shape) == (1, 65) for x in fit[:4]) and tuple(fit.chi2_null.shape) == (1,)
    what = (N, J, P0)
    check("finish delta_chi2 vs dense", fit.delta_chi2[0].numpy(), dchi2, what)
    check("finish amplitude vs dense", fit.amplitude[0].numpy(), amp, what)
    check("finish amplitude_err vs dense", fit.amplitude_err[0].numpy(), aerr, what)
    check("finish snr vs dense", fit.snr[0].numpy(), amp / aerr, what)
    check("finish chi2_null vs dense", fit.chi2_null.numpy(), [chi2_0], what)


def test_in_domain_and_nan_rules():
    """in_domain, case by case, and finish's mask: each trial outside the domain holds NaN and leaves its neighbours their
    bits; without `trials` nothing is masked."""
    from celerite2_amd import shapes as sh

    nan, inf = float("nan"), float("inf")
    rows = {"good fold": (2.0, 0.3, 0.5, 1.0), "good single": (0.0, 0.3, 0.5, 2.0), "w = P": (2.0, 0.3, 2.0, 0.0),
            "w == 0": (2.0, 0.3, 0.0, 0.0), "w < 0": (2.0, 0.3, -0.5, 0.0), "w > P": (0.4, 0.3, 0.5, 0.0), "P < 0": (-2.0, 0.3, 0.5, 0.0),
            "P NaN": (nan, 0.3, 0.5, 0.0), "t0 NaN": (2.0, nan, 0.5, 0.0), "w NaN": (2.0, 0.3, nan, 0.0), "w inf": (0.0, 0.3, inf, 0.0),
            "s = 0.5": (2.0, 0.3, 0.5, 0.5), "s = -1": (2.0, 0.3, 0.5, -1.0), "s = NS": (2.0, 0.3, 0.5, 3.0), "s NaN": (2.0, 0.3, 0.5, nan)}
    got = sh.in_domain(torch.tensor(list(rows.values()), dtype=torch.float64), 3)
    assert got.tolist() == [name in ("good fold", "good single", "w = P") for name in rows], got.tolist()
    assert sh.in_domain(torch.zeros(2, 5, 4, dtype=torch.float64), 1).shape == (2, 5)
    D = R.case(5, 33, 3, 2)
    args = [D[x] for x in ("t", "c", "U", "W", "d", "Z0")]
    good = finish_of(D, R.whitened_shapes(*args, D["trials"], D["shapes"]))
    assert all(bool(torch.isfinite(x).all()) for x in good)
    base = D["trials"][4].copy()
    for name, s in (("s = 0.5", 0.5), ("s = -1", -1.0), ("s = NS", 3.0), ("s NaN", nan)):
        E = dict(D, trials=D["trials"].copy())
        E["trials"][7] = (base[0], base[1], base[2], s)
        T = R.whitened_shapes(*args, E["trials"], D["shapes"])
        assert np.all(np.isfinite(T)), name                              # clamped to shape 0: a value, not a read elsewhere
        got = finish_of(E, T)
        for x, xo in zip(got[:4], good[:4]):
            assert bool(torch.isnan(x[0, 7])), name
            keep = np.arange(65) != 7
            assert np.array_equal(x[0].numpy()[keep], xo[0].numpy()[keep]), name
        assert torch.equal(got.chi2_null, good.chi2_null)
        free = sh.finish(torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None], torch.from_numpy(T)[None], 33)
        assert bool(torch.isfinite(free.delta_chi2).all())
    with pytest.raises(ValueError, match="n_shapes"):
        sh.finish(torch.zeros(1, 2, 2), torch.zeros(1, 3, 3), 5, trials=torch.zeros(3, 4))
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        sh.finish(torch.eye(2, dtype=torch.float64)[None], torch.ones(1, 3, 3, dtype=torch.float64), 5,
                  trials=torch.zeros(2, 4, dtype=torch.float64), n_shapes=1)


def test_trial_grid():
    from celerite2_amd import shapes as sh

    g = sh.trial_grid([2.0, 3.0], [0.5, 0.25, 2.5], phase_step=0.5, t0=10.0, shape=2)
    assert g.dtype == torch.float64 and g.shape[1] == 4
    assert g.shape[0] == 8 + 16 + 12 + 24 + 3           # epochs per (P, w): ceil(P / (0.5 w)); w = 2.5 exceeds P = 2
    assert bool(sh.in_domain(g, 3).all()) and not bool(sh.in_domain(g, 2).any())
    first = g[:8]
    assert torch.equal(first[:, 0], torch.full((8,), 2.0, dtype=torch.float64)) and torch.equal(first[:, 2], torch.full((8,), 0.5, dtype=torch.float64))
    assert torch.equal(first[:, 1], 10.0 + 0.25 * torch.arange(8, dtype=torch.float64))
    assert torch.equal(g[:, 3], torch.full((g.shape[0],), 2.0, dtype=torch.float64))
    assert sh.trial_grid(torch.tensor([1.0]), torch.tensor([0.5])).shape == (8, 4)
    for bad in (dict(phase_step=0.0), dict(shape=-1), dict(shape=0.5)):
        with pytest.raises(ValueError):
            sh.trial_grid([1.0], [0.1], **bad)
    with pytest.raises(ValueError):
        sh.trial_grid([0.0], [0.1])


def lens_area(z, k):
    """The area two circles of radii 1 and k share at centre distance z (closed form)."""
    z = np.asarray(z, dtype=float)
    out = np.where(z <= 1.0 - k, np.pi * k * k, 0.0)
    m = (z > 1.0 - k) & (z < 1.0 + k)
    zz = z[m]
    out[m] = (k * k * np.arccos((zz * zz + k * k - 1.0) / (2.0 * zz * k)) + np.arccos((zz * zz + 1.0 - k * k) / (2.0 * zz))
              - 0.5 * np.sqrt((-zz + k + 1.0) * (zz + k - 1.0) * (zz - k + 1.0) * (zz + k + 1.0)))
    return out


# max |limb_darkened(0.2, 0.3, 0, 0, 65, quad=64) - limb_darkened(..., quad=128)| as measured on the CPU: 2.3284e-3 (the
# midpoint rule loses the cells the stellar limb cuts).  The tolerance against the closed form is four times that.
QUAD_DIFFERENCE = 2.3284e-3


def test_builders():
    from celerite2_amd import shapes as sh

    k, b = 0.2, 0.3
    uni, fine = sh.limb_darkened(k, b, 0.0, 0.0), sh.limb_darkened(k, b, 0.0, 0.0, quad=128)
    diff = float((uni - fine).abs().max())
    assert 0.5 * QUAD_DIFFERENCE <= diff <= 1.0001 * QUAD_DIFFERENCE, diff
    x = np.linspace(-1.0, 1.0, 65) * np.sqrt((1.0 + k) ** 2 - b * b)
    area = lens_area(np.sqrt(x * x + b * b), k)
    worst = float(np.abs(uni.numpy() - area / area.max()).max())
    print("limb_darkened(u = 0) vs the lens area: %.3e (tolerance %.3e)" % (worst, 4.0 * QUAD_DIFFERENCE))
    assert worst <= 4.0 * QUAD_DIFFERENCE
    ld = sh.limb_darkened(0.1, 0.3, 0.4, 0.3)
    assert ld.shape == (65,) and ld.dtype == torch.float64 and float(ld[0]) == 0.0 and float(ld[-1]) == 0.0
    assert torch.allclose(ld, ld.flip(0), atol=1e-12) and bool((ld[1:33] > ld[:32]).all())      # symmetric, rising to mid-transit
    flat = sh.limb_darkened(0.1, 0.3, 0.0, 0.0)
    assert float(ld[16]) < float(flat[16]) and abs(float(ld[16]) - float(flat[16])) > 0.01   # darkened: rounder shoulders
    fl = sh.flare(0.125, 0.3)
    assert float(fl[0]) == 0.0 and float(fl[8]) == 1.0 and int(fl.argmax()) == 8
    assert np.allclose(fl[8:].numpy(), np.exp(-(np.arange(8, 65) / 64.0 - 0.125) / 0.3), rtol=1e-15)
    assert np.array_equal(fl[:9].numpy(), np.arange(9) / 8.0)
    assert float(sh.flare(0.0, 0.5)[0]) == 1.0
    tz = sh.trapezoid(0.25, 9)
    assert tz.tolist() == [0.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.0]
    assert sh.trapezoid(0.5, 3).tolist() == [0.0, 1.0, 0.0]
    assert sh.box().tolist() == [1.0, 1.0] and sh.box(5).tolist() == [1.0] * 5
    for s in (sh.box(), sh.box(7), tz, sh.trapezoid(0.5, 3), ld, uni, flat, fl, sh.flare(0.1, 0.3, 10), sh.flare(0.0, 0.5, 4)):
        assert s.dim() == 1 and s.dtype == torch.float64 and float(s.max()) == 1.0 and float(s.min()) >= 0.0
    bank = sh.stack(ld, fl, sh.box(65))
    assert tuple(bank.shape) == (3, 65) and torch.equal(bank[1], fl)
    for bad in (lambda: sh.stack(), lambda: sh.stack(sh.box(), sh.box(3)), lambda: sh.box(1), lambda: sh.flare(1.0, 0.3),
                lambda: sh.flare(0.1, 0.0), lambda: sh.limb_darkened(0.1, 1.2, 0.0, 0.0), lambda: sh.limb_darkened(0.0, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            bad()


INGRESS = (0.0625, 0.125, 0.1875, 0.25, 0.3125, 0.375, 0.4375, 0.5)     # the trapezoids of S = 65 tried against the true shape


def test_injected_limb_darkened_transit():
    """A folded limb-darkened transit added to a low-noise draw, so that template mismatch dominates: searched with a bank
    of [the limb-darkened shape, the box, eight trapezoids], the highest delta_chi2 of the whole grid falls on the injected
    (P, t0, w) with the limb-darkened shape, and there it exceeds the box's and the best trapezoid's.  The margins were
    confirmed with the dense algebra (below) for this seed before they were fixed: delta_chi2 of the box / limb-darkened
    = 0.4074 (a box from first to fourth contact), of the best trapezoid / limb-darkened = 0.9648."""
    from celerite2_amd import shapes as sh

    S, depth = 65, -1.0
    bank = sh.stack(sh.limb_darkened(0.1, 0.3, 0.5, 0.2, S), sh.box(S), *[sh.trapezoid(g, S) for g in INGRESS]).numpy()
    NS = bank.shape[0]
    D = R.case(42, 150, 3, 1)
    t = D["t"]
    span = t[-1] - t[0]
    periods, widths = [span / 4.3, span / 3.1], [0.04 * span, 0.06 * span]
    nodes = sh.trial_grid(periods, widths, phase_step=0.5, t0=float(t[0])).numpy()
    true = int(np.flatnonzero((nodes[:, 0] == periods[1]) & (nodes[:, 2] == widths[1]))[5])
    trials = np.repeat(nodes, NS, axis=0)
    trials[:, 3] = np.tile(np.arange(NS), len(nodes))
    assert bool(sh.in_domain(torch.from_numpy(trials), NS).all())
    y = 0.02 * D["y"] + depth * R.column(t, nodes[true:true + 1], bank)[:, 0]
    assert (R.column(t, nodes[true:true + 1], bank)[:, 0] > 0).sum() >= 8
    D.update(trials=trials, shapes=bank)
    D["Z0"] = R.sweep(t, D["c"], D["U"], D["W"], np.concatenate([D["A0"], y[:, None]], axis=1))[0]
    d = D["d"] * 0.02 ** 2                                               # (the noise scaled with the draw: K -> 0.02^2 K)
    fit = finish_of(dict(D, d=d), R.whitened_shapes(t, D["c"], D["U"], D["W"], d, D["Z0"], trials, bank))
    dchi2 = fit.delta_chi2[0].numpy().reshape(len(nodes), NS)
    assert np.all(np.isfinite(dchi2[true]))
    assert np.unravel_index(np.nanargmax(dchi2), dchi2.shape) == (true, 0)
    box_ratio, trap_ratio = dchi2[true, 1] / dchi2[true, 0], dchi2[true, 2:].max() / dchi2[true, 0]
    print("delta_chi2 at the injected node: box / limb-darkened %.4f, best trapezoid / limb-darkened %.4f" % (box_ratio, trap_ratio))
    assert box_ratio < 0.5 and trap_ratio < 0.98
    assert abs(float(fit.amplitude[0, true * NS]) - depth) <= 3.0 * float(fit.amplitude_err[0, true * NS])
    K = 0.02 ** 2 * R.dense(t, D["c"], D["a"], D["U"], D["V"])
    want = R.dense_search(K, t, D["A0"], y, trials[true * NS:(true + 1) * NS], bank)
    check("injected: delta_chi2 at the node vs dense", dchi2[true], want[0])
    assert want[0][1] / want[0][0] < 0.5 and want[0][2:].max() / want[0][0] < 0.98


# ---- the binding of the seventh header ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def sh_args(B=1, N=4, J=2, Q0=1, K=3, NS=1, S=2, p=None, T=None, sh_bs=0):
    return [B, N, J, Q0, K, p, 0, p, 0, p, p, p, p, p, 0, T, p, sh_bs, NS, S, None]


def pr_args(B=1, N=4, K=3, R=2, NS=1, S=2, p=None, P=None, sh_bs=0):
    return [B, N, K, R, p, 0, p, 0, p, P, p, sh_bs, NS, S, None]


def test_shapes_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib, ops

    text = open(_lib.header_path("shapes")).read()
    for name, count in (("c2_whitened_shapes", 21), ("c2_shape_projections", 15)):
        fn = getattr(lib, name)
        assert len(fn.argtypes) == count and fn.restype is ctypes.c_int, name
        assert fn.argtypes[-1] is _lib.Pointer and fn.argtypes[-5] is _lib.Pointer and fn.argtypes[-4:-1] == (ctypes.c_int64,) * 3
    defines = dict(re.findall(r"^#define\s+(C2_SHAPE_\w+)\s+(\d+)\s*$", text, flags=re.M))
    assert int(defines["C2_SHAPE_MAX_NODES"]) == ops.SHAPE_MAX_NODES == 1024
    assert int(defines["C2_SHAPE_DRAWS"]) == ops.SHAPE_DRAWS and ops.SHAPE_DRAWS % 16 == 0


def test_shape_argument_errors(lib):
    """Sizes, null pointers, a bank stride that is neither 0 nor NS S, J = 33, Q0 = 9 and NS S = 1025 are refused before
    anything is launched: no device is needed."""
    from celerite2_amd import _lib

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    for bad in (dict(B=0), dict(N=0), dict(J=0), dict(Q0=0), dict(K=0), dict(NS=0), dict(S=1), dict(S=0), dict(N=-1), dict(sh_bs=3),
                dict(sh_bs=-2)):
        assert lib.c2_whitened_shapes(*sh_args(p=p, T=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_whitened_shapes(*sh_args(p=p, T=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_shapes(*sh_args(p=None, T=p)) == _lib.C2_ERR_INVALID
    for big in (dict(J=33), dict(Q0=9), dict(NS=1, S=1025), dict(NS=5, S=205), dict(NS=1025, S=2), dict(NS=2 ** 40, S=2 ** 40),
                dict(B=2 ** 31, K=64)):
        assert lib.c2_whitened_shapes(*sh_args(p=p, T=p, **big)) == _lib.C2_ERR_UNSUPPORTED, big
    for bad in (dict(B=0), dict(N=0), dict(K=0), dict(R=0), dict(NS=0), dict(S=1), dict(sh_bs=3)):
        assert lib.c2_shape_projections(*pr_args(p=p, P=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_shape_projections(*pr_args(p=p, P=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_shape_projections(*pr_args(p=None, P=p)) == _lib.C2_ERR_INVALID
    for big in (dict(NS=1, S=1025), dict(NS=513, S=2), dict(B=2 ** 31, K=16)):
        assert lib.c2_shape_projections(*pr_args(p=p, P=p, **big)) == _lib.C2_ERR_UNSUPPORTED, big
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_whitened_shapes(*sh_args()[:-1])
    with pytest.raises(refused):
        lib.c2_shape_projections(*pr_args(), None)


def test_python_argument_errors():
    """ops.whitened_shapes, ops.shape_projections and the two front ends raise ValueError before C is entered; the bank's
    limits are named (NS * S <= 1024), not reported as a width."""
    import types
    from celerite2_amd import gp as G, ops

    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    ins = [z(5), z(2), z(2, 5, 2), z(2, 5, 2), z(2, 5), z(2, 5, 3)]
    with pytest.raises(ValueError, match="GPU"):
        ops.whitened_shapes(*ins, z(6, 4), z(3, 9))
    with pytest.raises(ValueError, match="GPU"):
        ops.whitened_shapes(*ins, z(6, 4), z(4, 256))                       # NS S = 1024: allowed
    for bank in (z(5, 205), z(1, 1025), z(2, 5, 205)):
        with pytest.raises(ValueError, match=r"NS \* S <= 1024"):
            ops.whitened_shapes(*ins, z(6, 4), bank)
        with pytest.raises(ValueError, match=r"NS \* S <= 1024"):
            ops.shape_projections(z(5), z(2, 5, 3), z(6, 4), bank)
    for bank in (z(9), z(3, 1), z(0, 9), z(3, 3, 9), z(1, 2, 3, 9)):
        with pytest.raises(ValueError, match=r"^Invalid shape: shapes "):
            ops.whitened_shapes(*ins, z(6, 4), bank)
        with pytest.raises(ValueError, match=r"^Invalid shape: shapes "):
            ops.shape_projections(z(5), z(2, 5, 3), z(6, 4), bank)
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops.whitened_shapes(*ins, z(6, 3), z(3, 9))
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops.shape_projections(z(5), z(2, 5, 3), z(24), z(3, 9))
    with pytest.raises(ValueError, match=r"^Invalid shape: alpha "):
        ops.shape_projections(z(5), z(5, 3), z(6, 4), z(3, 9))
    with pytest.raises(ValueError, match=r"^Invalid shape: Z0 "):
        ops.whitened_shapes(*ins[:5], z(5, 3), z(6, 4), z(3, 9))
    gp = types.SimpleNamespace(_need=lambda: None, _check_vector=lambda y: None, _diag=z(2, 5), mean=0.0)
    gp._shape_args = lambda trials, shapes: G.GaussianProcess._shape_args(gp, trials, shapes)
    for search in (G.GaussianProcess.shape_search, G.GaussianProcess.shape_search_significance):
        for bad in (z(6, 3), z(3, 6, 4), z(24), z(0, 4), [[1.0, 0.0, 0.1, 0.0]]):
            with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
                search(gp, z(2, 5), bad, z(3, 9))
        for bad in (z(9), z(3, 3, 9), [[1.0, 1.0]]):
            with pytest.raises(ValueError, match=r"^Invalid shape: shapes "):
                search(gp, z(2, 5), z(6, 4), bad)
    with pytest.raises(ValueError, match="normalization"):
        G.GaussianProcess.shape_search_significance(gp, z(2, 5), z(6, 4), z(3, 9), normalization="psd")


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
