# -*- coding: utf-8 -*-
"""The transit search under correlated noise on the CPU: the numpy restatement of the whitened-transit sweep
(tests/transit_ref.py, what csrc/c2_transit.hip implements) against dense algebra, the torch finish
(celerite2_amd/transit.py) on the restated products against two dense generalized-least-squares fits per trial, against
classical weighted box least squares in the white-noise limit and on an injected transit, the template rule against an
independent construction, and the binding of the fourth public header (include/celerite2_amd_transit.h), which needs no
device.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide
exactly.  Every trial set has its template edges at midpoints between neighbouring sample distances (transit_ref.trials_for),
so no sample decides differently however the template is built."""
import ctypes

import numpy as np
import pytest
import torch

import transit_ref as R

WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
LENGTHS = [1, 2, 7, 8, 9, 16, 17, 33, 150]
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


def populated(D):
    """Every trial is in the domain and has two samples in transit and two out of it: nothing is NaN by accident."""
    from celerite2_amd import transit as tr

    n_in, n_out = R.counts(D["t"], D["trials"])
    assert n_in.min() >= 2 and n_out.min() >= 2, (n_in.min(), n_out.min())
    assert bool(tr.in_domain(torch.from_numpy(D["trials"])).all())


def finish_of(D, T, **kw):
    from celerite2_amd import transit as tr

    S0 = torch.from_numpy(R.null_products(D["Z0"], D["d"]))[None]
    return tr.finish(S0, torch.from_numpy(np.asarray(T))[None], len(D["t"]), trials=torch.from_numpy(D["trials"]), **kw)


@pytest.mark.parametrize("J", WIDTHS)
def test_restatement_against_dense(J):
    """T from the restated sweep, single-series and batched, against b^T K^-1 [b | Y0] from np.linalg.solve on the dense
    matrix with the template built the independent way, on every length; boxes and trapezoids, folded and single, lane by
    lane; the nuisance columns rotate over P0 = 1, 0, 3."""
    for i, N in enumerate(LENGTHS):
        P0 = (1, 0, 3)[(i + J) % 3]
        D = R.case(100 * J + i, N, J, P0)
        if N >= 8:
            populated(D)
        K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
        want = R.dense_products(K, D["t"], D["Y0"], D["trials"])
        args = [D[x] for x in SWEEP_ARGS]
        got = R.whitened_transits(*args)
        assert got.shape == (65, 2 + P0)
        check("restatement vs dense", got, want, (J, N, P0))
        gotb = R.whitened_transits_batched(*[np.stack([a, a]) for a in args])
        assert gotb.shape == (2, 65, 2 + P0) and np.array_equal(gotb[0], gotb[1])
        check("batched restatement vs dense", gotb[0], want, (J, N, P0))
        check("batched vs single restatement", gotb[0], got, (J, N, P0))


@pytest.mark.parametrize("N,J,P0", [(150, 8, 1), (33, 3, 1), (17, 1, 0), (150, 32, 3), (60, 4, 0), (60, 4, 3)])
def test_finish_against_dense(N, J, P0):
    """The torch finish on the restated products against two dense generalized-least-squares fits per trial ([A0] and
    [A0 | b_k]): delta_chi2, the depth, its error from the fit's covariance, snr and chi2 of the null fit."""
    D = R.case(7 * N + J + P0, N, J, P0)
    populated(D)
    K = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    dchi2, depth, derr, chi2_0 = R.dense_search(K, D["t"], D["A0"], D["y"], D["trials"])
    fit = finish_of(D, R.whitened_transits(*[D[x] for x in SWEEP_ARGS]))
    assert all(tuple(x.shape) == (1, 65) for x in fit[:4]) and tuple(fit.chi2_null.shape) == (1,)
    what = (N, J, P0)
    check("finish delta_chi2 vs dense", fit.delta_chi2[0].numpy(), dchi2, what)
    check("finish depth vs dense", fit.depth[0].numpy(), depth, what)
    check("finish depth_err vs dense", fit.depth_err[0].numpy(), derr, what)
    check("finish snr vs dense", fit.snr[0].numpy(), depth / derr, what)
    check("finish chi2_null vs dense", fit.chi2_null.numpy(), [chi2_0], what)
    assert bool((fit.delta_chi2 >= 0).all())


def test_white_noise_limit():
    """U = V = 0 (so W = 0 and d = the diagonal): delta_chi2 and the depth are classical weighted box least squares with a
    floating mean, written from the in-transit weight and the weighted in-transit flux -- the one known answer that shares
    no code with the sweep."""
    rng = np.random.default_rng(3)
    N, J = 80, 2
    t = np.sort(rng.uniform(0.0, 20.0, N))
    sigma2 = rng.uniform(0.05, 0.5, N)
    trials = R.trials_for(t, 65, kinds=("fold-box", "single-box"), seed=4)
    y = 0.7 - 0.4 * R.template(t, trials[:1])[:, 0] + np.sqrt(sigma2) * rng.normal(size=N)
    D = dict(t=t, d=sigma2, Z0=np.stack([np.ones(N), y], axis=1), trials=trials)
    populated(D)
    T = R.whitened_transits(t, np.array([0.3, 1.1]), np.zeros((N, J)), np.zeros((N, J)), sigma2, D["Z0"], trials)
    fit = finish_of(D, T)
    dchi2, depth = R.classical_bls(t, y, sigma2, trials)
    check("white-noise limit vs classical, delta_chi2", fit.delta_chi2[0].numpy(), dchi2)
    check("white-noise limit vs classical, depth", fit.depth[0].numpy(), depth)


@pytest.mark.parametrize("delta", [3.0, -3.0])
def test_injected_transit(delta):
    """A folded box of depth delta added to a draw (delta < 0: a dip): the maximum of snr (the minimum, for a dip) and of
    delta_chi2 fall on the injected (P, t0, w) among trials of other periods, epochs and durations, by a margin, and the
    depth is recovered within 3 depth_err."""
    D = R.case(21, 150, 4, 1)
    t = D["t"]
    true = R.trials_for(t, 1, kinds=("fold-box",), seed=5)[0]
    others = R.trials_for(t, 64, kinds=("fold-box", "fold-trap", "single-box"), seed=6)
    D["trials"] = np.concatenate([others[:23], true[None], others[23:]])
    populated(D)
    y = D["y"] + delta * R.template(t, true[None])[:, 0]
    Y0 = np.concatenate([D["A0"], y[:, None]], axis=1)
    D["Z0"] = R.sweep(t, D["c"], D["U"], D["W"], Y0)[0]
    fit = finish_of(D, R.whitened_transits(*[D[x] for x in SWEEP_ARGS]))
    snr = fit.snr[0].numpy() * np.sign(delta)
    assert int(np.argmax(snr)) == 23 and int(torch.argmax(fit.delta_chi2[0])) == 23
    assert snr[23] > 5.0 and np.sort(np.abs(snr))[-2] < 0.8 * snr[23], np.sort(np.abs(snr))[-3:]
    assert abs(float(fit.depth[0, 23]) - delta) <= 3.0 * float(fit.depth_err[0, 23])
    K = R.dense(t, D["c"], D["a"], D["U"], D["V"])
    dchi2, depth, derr, _ = R.dense_search(K, t, D["A0"], y, D["trials"])
    check("finish delta_chi2 vs dense", fit.delta_chi2[0].numpy(), dchi2, "injected")
    check("finish depth vs dense", fit.depth[0].numpy(), depth, "injected")
    check("finish depth_err vs dense", fit.depth_err[0].numpy(), derr, "injected")


def test_template_rule():
    """The numpy rule against the np.fmod-based construction on midpoint-edge trials (the same discrete decisions; the
    ramps to rounding), on times offset by 2.45e6 with t0 at the offset, and the rule's explicit edge cases."""
    for seed, N in enumerate((9, 33, 150)):
        t = R.draw(seed, N, 2)["t"]
        for shift in (0.0, 2.45e6):
            ts = t + shift
            trials = R.trials_for(ts, 65, seed=seed)
            b, bo = R.template(ts, trials), R.template_independent(ts, trials)
            assert b.shape == (N, 65)
            assert np.array_equal(b == 0.0, bo == 0.0) and np.array_equal(b == 1.0, bo == 1.0)
            assert np.all((b >= 0.0) & (b <= 1.0)) and np.any((b > 0.0) & (b < 1.0))
            # (a ramp value is u / tau with u a difference of times: its absolute error is that of the times, over tau)
            ramp = trials[:, 3] > 0
            tol = 8.0 * np.spacing(np.abs(ts).max()) / np.where(ramp, trials[:, 3], 1.0)
            assert np.all(np.abs(b - bo) <= tol[None, :])
    one = lambda tn, *trial: float(R.template(np.array([tn]), np.array([trial]))[0, 0])
    assert one(1.0, 0.0, 0.0, 2.0, 0.5) == 0.0          # u == 0 on a ramp: 0 / tau
    assert one(1.0, 0.0, 0.0, 2.0, 0.0) == 1.0          # u == 0, tau == 0: the box is closed at its edges
    assert one(-1.0, 0.0, 0.0, 2.0, 0.0) == 1.0
    assert one(np.nextafter(1.0, 2.0), 0.0, 0.0, 2.0, 0.0) == 0.0
    assert one(0.5, 0.0, 0.0, 2.0, 0.5) == 1.0          # u == tau: the plateau is closed
    assert one(0.75, 0.0, 0.0, 2.0, 0.5) == 0.5         # half-way up the ramp
    assert one(7.25, 0.0, 0.25, 1.0, 0.0) == 0.0        # P == 0: no fold, the event at t0 only
    assert one(7.25, 1.0, 0.25, 1.0, 0.0) == 1.0        # folded at P = 1: phi = 0
    assert one(7.5, 2.0, 0.5, 1.0, 0.0) == 0.0 and one(5.5, 2.0, 0.5, 1.0, 0.0) == 0.0   # x / P = 3.5 and 2.5: ties to even, |phi| = P / 2
    assert one(2.45e6 + 3.25, 1.5, 2.45e6 + 0.25, 0.5, 0.0) == 1.0      # x = 3 exactly: two periods on
    assert one(2.45e6 + 3.25, 1.5, 2.45e6 + 0.625, 1.0, 0.25) == 0.5    # x = 2.625, q = 2, phi = -0.375: u = 0.125 on a ramp of 0.25
    # the offset changes no bit when the times stay representable: t - t0 is formed first
    t = np.arange(40) * 0.125
    trials = R.trials_for(t, 16, seed=1)
    trials[:, 1] = np.round(trials[:, 1] * 1024.0) / 1024.0      # (epochs that stay representable beside 2.45e6)
    far = trials.copy()
    far[:, 1] += 2.45e6
    assert np.array_equal(R.template(t + 2.45e6, far), R.template(t, trials))


def test_nan_rules():
    """Each degenerate case, one at a time, holds NaN and leaves its neighbours their bits: no sample in transit, a template
    in the span of A0, each way out of the domain, N < P0 + 2; a rank-deficient nuisance matrix and a series that is not `ok`
    are NaN throughout."""
    from celerite2_amd import transit as tr

    D = R.case(5, 33, 3, 2)
    populated(D)
    t, span = D["t"], D["t"][-1] - D["t"][0]
    args = [D[x] for x in ("t", "c", "U", "W", "d", "Z0")]
    good = finish_of(D, R.whitened_transits(*args, D["trials"]))
    assert all(bool(torch.isfinite(x).all()) for x in good)
    base = D["trials"][4].copy()                                       # a folded box
    assert base[0] > 0 and base[3] == 0
    cases = {"no sample in transit": (0.0, t[0] - span, 0.1 * span, 0.0),
             "all in transit beside the constant column": (0.0, t[16], 4.0 * span, 0.0),
             "w == 0": (base[0], base[1], 0.0, 0.0), "w < 0": (base[0], base[1], -base[2], 0.0),
             "tau < 0": (base[0], base[1], base[2], -0.01 * base[2]), "tau > w / 2": (base[0], base[1], base[2], 0.51 * base[2]),
             "P < 0": (-base[0], base[1], base[2], 0.0), "w > P": (0.5 * base[2], base[1], base[2], 0.0)}
    for name, trial in cases.items():
        E = dict(D, trials=D["trials"].copy())
        E["trials"][7] = trial
        T = R.whitened_transits(*args, E["trials"])
        if name == "no sample in transit":
            assert np.all(T[7] == 0.0)                                 # exact zeros, not small numbers
        got = finish_of(E, T)
        for x, xo in zip(got[:4], good[:4]):
            assert bool(torch.isnan(x[0, 7])), name
            keep = np.arange(65) != 7
            assert np.array_equal(x[0].numpy()[keep], xo[0].numpy()[keep]), name
        assert torch.equal(got.chi2_null, good.chi2_null)
    assert not bool(tr.in_domain(torch.tensor([c for n, c in cases.items() if n[0] in "wtP"])).any())
    # N < P0 + 2: two points beside a constant column leave nothing to compare
    for N, P0 in ((1, 0), (2, 1), (3, 2)):
        S = R.case(11 + N, N, 3, P0, K=7)
        fit = finish_of(S, R.whitened_transits(*[S[x] for x in SWEEP_ARGS]))
        assert all(bool(torch.isnan(x).all()) for x in fit[:4]) and bool(torch.isfinite(fit.chi2_null).all())
    # a repeated nuisance column, and a series that is not ok, between two good ones
    Y2 = D["Y0"].copy()
    Y2[:, 1] = Y2[:, 0]
    Z2 = R.sweep(D["t"], D["c"], D["U"], D["W"], Y2)[0]
    T, T2 = R.whitened_transits(*args, D["trials"]), R.whitened_transits(*args[:5], Z2, D["trials"])
    S0 = torch.from_numpy(np.stack([R.null_products(Z, D["d"]) for Z in (D["Z0"], Z2, D["Z0"], D["Z0"])]))
    TT = torch.from_numpy(np.stack([T, T2, T, T]))
    got = tr.finish(S0, TT, 33, ok=torch.tensor([True, True, False, True]), trials=torch.from_numpy(D["trials"]))
    for b in (1, 2):
        assert all(bool(torch.isnan(x[b]).all()) for x in got)
    for b in (0, 3):
        for x, xo in zip(got, good):
            assert np.array_equal(x[b].numpy(), xo[0].numpy())
    with pytest.raises(ValueError, match=r"^Invalid shape: T "):
        tr.finish(S0, TT[..., :-1], 33)
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        tr.finish(S0, TT, 33, trials=torch.from_numpy(D["trials"][:-1]))


def test_trial_grid():
    from celerite2_amd import transit as tr

    g = tr.trial_grid([2.0, 3.0], [0.5, 0.25, 2.5], phase_step=0.5, t0=10.0, ingress=0.2)
    assert g.dtype == torch.float64 and g.shape[1] == 4
    # epochs per (P, w): ceil(P / (0.5 w)); w = 2.5 exceeds P = 2 and is left out there
    assert g.shape[0] == 8 + 16 + 12 + 24 + 3
    assert bool(tr.in_domain(g).all())
    first = g[:8]
    assert torch.equal(first[:, 0], torch.full((8,), 2.0, dtype=torch.float64)) and torch.equal(first[:, 2], torch.full((8,), 0.5, dtype=torch.float64))
    assert torch.equal(first[:, 1], 10.0 + 0.25 * torch.arange(8, dtype=torch.float64))
    assert torch.allclose(first[:, 3], torch.full((8,), 0.1, dtype=torch.float64))
    assert bool((g[:, 1] < 10.0 + g[:, 0]).all())
    assert tr.trial_grid(torch.tensor([1.0]), torch.tensor([0.5])).shape == (8, 4)
    for bad in (dict(phase_step=0.0), dict(ingress=0.6), dict(ingress=-0.1)):
        with pytest.raises(ValueError):
            tr.trial_grid([1.0], [0.1], **bad)
    with pytest.raises(ValueError):
        tr.trial_grid([0.0], [0.1])


# ---- the binding of the fourth header ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


def tr_args(B=1, N=4, J=2, Q0=1, K=3, p=None, T=None):
    return [B, N, J, Q0, K, p, 0, p, 0, p, p, p, p, p, 0, T, None]


def test_transit_header_is_exported_and_typed(lib):
    """What is this header's own (what holds of every public header: tests/test_abi.py::test_public_header)."""
    from celerite2_amd import _lib

    fn = lib.c2_whitened_transits
    assert len(fn.argtypes) == 17 and fn.restype is ctypes.c_int
    assert fn.argtypes[:5] == (ctypes.c_int64,) * 5 and fn.argtypes[5] is _lib.Pointer and fn.argtypes[6] is ctypes.c_int64
    assert fn.argtypes[13] is _lib.Pointer and fn.argtypes[14] is ctypes.c_int64 and fn.argtypes[15] is _lib.Pointer


def test_bad_transit_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_whitened_transits(*tr_args()[:-1])
    with pytest.raises(refused):
        lib.c2_whitened_transits(*tr_args(), None)
    with pytest.raises(refused):
        lib.c2_whitened_transits(*tr_args(B=1.0))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_whitened_transits(*tr_args(p=text))


def test_transit_argument_errors(lib):
    """Sizes, null pointers, J = 33 and Q0 = 9 are refused before anything is launched: no device is needed."""
    from celerite2_amd import _lib

    keep = np.ones(64)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    for bad in (dict(B=0), dict(N=0), dict(J=0), dict(Q0=0), dict(K=0), dict(N=-1), dict(K=-3)):
        assert lib.c2_whitened_transits(*tr_args(p=p, T=p, **bad)) == _lib.C2_ERR_INVALID, bad
    assert lib.c2_whitened_transits(*tr_args(p=p, T=None)) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_transits(*tr_args(p=None, T=p)) == _lib.C2_ERR_INVALID
    neg = tr_args(p=p, T=p)
    neg[14] = -4
    assert lib.c2_whitened_transits(*neg) == _lib.C2_ERR_INVALID
    assert lib.c2_whitened_transits(*tr_args(J=33, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_transits(*tr_args(Q0=9, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    # 2^31 blocks or more: 64 trials a block at every width
    assert lib.c2_whitened_transits(*tr_args(B=2 ** 31, K=64, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_transits(*tr_args(B=2 ** 25, K=64 * 64, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED
    assert lib.c2_whitened_transits(*tr_args(B=2 ** 25, K=64 * 64, J=32, p=p, T=p)) == _lib.C2_ERR_UNSUPPORTED


def test_python_argument_errors():
    """ops.whitened_transits and gp.transit_search raise ValueError before C is entered (CPU tensors: the dtype / device check
    of the op comes first, so its shape specs are exercised through the helper)."""
    from celerite2_amd import gp as G, ops

    dims = dict(B=2, N=5, J=2, Q=3, K=6, F=4, R=4)
    ops._shapes(dims, [("Z0", torch.zeros(2, 5, 3), "BNQ"), ("trials", torch.zeros(6, 4), "KF|BKF"),
                       ("trials", torch.zeros(2, 6, 4), "KF|BKF"), ("out", torch.zeros(2, 6, 4), "BKR")])
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops._shapes(dims, [("trials", torch.zeros(3, 6, 4), "KF|BKF")])
    with pytest.raises(ValueError, match=r"^Invalid shape: out "):
        ops._shapes(dims, [("out", torch.zeros(2, 6, 3), "BKR")])
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    ins = [z(5), z(2), z(2, 5, 2), z(2, 5, 2), z(2, 5), z(2, 5, 3)]
    with pytest.raises(ValueError, match="GPU"):
        ops.whitened_transits(*ins, z(6, 4))
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops.whitened_transits(*ins, z(6, 3))
    with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
        ops.whitened_transits(*ins, z(24))
    with pytest.raises(ValueError, match=r"^Invalid shape: Z0 "):
        ops.whitened_transits(*ins[:5], z(5, 3), z(6, 4))
    # the front end on a stand-in for a computed GP: trials and A are refused before anything is solved
    import types
    gp = types.SimpleNamespace(_need=lambda: None, _check_vector=lambda y: None, _diag=z(2, 5), mean=0.0)
    gp._whitened_columns = lambda y, A: G.GaussianProcess._whitened_columns(gp, y, A)
    for bad in (z(6, 3), z(3, 6, 4), z(24), z(0, 4), [[1.0, 0.0, 0.1, 0.0]]):
        with pytest.raises(ValueError, match=r"^Invalid shape: trials "):
            G.GaussianProcess.transit_search(gp, z(2, 5), bad)
    with pytest.raises(ValueError, match="A must be"):
        G.GaussianProcess.transit_search(gp, z(2, 5), z(6, 4), A="ones")
    with pytest.raises(ValueError, match=r"^Invalid shape: A "):
        G.GaussianProcess.transit_search(gp, z(2, 5), z(6, 4), A=z(4, 2))


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
