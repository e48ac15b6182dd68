# -*- coding: utf-8 -*-
"""GPU checks of the Keplerian search under correlated noise: ops.whitened_keplerians (c2_whitened_keplerians,
csrc/c2_kepler.hip), GaussianProcess.keplerian_search and GaussianProcess.keplerian_periodogram.

References: the numpy restatement of the solver and the sweep (tests/kepler_ref.py, pinned to a bracketed extended-precision
solution of Kepler's equation and to dense algebra by tests/test_kepler.py), fed with the device's own d, W and Z0, and two
dense generalized-least-squares fits per trial on the host with the columns from bisection.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import numpy as np
import pytest

import kepler_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
LENGTHS = [1, 2, 7, 8, 9, 16, 17, 33, 150]   # the 8- and 16-row staged blocks and their tails, from both sides
WORST = {}


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


def dev(*xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(x):
    return x.detach().cpu().numpy()


def check(key, x, xo, what=None):
    x = host(x) if hasattr(x, "cpu") else np.asarray(x, dtype=float)
    xo = np.asarray(xo, dtype=float)
    assert x.shape == xo.shape, (what, key, x.shape, xo.shape)
    assert np.array_equal(np.isnan(x), np.isnan(xo)), (what, key)
    m = ~np.isnan(xo)
    e = R.err(x[m], xo[m]) if m.any() and np.any(xo[m]) else (0.0 if not np.any(x[m]) else np.inf)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert e <= 1.0, (what, key, e)


def batch(seed, B, N, J, Q0, K, per_tc, per_tr, shift=0.0, trials=None):
    """B seeded draws with Y0 = [design(t, Q0 - 1) | y] and K trials each (e rotating through 0, 1e-9, a uniform draw below
    0.99 and 0.99; tp inside and outside the span).  per_tc: every series on its own grid with its own rates, else all on
    the first draw's t and c (shared (N,) and (J,) arrays); per_tr: (B, K, 3) trials, else the first draw's (K, 3).  shift:
    added to every time and every tp.  trials: a function of the (unshifted) times that replaces the drawn trials."""
    draws = []
    for k in range(B):
        D = R.draw(1000 * seed + k, N, J, t=None if (per_tc or k == 0) else draws[0]["t"])
        D["Y0"] = np.concatenate([R.design(D["t"], Q0 - 1), D["y"][:, None]], axis=1)
        D["trials"] = R.trials_for(D["t"], K, seed=seed + k) if trials is None else trials(D["t"], k)
        D["trials"][:, 2] += shift
        D["t"] = D["t"] + shift
        draws.append(D)
    st = lambda key: np.stack([D[key] for D in draws])
    return dict(t=st("t") if per_tc else draws[0]["t"], c=st("c") if per_tc else draws[0]["c"], a=st("a"), U=st("U"), V=st("V"),
                Y0=st("Y0"), trials=st("trials") if per_tr else draws[0]["trials"])


def run(ops, bt):
    """(T on the device, the batched restatement on the device's own d, W, Z0)."""
    import torch

    t, c, a, U, V, Y0, trials = dev(*[bt[k] for k in ("t", "c", "a", "U", "V", "Y0", "trials")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    Z0 = ops.solve_lower(t, c, U, W, Y0)
    T = ops.whitened_keplerians(t, c, U, W, d, Z0, trials)
    torch.cuda.synchronize()
    B, N, J = U.shape
    full = lambda x, n: np.broadcast_to(x, (B,) + x.shape[-n:]) if x.ndim == n else x
    want = R.whitened_keplerians_batched(full(bt["t"], 1), full(bt["c"], 1), bt["U"], host(W), host(d), host(Z0),
                                         full(bt["trials"], 2))
    return T, want, (t, c, U, W, d, Z0, trials)


@pytest.mark.parametrize("J", WIDTHS)
def test_op_vs_restatement(ops, J):
    """Every width on every length at K = 65, Q0 = 2; B = 1 and 3, shared and per-series t, c and trials rotate so that each
    meets each length over the widths."""
    jx = WIDTHS.index(J)
    for i, N in enumerate(LENGTHS):
        B = (1, 3)[(i + jx) % 2]
        per_tc, per_tr = bool((i // 2 + jx) % 2), bool((i + jx // 2) % 2)
        T, want, _ = run(ops, batch(10 * J + N, B, N, J, 2, 65, per_tc, per_tr))
        assert tuple(T.shape) == (B, 65, 7)
        check("T vs restatement", T, want, (J, N, B, per_tc, per_tr))


@pytest.mark.parametrize("J", [3, 8, 32])
def test_lane_tail_and_columns(ops, J):
    """The lane tail, a second and a third wavefront and every accumulator count: K x Q0 at N = 33.  (J = 32 takes two lanes
    per trial, 32 trials a wavefront: its tails are at 31 .. 33 as well.)"""
    for K in (1, 2, 31, 33, 63, 64, 65, 130):
        for Q0 in (1, 2, 3, 8):
            B = 1 + (K + Q0) % 3
            T, want, _ = run(ops, batch(J + K + Q0, B, 33, J, Q0, K, bool(K % 2), bool(Q0 % 2)))
            assert tuple(T.shape) == (B, K, 3 + 2 * Q0)
            check("T vs restatement", T, want, (J, K, Q0, B))


@pytest.mark.parametrize("J", [2, 8, 32])
def test_circular_limit(ops, J):
    """e = 0 and tp = t_ref: T is ops.whitened_sinusoids' on the same inputs, to the criterion.  Phases stay below 1e3, so
    the reduction by the double 2 pi here and the sine's own reduction there differ by less than 4e-14."""
    import torch

    t_ref = 1.375
    circ = lambda t, k: np.stack([R.trials_for(t, 65, seed=k)[:, 0], np.zeros(65), np.full(65, t_ref)], axis=1)
    bt = batch(40 + J, 3, 33, J, 2, 65, True, True, trials=circ)
    assert float(np.abs(bt["trials"][:, None, :, 0] * (bt["t"][:, :, None] - t_ref)).max()) <= 1e3
    T, _, (t, c, U, W, d, Z0, trials) = run(ops, bt)
    Ts = ops.whitened_sinusoids(t, c, U, W, d, Z0, trials[..., 0].contiguous(), t_ref=t_ref)
    torch.cuda.synchronize()
    check("circular limit vs whitened_sinusoids", T, host(Ts), J)


@pytest.mark.parametrize("J", [2, 8, 32])
def test_edges(ops, J):
    """Against the restatement: rows exactly at periastron (t_n == tp) and rows half a period away (r at +-pi, on either
    side of it by the rounding of the frequency); e = 0.99 throughout; times offset by 2.45e6 with tp at the offset; |x| up
    to 1e6."""
    N, K = 33, 65

    def at_rows(t, k):
        """tp on a row; the frequency puts another row half a period (or three halves) away."""
        tr = R.trials_for(t, K, seed=k)
        i = np.arange(K) % N
        j = (i + 1 + np.arange(K) % 5) % N
        tr[:, 2] = t[i]
        tr[:, 0] = np.pi * (1 + 2 * (np.arange(K) % 2)) / np.abs(t[j] - t[i])
        return tr

    bt = batch(80 + J, 3, N, J, 2, K, True, True, trials=at_rows)
    x = bt["trials"][:, None, :, 0] * (bt["t"][:, :, None] - bt["trials"][:, None, :, 2])
    r = R.reduce_array(x)
    assert np.all((x == 0.0).sum(axis=1) == 1) and np.all((np.abs(np.abs(r) - np.pi) < 1e-12).sum(axis=1) >= 1)
    T, want, _ = run(ops, bt)
    check("T vs restatement, rows at periastron and apastron", T, want, J)

    def high(t, k):
        tr = R.trials_for(t, K, seed=k)
        tr[:, 1] = 0.99
        return tr

    T, want, _ = run(ops, batch(81 + J, 3, N, J, 2, K, True, True, trials=high))
    check("T vs restatement, e = 0.99", T, want, J)

    T, want, _ = run(ops, batch(82 + J, 3, N, J, 2, K, True, True, shift=2.45e6))
    check("T vs restatement, offset times", T, want, J)

    def fast(t, k):
        tr = R.trials_for(t, K, seed=k)
        tr[:, 0] = 1.0e6 / np.max(np.abs(t[:, None] - tr[None, :, 2]), axis=0) * np.linspace(0.01, 1.0, K)
        return tr

    bt = batch(83 + J, 3, N, J, 2, K, True, True, trials=fast)
    x = bt["trials"][:, None, :, 0] * (bt["t"][:, :, None] - bt["trials"][:, None, :, 2])
    assert 0.99e6 < float(np.abs(x).max()) <= 1.0e6 * (1 + 1e-12)
    T, want, _ = run(ops, bt)
    check("T vs restatement, |x| up to 1e6", T, want, J)


@pytest.mark.parametrize("J,N,K,Q0", [(2, 9, 5, 1), (8, 33, 65, 2), (32, 20, 40, 3), (16, 150, 130, 8)])
def test_plain_call_properties(ops, J, N, K, Q0):
    """Two calls give identical bits, a caller-owned `out` gives the same bits, inputs are unchanged, `out` may not alias an
    input, a non-contiguous or mis-shaped input is refused, and so are Q0 = 9 and J = 33."""
    import torch

    T0, want, ins = run(ops, batch(50 + J, 3, N, J, Q0, K, True, True))
    before = [x.clone() for x in ins]
    T1 = ops.whitened_keplerians(*ins)
    own = torch.full((3, K, 3 + 2 * Q0), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.whitened_keplerians(*ins, out=own) is own
    torch.cuda.synchronize()
    assert torch.equal(T0, T1) and torch.equal(T0, own)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))
    t, c, U, W, d, Z0, trials = ins
    pool = torch.zeros(max(own.numel(), Z0.numel()), dtype=torch.float64, device="cuda")
    pool[:Z0.numel()] = Z0.reshape(-1)
    with pytest.raises(ValueError, match="out must not alias Z0"):
        ops.whitened_keplerians(t, c, U, W, d, pool[:Z0.numel()].view(Z0.shape), trials, out=pool[:own.numel()].view(own.shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_keplerians(t, c, U, W, d, Z0.transpose(0, 1).contiguous().transpose(0, 1), trials)
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_keplerians(t, c, U, W, d, Z0, torch.stack([trials, trials], dim=-1)[..., 0])
    with pytest.raises(ValueError, match="Invalid shape: trials"):
        ops.whitened_keplerians(t, c, U, W, d, Z0, trials[:2])
    with pytest.raises(ValueError, match="Invalid shape: trials"):
        ops.whitened_keplerians(t, c, U, W, d, Z0, torch.cat([trials, trials[..., :1]], dim=-1))
    with pytest.raises(ValueError, match="Invalid shape: Z0"):
        ops.whitened_keplerians(t, c, U, W, d, Z0[:, :-1].contiguous(), trials)
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.whitened_keplerians(*ins, out=own[:, :-1].contiguous())
    if Q0 == 8:
        wide = torch.zeros((3, N, 9), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            ops.whitened_keplerians(t, c, U, W, d, wide, trials)
    if J == 32:
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            ops.whitened_keplerians(t, z(3, 33), z(3, N, 33), z(3, N, 33), d, Z0, trials)


# ---- gp.keplerian_search ---------------------------------------------------------------------------------------------------
def gp_case(B, N, seed=1):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.3, (B, N))
    A = np.stack([np.ones_like(x), x / 30.0 - 0.5, (x / 30.0 - 0.5) ** 2], axis=2)
    orbit = np.array([[1.9, 0.6, 3.0]])
    y = np.stack([0.8 * R.columns(x[b], orbit)[0][:, 0] - 0.5 * R.columns(x[b], orbit)[1][:, 0] for b in range(B)])
    y = y + 0.3 * rng.standard_normal((B, N)) + 0.3 + A @ np.array([0.5, -2.0, 1.0])
    return x, diag, A, y


def make_kernel():
    import torch
    from celerite2_amd import terms as T

    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    return T.SHOTerm(S0=tn(0.4), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.2), c=0.3), tn


def dense_of(gp, x, b):
    c = host(gp._c)
    return R.dense(x[b], c[b] if c.ndim == 2 else c, host(gp._a)[b], host(gp._U)[b], host(gp._V)[b])


def search_trials(B, K, seed=2):
    rng = np.random.default_rng(seed)
    return np.stack([2.0 * np.pi / 30.0 * rng.uniform(1.0, 25.0, (B, K)), rng.uniform(0.0, 0.9, (B, K)),
                     rng.uniform(-10.0, 40.0, (B, K))], axis=2)


@pytest.mark.parametrize("design", ["mean", None, "shared3", "batched3"])
def test_gp_keplerian_search_vs_dense(ops, design):
    """All three normalisations and return_fit against two dense GLS fits per trial on the host (columns by bisection in
    extended precision), for every series of a batch of 3; shared and per-series trials, a tensor mean."""
    import torch
    from celerite2_amd import gp as G, kepler as kp

    B, N, K = 3, 120, 40
    x, diag, A, y = gp_case(B, N)
    A[...] = A[0]                                      # (one design matrix for "shared3"; "batched3" scales it per series)
    if design == "batched3":
        A = A * (1.0 + 0.5 * np.arange(B))[:, None, None]
    xd, dd, Ad, yd = dev(x, diag, A, y)
    kernel, tn = make_kernel()
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=tn(0.3))
    use = {"mean": "mean", None: None, "shared3": Ad[0].contiguous(), "batched3": Ad}[design]
    A0 = {"mean": A[..., :1] * 0 + 1, None: A[..., :0], "shared3": A, "batched3": A}[design]
    trials = search_trials(B, K)
    for tr in (trials, trials[0]):
        td, = dev(tr)
        want = [R.dense_keplerian(dense_of(gp, x, b), x[b], A0[b], y[b] - 0.3, tr[b] if tr.ndim == 3 else tr) for b in range(B)]
        dchi2, amp, chi2_0 = [np.stack([w[k] for w in want]) for k in range(3)]
        for nm, ref in (("standard", dchi2 / chi2_0[:, None]), ("chi2", dchi2), ("log_likelihood", 0.5 * dchi2)):
            fit = gp.keplerian_search(yd, td, A=use, normalization=nm, return_fit=True)
            assert isinstance(fit, kp.KeplerianSearch)
            assert tuple(fit.power.shape) == (B, K) and tuple(fit.amplitude.shape) == (B, K, 2) and tuple(fit.chi2_null.shape) == (B,)
            assert tuple(fit.semi_amplitude.shape) == (B, K) and tuple(fit.omega.shape) == (B, K)
            what = (design, nm, tr.ndim)
            check("gp power vs dense", fit.power, ref, what)
            check("gp amplitude vs dense", fit.amplitude, amp, what)
            check("gp semi_amplitude vs dense", fit.semi_amplitude, np.hypot(amp[..., 0], amp[..., 1]), what)
            check("gp omega vs dense", fit.omega, np.arctan2(-amp[..., 1], amp[..., 0]), what)
            check("gp chi2_null vs dense", fit.chi2_null, chi2_0, what)
            assert torch.equal(gp.keplerian_search(yd, td, A=use, normalization=nm), fit.power)


def injection(seed=4):
    """One series with an e = 0.6 orbit of ten noise sigmas on the search grid's own nodes."""
    rng = np.random.default_rng(seed)
    N, sigma = 120, 0.1
    x = np.sort(rng.uniform(0.0, 30.0, (1, N)), axis=1)
    freq = 2.0 * np.pi / 30.0 * np.linspace(4.0, 14.0, 11)
    ecc = np.array([0.0, 0.2, 0.4, 0.6, 0.8])
    n_phase = 8
    w = freq[6]
    true = np.array([w, 0.6, 3 * (2.0 * np.pi / w) / n_phase])
    C, S = R.columns(x[0], true[None])
    y = 0.7 + 10.0 * sigma * (np.cos(0.8) * C[:, 0] - np.sin(0.8) * S[:, 0]) + sigma * rng.standard_normal(N)
    return x, np.full((1, N), sigma ** 2), y[None], freq, ecc, n_phase, true


def test_injected_orbit(ops):
    """The best trial of keplerian_periodogram lies within one grid step of the truth in w, e and tp, and its power exceeds
    the maximum of gp.periodogram on the same frequencies."""
    import torch
    from celerite2_amd import gp as G, terms as T

    x, diag, y, freq, ecc, n_phase, true = injection()
    xd, dd, yd, fd, ed = dev(x, diag, y, freq, ecc)
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    gp = G.GaussianProcess(T.RealTerm(a=tn(0.002), c=tn(0.5)), xd, diag=dd)
    power, best, amp = gp.keplerian_periodogram(yd, fd, ed, n_phase)
    assert tuple(power.shape) == (1, 11) and tuple(best.shape) == (1, 11, 3) and tuple(amp.shape) == (1, 11, 2)
    f = int(torch.argmax(power[0]))
    w, e, tp = host(best[0, f])
    period = 2.0 * np.pi / true[0]
    assert abs(w - true[0]) <= (freq[1] - freq[0]) * (1 + 1e-12), (w, true)
    assert abs(e - true[1]) <= 0.2 * (1 + 1e-12), (e, true)
    assert abs(np.remainder(tp - true[2] + 0.5 * period, period) - 0.5 * period) <= period / n_phase * (1 + 1e-9), (tp, true)
    sinus = gp.periodogram(yd, fd)
    assert float(power.max()) > float(sinus.max()), (float(power.max()), float(sinus.max()))
    assert float(power.max()) > 0.9


def test_quiet_failures_and_argument_errors(ops):
    """compute(quiet=True) with one series failing its factorisation: it holds NaN, its neighbours keep their bits; a
    repeated nuisance column is NaN for that series only; trials outside the domain are NaN at those trials only; bad
    arguments are named."""
    import torch
    from celerite2_amd import gp as G

    B, N, K = 4, 33, 70
    x, diag, A, y = gp_case(B, N, seed=9)
    bad_diag, bad_A = diag.copy(), A.copy()
    bad_diag[1, 7] = -50.0            # not positive definite from row 7 on
    bad_A[2, :, 2] = bad_A[2, :, 1]   # rank 2
    trials = search_trials(1, K, seed=3)[0]
    trials[:, 0] = 2.0 * np.pi / 30.0 * np.linspace(1.5, 12.0, K)
    out = {5: (1, -0.01), 6: (1, 0.995), 7: (0, 0.0), 8: (0, -1.0), 9: (1, float(np.nextafter(0.99, 1.0)))}
    for k, (col, v) in out.items():
        trials[k, col] = v
    trials[10, 1] = 0.99              # the domain's edge is inside
    inside = np.array([k not in out for k in range(K)])
    xd, dd, bdd, Ad, bAd, yd, td = dev(x, diag, bad_diag, A, bad_A, y, trials)
    kernel, tn = make_kernel()
    clean = G.GaussianProcess(kernel, xd, diag=dd).keplerian_search(yd, td, return_fit=True)
    for field in clean[:4]:
        nan = host(torch.isnan(field).reshape(B, K, -1).all(dim=-1))
        fin = host(torch.isfinite(field).reshape(B, K, -1).all(dim=-1))
        assert np.array_equal(nan, np.broadcast_to(~inside, (B, K))) and np.array_equal(fin, np.broadcast_to(inside, (B, K)))
    assert bool(torch.isfinite(clean.chi2_null).all())
    gp = G.GaussianProcess(kernel)
    gp.compute(xd, diag=bdd, quiet=True)
    fit = gp.keplerian_search(yd, td, return_fit=True)
    for b in range(B):
        if b == 1:
            assert all(bool(torch.isnan(f[b]).all()) for f in fit)
        else:
            for got, want in zip(fit, clean):
                assert np.array_equal(host(got[b]), host(want[b]), equal_nan=True), b
    rank = G.GaussianProcess(kernel, xd, diag=dd).keplerian_search(yd, td, A=bAd, return_fit=True)
    full = G.GaussianProcess(kernel, xd, diag=dd).keplerian_search(yd, td, A=Ad, return_fit=True)
    for b in range(B):
        if b == 2:
            assert all(bool(torch.isnan(f[b]).all()) for f in rank)
        else:
            assert bool(torch.isfinite(rank.power[b][torch.from_numpy(inside).cuda()]).all())
            for nm, got, want in zip(rank._fields, rank, full):
                check("rank-deficient neighbour " + nm, got[b], host(want[b]), b)
    good = G.GaussianProcess(kernel, xd, diag=dd)
    for bad in (Ad[:, :-1], Ad[:-1], Ad[0, :, 0], Ad[..., None], torch.cat([Ad, Ad, Ad], dim=-1)[..., :8]):
        with pytest.raises(ValueError, match="Invalid shape: A"):
            good.keplerian_search(yd, td, A=bad.contiguous())
    with pytest.raises(ValueError, match="A must be"):
        good.keplerian_search(yd, td, A="ones")
    for bad in (td[:, :2], torch.stack([td, td]), td.reshape(-1)):
        with pytest.raises(ValueError, match="Invalid shape: trials"):
            good.keplerian_search(yd, bad.contiguous())
    with pytest.raises(ValueError, match="normalization"):
        good.keplerian_search(yd, td, normalization="psd")
    with pytest.raises(ValueError, match="Invalid shape: y"):
        good.keplerian_search(yd[:, :-1], td)


def test_keplerian_periodogram(ops):
    """It is the reshape-and-max of keplerian_search on the same grid; chunked by max_trials it gives the same bits; a
    max_trials below one frequency's trials is refused."""
    import torch
    from celerite2_amd import gp as G, kepler as kp

    B, N, F = 3, 60, 7
    x, diag, A, y = gp_case(B, N, seed=5)
    xd, dd, yd = dev(x, diag, y)
    freq = 2.0 * np.pi / 30.0 * np.linspace(3.0, 12.0, F)
    ecc = [0.0, 0.5, 0.9, 1.2]                                # (the last is outside the domain: NaN trials are ignored)
    fd, = dev(freq)
    kernel, tn = make_kernel()
    gp = G.GaussianProcess(kernel, xd, diag=dd)
    for nm in ("standard", "chi2"):
        power, best, amp = gp.keplerian_periodogram(yd, fd, ecc, 6, normalization=nm, t0=2.0)
        grid = kp.trial_grid(fd, ecc, 6, t0=2.0)
        assert tuple(grid.shape) == (F * 4 * 6, 3) and grid.is_cuda
        fit = gp.keplerian_search(yd, grid, normalization=nm, return_fit=True)
        p = host(fit.power).reshape(B, F, 24)
        assert np.isnan(p[:, :, 18:]).all() and np.isfinite(p[:, :, :18]).all()
        arg = np.nanargmax(p, axis=2)
        assert np.array_equal(host(power), np.take_along_axis(p, arg[..., None], axis=2)[..., 0])
        idx = arg + 24 * np.arange(F)[None, :]
        assert np.array_equal(host(best), host(grid)[idx])
        assert np.array_equal(host(amp), np.stack([host(fit.amplitude)[b][idx[b]] for b in range(B)]))
        for max_trials in (24, 50, 24 * F - 1, 24 * F, 10 ** 6):
            chunked = gp.keplerian_periodogram(yd, fd, ecc, 6, normalization=nm, t0=2.0, max_trials=max_trials)
            assert all(torch.equal(a, b) for a, b in zip(chunked, (power, best, amp))), max_trials
    with pytest.raises(ValueError, match="max_trials"):
        gp.keplerian_periodogram(yd, fd, ecc, 6, max_trials=23)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
