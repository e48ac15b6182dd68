# -*- coding: utf-8 -*-
"""GPU checks of the false-alarm probabilities of the three searches: ops.trial_projections (c2_trial_projections,
csrc/c2_trial_project.hip) and GaussianProcess.search_significance.

References: the numpy restatement of the projections (tests/trial_projections_ref.py: the existing restatements' columns,
contracted in np.longdouble) fed with the device's own alpha; np.linalg.solve on the dense matrix; the loop of the existing
search entry points over the draws; and two dense generalized-least-squares fits per trial and draw on the host.
Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import numpy as np
import pytest

import trial_projections_ref as R

pytestmark = pytest.mark.gpu
LENGTHS = [1, 2, 3, 4, 5, 17, 150]       # the four-row step of the matrix product and its tails
TRIAL_COUNTS = [1, 15, 16, 17, 33]       # 16 trials a wavefront
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


def draw_counts(ops, kind):
    RB = ops.TRIAL_KINDS[kind][3]
    return [1, 15, 16, 17, RB - 1, RB, RB + 1]


def trials_of(kind, t, K, seed):
    if kind == "periodogram":
        return R.PR.grid(t, K) if K > 1 else R.PR.grid(t, 2)[:1]
    if kind == "transit":
        return R.TR.trials_for(t, K, seed=seed)
    return R.KR.trials_for(t, K, seed=seed)


def alpha_batch(ops, seed, B, N, Rmax, J=3):
    """B seeded series, each on its own grid, factored on the device; alpha (B, N, Rmax) = L^-T D^-1/2 n from the device's own
    solve_upper.  Returns (t (B, N) on the host, alpha on the device)."""
    import torch

    draws = [R.KR.draw(1000 * seed + b, N, J) for b in range(B)]
    st = lambda key: np.stack([D[key] for D in draws])
    t, c, a, U, V = dev(*[st(k) for k in ("t", "c", "a", "U", "V")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    n = torch.from_numpy(np.random.default_rng(seed).normal(size=(B, N, Rmax))).cuda()
    return st("t"), ops.solve_upper(t, c, U, W, (n * torch.rsqrt(d)[..., None]).contiguous())


def project(ops, kind, t, alpha, trials, t_ref=0.0, **kw):
    """(P on the device, the restatement on the same alpha) for host t (N,) | (B, N) and trials."""
    import torch

    td, trd = dev(t, trials)
    P = ops.trial_projections(kind, td, alpha, trd, t_ref=t_ref, **kw)
    torch.cuda.synchronize()
    return P, R.projections_batched(kind, t, host(alpha), trials, t_ref)


# ---- the op ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_op_vs_restatement(ops, kind, N):
    """Every trial count on every draw count at this length: B = 1 and 3, shared and per-series t and trials rotate so that
    each meets each count."""
    counts = draw_counts(ops, kind)
    batches = {B: alpha_batch(ops, 10 * N + B, B, N, max(counts)) for B in (1, 3)}
    for i, K in enumerate(TRIAL_COUNTS):
        for j, Rn in enumerate(counts):
            B = (1, 3)[(i + j) % 2]
            per_t, per_tr = bool((i + j // 2) % 2), bool((i // 2 + j) % 2)
            t, alpha = batches[B]
            if not per_t:
                t = t[0]                                       # (the projection of any alpha on the first grid's columns)
            trials = np.stack([trials_of(kind, t[b] if per_t else t, K, N + b) for b in range(B)])
            trials = trials if per_tr else trials[0]
            P, want = project(ops, kind, t, alpha[..., :Rn].contiguous(), trials)
            assert tuple(P.shape) == (B, K, R.NCOL[kind], Rn)
            check("%s: P vs restatement" % kind, P, want, (N, K, Rn, B, per_t, per_tr))


def edge_trials(kind, t, K, seed):
    """Trials on the rules' edges, and what the test asserts about them."""
    tr = trials_of(kind, t, K, seed)
    if kind == "periodogram":
        tr = tr.copy()
        tr[1::3] *= 4.0e6 / (tr[1::3] * np.max(np.abs(t - 1.375)))   # phases beyond kSincosFastMax = 1.6e6 on some rows
    elif kind == "keplerian":
        tr[:, 1] = np.array([0.0, 0.5, 0.99])[np.arange(K) % 3]
        tr[4, 1], tr[5, 0] = 0.995, -tr[5, 0]                  # outside the domain: evaluated as written
    else:
        tr[6, 3] = 0.75 * tr[6, 2]                             # tau > w / 2: outside the domain, evaluated as written
    return tr


@pytest.mark.parametrize("kind", R.KINDS)
def test_op_edges(ops, kind):
    """t_ref off zero with phases on both sides of kSincosFastMax; e = 0, 0.5 and 0.99; single-event and folded boxes and
    trapezoids with samples on a ramp; trials outside the domain; times offset by 2.45e6."""
    B, N, K = 3, 150, 33
    Rn = ops.TRIAL_KINDS[kind][3] + 1
    t, alpha = alpha_batch(ops, 77, B, N, Rn)
    trials = np.stack([edge_trials(kind, t[b], K, 5 + b) for b in range(B)])
    t_ref = 1.375 if kind == "periodogram" else 0.0
    if kind == "periodogram":
        x = np.abs(trials[:, None, :] * (t - t_ref)[:, :, None])
        assert (x > 1.6e6).any() and (x < 1.6e6).any() and x.max() < 5e6
    elif kind == "transit":
        b = R.TR.template(t, trials)
        ramp = ((b > 0) & (b < 1)).any(axis=1)
        assert ramp[:, trials[0, :, 0] > 0].any() and ramp[:, trials[0, :, 0] == 0].any()     # folded and single events
    P, want = project(ops, kind, t, alpha, trials, t_ref)
    assert np.isfinite(want).all()
    check("%s: P vs restatement, edges" % kind, P, want)
    if kind != "transit":                                      # Julian dates, the reference time / periastron at the offset
        shift = 2.45e6
        tr = trials_of(kind, t[0], K, 3).copy()
        if kind == "keplerian":
            tr[:, 2] += shift
        P, want = project(ops, kind, t[0] + shift, alpha, tr, shift if kind == "periodogram" else 0.0)
        check("%s: P vs restatement, offset times" % kind, P, want)


@pytest.mark.parametrize("kind", R.KINDS)
def test_plain_call_properties(ops, kind):
    """Two calls give identical bits, a caller-owned `out` gives the same bits, inputs are unchanged, `out` may not alias an
    input, and a non-contiguous or mis-shaped input is refused."""
    import torch

    B, N, K, Rn = 3, 33, 20, 21
    t, alpha = alpha_batch(ops, 31, B, N, Rn)
    trials = np.stack([trials_of(kind, t[b], K, b) for b in range(B)])
    td, trd = dev(t, trials)
    before = [x.clone() for x in (td, alpha, trd)]
    C = R.NCOL[kind]
    P0 = ops.trial_projections(kind, td, alpha, trd)
    P1 = ops.trial_projections(kind, td, alpha, trd)
    own = torch.full((B, K, C, Rn), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.trial_projections(kind, td, alpha, trd, out=own) is own
    torch.cuda.synchronize()
    assert torch.equal(P0, P1) and torch.equal(P0, own) and bool(torch.isfinite(P0).all())
    assert all(torch.equal(x, y) for x, y in zip((td, alpha, trd), before))
    pool = torch.zeros(max(own.numel(), alpha.numel()), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="out must not alias alpha"):
        ops.trial_projections(kind, td, pool[:alpha.numel()].view(alpha.shape), trd, out=pool[:own.numel()].view(own.shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.trial_projections(kind, td, alpha.transpose(0, 1).contiguous().transpose(0, 1), trd)
    with pytest.raises(ValueError, match="Invalid shape: trials"):
        ops.trial_projections(kind, td, alpha, trd[:2])
    with pytest.raises(ValueError, match="Invalid shape: t "):
        ops.trial_projections(kind, td[:, :-1].contiguous(), alpha, trd)
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.trial_projections(kind, td, alpha, trd, out=own[..., :-1].contiguous())


# ---- the front end ---------------------------------------------------------------------------------------------------------
MEAN = 0.3


def gp_case(B, N, seed=1):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.3, (B, N))
    A = np.stack([np.ones_like(x), x / 30.0 - 0.5, (x / 30.0 - 0.5) ** 2], axis=2)
    y = 0.3 * rng.standard_normal((B, N)) + MEAN + A @ np.array([0.5, -2.0, 1.0])
    return x, diag, A, y


def make_gp(xd, dd, **kw):
    import torch
    from celerite2_amd import gp as G, terms as T

    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kernel = T.SHOTerm(S0=tn(0.4), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.2), c=0.3)
    gp = G.GaussianProcess(kernel, mean=tn(MEAN))
    return gp.compute(xd, diag=dd, **kw)


def search_trials(kind, x, K, seed=2):
    """(B, K[, words]) trials inside each search's domain on the times x (B, N)."""
    rng = np.random.default_rng(seed)
    B = x.shape[0]
    w = 2.0 * np.pi / 30.0 * rng.uniform(1.0, 25.0, (B, K))
    if kind == "periodogram":
        return w
    if kind == "keplerian":
        return np.stack([w, rng.uniform(0.0, 0.9, (B, K)), rng.uniform(-10.0, 40.0, (B, K))], axis=2)
    return np.stack([R.TR.trials_for(x[b], K, seed=seed + b) for b in range(B)])


def existing_search(gp, kind, yd, td, nm, A="mean"):
    """The existing entry point's statistic in normalisation `nm`, (B, K)."""
    if kind == "periodogram":
        return gp.periodogram(yd, td, A=A, normalization=nm)
    if kind == "keplerian":
        return gp.keplerian_search(yd, td, A=A, normalization=nm)
    fit = gp.transit_search(yd, td, A=A, return_fit=True)
    return R.normalized(fit.delta_chi2, fit.chi2_null[:, None], nm)


def dense_case(gp, kind, x, A0, trials, b):
    c = host(gp._c)
    D = dict(t=x[b], c=c[b] if c.ndim == 2 else c, a=host(gp._a)[b], U=host(gp._U)[b], V=host(gp._V)[b], A0=A0[b])
    D[R.TRIALS_KEY[kind]] = trials[b]
    return D


@pytest.mark.parametrize("kind", R.KINDS)
def test_projection_is_the_sweeps_gty(ops, kind):
    """With alpha = apply_inverse(y - mean), P[..., 0] is the entry gty of the existing sweep's T; both are judged against
    np.linalg.solve on the dense matrix."""
    B, N, K = 3, 120, 40
    x, diag, A, y = gp_case(B, N)
    trials = search_trials(kind, x, K)
    xd, dd, yd, td, Ad = dev(x, diag, y, trials, A)
    gp = make_gp(xd, dd)
    alpha = gp.apply_inverse(yd - MEAN)[..., None].contiguous()
    P = ops.trial_projections(kind, xd, alpha, td)
    Z0 = gp._whitened_columns(yd, Ad)
    sweep = {"periodogram": ops.whitened_sinusoids, "transit": ops.whitened_transits, "keplerian": ops.whitened_keplerians}[kind]
    T = sweep(gp._t, gp._c, gp._U, gp._W, gp._d, Z0, td)
    cols = [1 + 3] if kind == "transit" else [3 + 3, 3 + 4 + 3]
    for b in range(B):
        D = dense_case(gp, kind, x, A, trials, b)
        Kd = R.dense(D["t"], D["c"], D["a"], D["U"], D["V"])
        Y0 = np.concatenate([A[b], (y[b] - MEAN)[:, None]], axis=1)
        want = R.REF[kind].dense_products(Kd, x[b], Y0, trials[b])
        for c, col in enumerate(cols):
            check("%s: P vs dense gty" % kind, P[b, :, c, 0], want[:, col], b)
            check("%s: sweep's gty vs dense gty" % kind, T[b, :, col], want[:, col], b)


@pytest.mark.parametrize("nm", ["standard", "chi2", "log_likelihood"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_end_to_end_vs_loop_and_dense(ops, kind, nm):
    """Five given normals: null_maxima against the loop y_r = mean + dot_tril(n_r) -> the existing search -> nanmax, and both
    against the dense fits of y_r; the statistic is the existing search's, to the bit; fap is the count."""
    import torch
    from celerite2_amd import significance as sg

    B, N, K, Rn = 2, 60, 20, 5
    x, diag, A, y = gp_case(B, N, seed=3)
    trials = search_trials(kind, x, K, seed=4)
    normals = np.random.default_rng(5).normal(size=(B, N, Rn))
    xd, dd, yd, td, nd = dev(x, diag, y, trials, normals)
    gp = make_gp(xd, dd)
    got = gp.search_significance(kind, yd, td, normalization=nm, normals=nd)
    assert isinstance(got, sg.Significance) and tuple(got.statistic.shape) == tuple(got.fap.shape) == (B, K)
    assert tuple(got.null_maxima.shape) == (B, Rn)
    assert torch.equal(got.statistic, existing_search(gp, kind, yd, td, nm))
    loop, dense = [], []
    for r in range(Rn):
        yr = MEAN + gp.dot_tril(nd[..., r].contiguous())
        stat = existing_search(gp, kind, yr, td, nm)
        assert bool(torch.isfinite(stat).all())
        loop.append(host(stat).max(axis=1))
        per = []
        for b in range(B):
            D = dense_case(gp, kind, x, np.ones((B, N, 1)), trials, b)
            dchi2, chi2_0, _ = R.dense_statistics(kind, D, (host(yr)[b] - MEAN)[:, None])
            per.append(R.normalized(dchi2, chi2_0[None, :], nm).max())
        dense.append(per)
    dense = np.array(dense).T
    check("%s: null_maxima vs dense fits" % kind, got.null_maxima, dense, nm)
    check("%s: loop of the existing search vs dense fits" % kind, np.stack(loop, axis=1), dense, nm)
    stat = host(got.statistic)
    want = (1 + (host(got.null_maxima)[:, None, :] >= (stat - 1e-10 * np.abs(stat))[:, :, None]).sum(-1)) / (Rn + 1)
    assert np.array_equal(host(got.fap), want)


def test_injected_and_null_series(ops):
    """A strong injected sinusoid: fap at the peak is 1 / (R + 1).  A series that IS the first draw: its maximum meets
    null_maxima[:, 0] and its fap is at least 2 / (R + 1)."""
    import torch

    B, N, K, Rn = 2, 80, 30, 19
    x, diag, A, y = gp_case(B, N, seed=6)
    freq = 2.0 * np.pi / 30.0 * np.linspace(2.0, 20.0, K)
    y = y + 5.0 * np.cos(freq[11] * x + 0.4)
    xd, dd, yd, fd = dev(x, diag, y, freq)
    gp = make_gp(xd, dd)
    gen = torch.Generator(device="cuda").manual_seed(7)
    sig = gp.search_significance("periodogram", yd, fd, draws=Rn, generator=gen)
    assert host(sig.statistic).argmax(axis=1).tolist() == [11, 11]
    assert host(sig.fap)[:, 11].tolist() == [1.0 / (Rn + 1)] * B
    assert bool(torch.isfinite(sig.null_maxima).all()) and tuple(sig.null_maxima.shape) == (B, Rn)
    normals = torch.randn((B, N, Rn), dtype=torch.float64, device="cuda", generator=gen)
    for kind in R.KINDS:
        td, = dev(search_trials(kind, x, K, seed=8))
        y0 = MEAN + gp.dot_tril(normals[..., 0].contiguous())
        sig = gp.search_significance(kind, y0, td, normals=normals, normalization="chi2", dips_only=kind == "transit")
        top = host(sig.statistic).max(axis=1)
        check("%s: the first draw as the observed series" % kind, top, host(sig.null_maxima)[:, 0])
        best = host(sig.fap)[np.arange(B), host(sig.statistic).argmax(axis=1)]
        assert np.all(best >= 2.0 / (Rn + 1) * (1 - 1e-15)), (kind, best)


@pytest.mark.parametrize("kind", R.KINDS)
def test_chunking(ops, kind):
    """max_trials: the same bits.  max_draws: the criterion (the solve may take another kernel at another column count)."""
    import torch

    B, N, K, Rn = 2, 60, 37, 70
    x, diag, A, y = gp_case(B, N, seed=9)
    xd, dd, yd, td, Ad = dev(x, diag, y, search_trials(kind, x, K, seed=10)[0], A)
    normals = torch.randn((B, N, Rn), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    gp = make_gp(xd, dd)
    whole = gp.search_significance(kind, yd, td, normals=normals, A=Ad[0].contiguous())
    assert bool(torch.isfinite(whole.null_maxima).all())
    for max_trials in (1, 16, K - 1, K, 10 ** 6):
        part = gp.search_significance(kind, yd, td, normals=normals, A=Ad[0].contiguous(), max_trials=max_trials)
        assert all(torch.equal(a, b) for a, b in zip(part, whole)), max_trials
    for max_draws in (1, 33, Rn - 1):
        part = gp.search_significance(kind, yd, td, normals=normals, A=Ad[0].contiguous(), max_draws=max_draws, max_trials=20)
        assert torch.equal(part.statistic, whole.statistic)
        check("%s: null_maxima under max_draws" % kind, part.null_maxima, host(whole.null_maxima), max_draws)


@pytest.mark.parametrize("kind", R.KINDS)
def test_quiet_failure(ops, kind):
    """compute(quiet=True) with one series failing its factorisation: it holds NaN in every field, its neighbours keep
    their bits."""
    import torch

    B, N, K, Rn = 3, 33, 20, 6
    x, diag, A, y = gp_case(B, N, seed=11)
    bad = diag.copy()
    bad[1, 7] = -50.0                                          # not positive definite from row 7 on
    xd, dd, bd, yd, td = dev(x, diag, bad, y, search_trials(kind, x, K, seed=12))
    normals = torch.randn((B, N, Rn), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    clean = make_gp(xd, dd).search_significance(kind, yd, td, normals=normals)
    got = make_gp(xd, bd, quiet=True).search_significance(kind, yd, td, normals=normals)
    for f, g in zip(got, clean):
        assert bool(torch.isnan(f[1]).all()) and bool(torch.isfinite(g).all())
        assert torch.equal(f[0], g[0]) and torch.equal(f[2], g[2])


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
