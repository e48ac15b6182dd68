# -*- coding: utf-8 -*-
"""GPU checks of the false-alarm probabilities of the multi-harmonic periodogram: ops.harmonic_projections and
ops.harmonic_null_chi2 (c2_harmonic_projections, c2_harmonic_null_chi2; csrc/c2_harmonic_trials.hip) and
GaussianProcess.search_significance(..., nterms=H).

References: ops.trial_projections("periodogram") at h * freq (bit for bit); the numpy restatement of the projections
(tests/harmonic_significance_ref.py, contracted in np.longdouble) fed with the device's own alpha; harmonics.null_statistics
(plain torch) fed the op's own P; the composed route -- H one-term projections, the permuting copy, null_statistics.
Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import numpy as np
import pytest

import harmonic_significance_ref as R
from linear_model_ref import draw

pytestmark = pytest.mark.gpu
LENGTHS = [1, 3, 4, 5, 67]               # the four-row step of the matrix product and its tails
FREQ_COUNTS = [1, 15, 16, 17, 33]        # 16 frequencies a wavefront
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
    xo = host(xo) if hasattr(xo, "cpu") else np.asarray(xo, dtype=float)
    assert x.shape == xo.shape, (what, key, x.shape, xo.shape)
    assert np.array_equal(np.isnan(x), np.isnan(xo)), (what, key)
    m = ~np.isnan(xo)
    e = R.err(x[m], xo[m]) if m.any() and np.any(xo[m]) else (0.0 if not np.any(x[m]) else np.inf)
    WORST[key] = max(WORST.get(key, 0.0), e)
    print("%s %s: %.3g of the criterion" % (key, what, e))
    assert e <= 1.0, (what, key, e)


def draw_counts(ops, H):
    RB = ops.HARMONIC_DRAWS[H]
    return [1, RB - 1, RB, RB + 1]


def alpha_batch(ops, seed, B, N, Rmax, J=3):
    """B seeded series, each on its own grid, factored on the device; alpha (B, N, Rmax) = L^-T D^-1/2 n from the device's own
    solve_upper.  Returns (t (B, N) on the host, alpha on the device)."""
    import torch

    draws = [draw(1000 * seed + b, N, J) for b in range(B)]
    st = lambda key: np.stack([D[key] for D in draws])
    t, c, a, U, V = dev(*[st(k) for k in ("t", "c", "a", "U", "V")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    n = torch.from_numpy(np.random.default_rng(seed).normal(size=(B, N, Rmax))).cuda()
    return st("t"), ops.solve_upper(t, c, U, W, (n * torch.rsqrt(d)[..., None]).contiguous())


def grid(t, F):
    return R.HR.grid(t, F) if F > 1 else R.HR.grid(t, 2)[:1]


def compare_projections(ops, H, t, alpha, freq, t_ref=0.0, what=None):
    """harmonic_projections against the one-term projection at h * freq (the same bits) and against the restatement."""
    import torch

    td, fd = dev(t, freq)
    P = ops.harmonic_projections(td, alpha, fd, H, t_ref=t_ref)
    B, N, Rn = alpha.shape
    assert tuple(P.shape) == (B, freq.shape[-1], 2 * H, Rn)
    for h in range(1, H + 1):
        one = ops.trial_projections("periodogram", td, alpha, (h * fd).contiguous(), t_ref=t_ref)
        assert torch.equal(P[:, :, 2 * h - 2:2 * h], one), (what, h)
    torch.cuda.synchronize()
    check("P vs restatement", P, R.projections_batched(t, host(alpha), freq, H, t_ref), what)
    return P


# ---- the projection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("H", [2, 3, 4])
def test_projections(ops, H, N):
    """Every frequency count on every draw count at this length: B = 1 and 3, shared and per-series t and freq rotate so
    that each meets each count."""
    counts = draw_counts(ops, H)
    batches = {B: alpha_batch(ops, 10 * N + B, B, N, max(counts)) for B in (1, 3)}
    for i, F in enumerate(FREQ_COUNTS):
        for j, Rn in enumerate(counts):
            B = (1, 3)[(i + j) % 2]
            per_t, per_f = bool((i + j // 2) % 2), bool((i // 2 + j) % 2)
            t, alpha = batches[B]
            if not per_t:
                t = t[0]
            freq = np.stack([grid(t[b] if per_t else t, F) * (1.0 + 0.01 * b) for b in range(B)])
            freq = freq if per_f else freq[0]
            compare_projections(ops, H, t, alpha[..., :Rn].contiguous(), freq, what=(H, N, F, Rn, B, per_t, per_f))


@pytest.mark.parametrize("H", [2, 3, 4])
def test_projection_edges(ops, H):
    """t_ref off zero with phases of the harmonics on both sides of kSincosFastMax = 1.6e6; times offset by 2.45e6 with t_ref
    at the offset."""
    B, N, F = 3, 67, 33
    Rn = ops.HARMONIC_DRAWS[H] + 1
    t, alpha = alpha_batch(ops, 77, B, N, Rn)
    t_ref = 1.375
    freq = np.stack([grid(t[b], F) for b in range(B)])
    freq[:, 1::3] *= 4.0e6 / (H * freq[:, 1::3] * np.max(np.abs(t - t_ref)))    # the H-th harmonic's phase reaches 4e6
    x = np.abs(freq[:, None, :] * (t - t_ref)[:, :, None])
    assert (H * x > 1.6e6).any() and (x < 1.6e6).any() and (H * x).max() < 5e6
    compare_projections(ops, H, t, alpha, freq, t_ref, "edges")
    shift = 2.45e6
    compare_projections(ops, H, t[0] + shift, alpha, grid(t[0], F), shift, "offset times")


# ---- the statistic finished in registers -------------------------------------------------------------------------------
def synthetic_products(seed, B, F, H, P0, rows=40):
    """S0 (B, Q0, Q0) and T (B, F, H (2 H + 1) + 2 H Q0) of a well-conditioned fit: the Gram products of `rows` random rows of
    [A0 | the 2 H columns | y] per series and frequency (A0 and y shared by a series' frequencies)."""
    rng = np.random.default_rng(seed)
    NC, Q0, HEAD = 2 * H, P0 + 1, H * (2 * H + 1)
    Y0 = rng.normal(size=(B, rows, Q0))
    C = rng.normal(size=(B, F, rows, NC))
    S0 = np.einsum("bnp,bnq->bpq", Y0, Y0)
    T = np.zeros((B, F, HEAD + NC * Q0))
    for i in range(NC):
        for j in range(i, NC):
            T[..., R.HR.tri(i, j, NC)] = np.einsum("bfn,bfn->bf", C[..., i], C[..., j])
        T[..., HEAD + i * Q0:HEAD + (i + 1) * Q0] = np.einsum("bfn,bnq->bfq", C[..., i], Y0)
    return S0, T, rows


@pytest.mark.parametrize("P0", [0, 1, 3, 7])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_null_chi2_vs_torch_finish(ops, H, P0):
    """harmonic_null_chi2 against harmonics.null_statistics fed the op's own P, on the walk's tails (N, F, R, B, shared and
    per-series t and freq as in test_projections).  The products S0, T are those of a well-conditioned synthetic fit, so that
    the statistic is finite at every length of the walk; one frequency is made singular on purpose (its Gtt zeroed) and, at
    B = 3, one series is not taken: the reference holds NaN there and nowhere else, and so does the op.  Two calls give
    equal bits."""
    import torch
    from celerite2_amd import harmonics as hm

    counts = draw_counts(ops, H)
    for N in LENGTHS:
        batches = {B: alpha_batch(ops, 10 * N + B + H, B, N, max(counts)) for B in (1, 3)}
        for i, F in enumerate(FREQ_COUNTS):
            j = (i + LENGTHS.index(N)) % len(counts)                   # (every F meets every R over the lengths)
            Rn = counts[j]
            B = (1, 3)[(i + j) % 2]
            per_t, per_f = bool((i + j // 2) % 2), bool((i // 2 + j) % 2)
            t, alpha = batches[B]
            alpha = alpha[..., :Rn].contiguous()
            t = t if per_t else t[0]
            freq = np.stack([grid(t[b] if per_t else t, F) * (1.0 + 0.01 * b) for b in range(B)])
            freq = freq if per_f else freq[0]
            S0, T, rows = synthetic_products(1000 * H + 100 * P0 + 10 * N + F, B, F, H, P0)
            gone = F // 2                                                  # the frequency made singular
            T[:, gone, :H * (2 * H + 1)] = 0.0
            rng = np.random.default_rng(F + Rn)
            G0Y, s_yy = rng.normal(size=(B, P0, Rn)), rows + rng.uniform(1.0, 2.0, size=(B, Rn)) * 50.0
            td, fd, S0d, Td, G0Yd, s_yyd = dev(t, freq, S0, T, G0Y, s_yy)
            ok = torch.tensor([True, False, True][:B], device="cuda") if B == 3 else None
            fac = hm.null_factors(S0d, Td, rows, H, ok)
            V, chi2_0 = hm.null_draws(fac, G0Yd, s_yyd)
            D = ops.harmonic_null_chi2(td, alpha, fd, H, fac.Lm, fac.Xt, V)
            again = ops.harmonic_null_chi2(td, alpha, fd, H, fac.Lm, fac.Xt, V)
            P = ops.harmonic_projections(td, alpha, fd, H)
            torch.cuda.synchronize()
            what = (H, P0, N, F, Rn, B, per_t, per_f)
            assert tuple(D.shape) == (B, F, Rn) and torch.equal(D.view(torch.int64), again.view(torch.int64)), what
            want = hm.null_statistics(S0d, Td, G0Yd, s_yyd, P, rows, H, normalization="chi2", ok=ok)
            placed = np.zeros((B, F, Rn), dtype=bool)
            placed[:, gone] = True
            if B == 3:
                placed[1] = True
            assert np.array_equal(np.isnan(host(want)), placed), what     # (the only NaN: the ones placed)
            check("null_chi2 vs null_statistics on the op's own P", D, want, what)
            check("null_chi2 vs the restated lines", D[0], R.null_chi2(host(P)[0], host(fac.Lm)[0], None if P0 == 0 else host(fac.Xt)[0],
                                                                        None if P0 == 0 else host(V)[0]), what)
            stat = hm.normalize(D, chi2_0, "standard")
            check("standard normalisation", stat, hm.null_statistics(S0d, Td, G0Yd, s_yyd, P, rows, H, ok=ok), what)


@pytest.mark.parametrize("H", [2, 4])
def test_nan_in_one_series(ops, H):
    """With NaN in one series' alpha the other series are bit-identical to the clean call, in both ops."""
    import torch
    from celerite2_amd import harmonics as hm

    B, N, F, P0 = 3, 67, 33, 3
    Rn = ops.HARMONIC_DRAWS[H] + 1
    t, alpha = alpha_batch(ops, 5, B, N, Rn)
    S0, T, rows = synthetic_products(9, B, F, H, P0)
    rng = np.random.default_rng(2)
    td, fd, S0d, Td, G0Yd, s_yyd = dev(t, np.stack([grid(t[b], F) for b in range(B)]), S0, T, rng.normal(size=(B, P0, Rn)),
                                       100.0 + rng.uniform(size=(B, Rn)))
    fac = hm.null_factors(S0d, Td, rows, H)
    V, _ = hm.null_draws(fac, G0Yd, s_yyd)
    dirty = alpha.clone()
    dirty[1, 11, 3] = float("nan")
    clean = ops.harmonic_null_chi2(td, alpha, fd, H, fac.Lm, fac.Xt, V), ops.harmonic_projections(td, alpha, fd, H)
    got = ops.harmonic_null_chi2(td, dirty, fd, H, fac.Lm, fac.Xt, V), ops.harmonic_projections(td, dirty, fd, H)
    torch.cuda.synchronize()
    for g, c in zip(got, clean):
        assert bool(torch.isfinite(c).all()) and torch.equal(g[0], c[0]) and torch.equal(g[2], c[2])
        assert bool(torch.isnan(g[1][..., 3]).all())
        keep = torch.arange(Rn, device="cuda") != 3
        assert torch.equal(g[1][..., keep], c[1][..., keep])               # (a draw is a column of the product: the others keep their bits)


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


def composed(gp, ops, yd, fd, Ad, normals, H, nm, t_ref=0.0):
    """The route there was: H one-term projections at h * freq, the permuting copy to (B, F, 2 H, R), null_statistics, the
    maximum over the frequencies.  Returns (the per-draw statistic (B, F, R), its maxima (B, R))."""
    import torch
    from celerite2_amd import harmonics as hm

    N = yd.shape[1]
    Z0 = gp._whitened_columns(yd, Ad)
    S0 = hm.null_products(Z0, gp._d)
    T = ops.whitened_harmonics(gp._t, gp._c, gp._U, gp._W, gp._d, Z0, fd, H, t_ref=t_ref)
    scaled = (normals * torch.rsqrt(gp._d)[..., None]).contiguous()
    s_yy, G0Y = (normals * normals).sum(dim=1), torch.matmul(Z0[..., :-1].transpose(1, 2), scaled)
    alpha = ops.solve_upper(gp._t, gp._c, gp._U, gp._W, scaled)
    P = torch.stack([ops.trial_projections("periodogram", gp._t, alpha, (h * fd).contiguous(), t_ref=t_ref) for h in range(1, H + 1)], dim=2)
    P = P.reshape(P.shape[0], P.shape[1], 2 * H, P.shape[-1]).contiguous()
    stat = hm.null_statistics(S0, T, G0Y, s_yy, P, N, H, normalization=nm, ok=gp._flag == 0)
    return stat, torch.where(torch.isnan(stat), torch.full_like(stat, -float("inf")), stat).amax(dim=1)


@pytest.mark.parametrize("nm", ["standard", "chi2", "log_likelihood"])
@pytest.mark.parametrize("H", [2, 3, 4])
def test_search_significance(ops, H, nm):
    """An injected two-harmonic signal: `statistic` is gp.periodogram(nterms=H) to the bit, null_maxima the composed
    route's within the criterion for given normals, fap equal; chunked equals unchunked."""
    import torch
    from celerite2_amd import significance as sg

    B, N, F, Rn = 2, 60, 21, 7
    x, diag, A, y = gp_case(B, N, seed=3 + H)
    freq = 2.0 * np.pi / 30.0 * np.linspace(1.3, 6.1, F)
    y = y + 1.5 * np.cos(freq[8] * x + 0.4) + 1.0 * np.sin(2.0 * freq[8] * x - 0.3)
    normals = np.random.default_rng(5).normal(size=(B, N, Rn))
    xd, dd, yd, fd, nd, Ad = dev(x, diag, y, freq, normals, A)
    gp = make_gp(xd, dd)
    got = gp.search_significance("periodogram", yd, fd, A=Ad, normalization=nm, normals=nd, nterms=H)
    assert isinstance(got, sg.Significance) and tuple(got.statistic.shape) == tuple(got.fap.shape) == (B, F)
    assert tuple(got.null_maxima.shape) == (B, Rn)
    assert torch.equal(got.statistic, gp.periodogram(yd, fd, A=Ad, normalization=nm, nterms=H))
    assert host(got.fap)[:, 8].tolist() == [1.0 / (Rn + 1)] * B               # (the injected signal: no draw reaches it)
    stat, maxima = composed(gp, ops, yd, fd, Ad, nd, H, nm)
    assert bool(torch.isfinite(stat).all())
    # no maximum of the reference route lies within 1e-8, relative, of a statistic: the count cannot turn on rounding
    gap = (maxima[:, None, :] - got.statistic[:, :, None]).abs() / got.statistic[:, :, None].abs()
    assert float(gap.min()) > 1e-8
    check("null_maxima vs the composed route", got.null_maxima, maxima, (H, nm))
    assert torch.equal(got.fap, sg.false_alarm_probability(got.statistic, maxima, rtol=1e-10))
    part = gp.search_significance("periodogram", yd, fd, A=Ad, normalization=nm, normals=nd, nterms=H, max_trials=5)
    assert all(torch.equal(a, b) for a, b in zip(part, got))
    part = gp.search_significance("periodogram", yd, fd, A=Ad, normalization=nm, normals=nd, nterms=H, max_trials=5, max_draws=3)
    assert torch.equal(part.statistic, got.statistic) and torch.equal(part.fap, got.fap)
    check("null_maxima, chunked vs unchunked", part.null_maxima, got.null_maxima, (H, nm))


def test_one_term_is_untouched(ops):
    """nterms=1 is the call without the keyword, to the bit."""
    import torch

    B, N, F, Rn = 2, 60, 21, 7
    x, diag, A, y = gp_case(B, N, seed=13)
    freq = 2.0 * np.pi / 30.0 * np.linspace(1.3, 6.1, F)
    normals = np.random.default_rng(6).normal(size=(B, N, Rn))
    xd, dd, yd, fd, nd = dev(x, diag, y, freq, normals)
    gp = make_gp(xd, dd)
    plain = gp.search_significance("periodogram", yd, fd, normals=nd)
    keyed = gp.search_significance("periodogram", yd, fd, normals=nd, nterms=1)
    assert all(torch.equal(a, b) for a, b in zip(plain, keyed)) and bool(torch.isfinite(plain.null_maxima).all())


def test_quiet_failure(ops):
    """compute(quiet=True) with one series failing its factorisation: it holds NaN in every field, its neighbours keep
    their bits."""
    import torch

    B, N, F, Rn, H = 3, 40, 20, 6, 3
    x, diag, A, y = gp_case(B, N, seed=11)
    bad = diag.copy()
    bad[1, 7] = -50.0
    freq = 2.0 * np.pi / 30.0 * np.linspace(1.3, 5.0, F)
    xd, dd, bd, yd, fd = dev(x, diag, bad, y, freq)
    normals = torch.randn((B, N, Rn), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    clean = make_gp(xd, dd).search_significance("periodogram", yd, fd, normals=normals, nterms=H)
    got = make_gp(xd, bd, quiet=True).search_significance("periodogram", yd, fd, normals=normals, nterms=H)
    for f, g in zip(got, clean):
        assert bool(torch.isnan(f[1]).all()) and bool(torch.isfinite(g).all())
        assert torch.equal(f[0], g[0]) and torch.equal(f[2], g[2])


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
