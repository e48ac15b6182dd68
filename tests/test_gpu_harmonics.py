# -*- coding: utf-8 -*-
"""GPU checks of the multi-harmonic periodogram under correlated noise: ops.whitened_harmonics (c2_whitened_harmonics,
csrc/c2_harmonics.hip) and GaussianProcess.periodogram(nterms=H).

References: the numpy restatement of the sweep (tests/harmonics_ref.py, pinned to dense algebra by tests/test_harmonics.py),
fed with the device's own d, W and Z0; ops.whitened_sinusoids at h * freq, bit for bit, for what T holds about one harmonic
alone; and two dense generalized-least-squares fits per frequency on the host.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide exactly."""
import numpy as np
import pytest

import harmonics_ref as R
from test_gpu_periodogram import batch, dense_of, dev, gp_case, host, make_kernel

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
LENGTHS = [1, 2, 7, 8, 9, 16, 17, 33, 150]   # the 8- and 16-row staged blocks and their tails, from both sides
TERMS = [2, 3, 4]
WORST = {}


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


def tpw(H, J):
    """Trials per wavefront: a trial takes H lanes rounded to 2 or 4 up to J = 16, 2 H lanes rounded to 4 or 8 above."""
    lanes = 2 if H == 2 else 4
    return 64 // (lanes if J <= 16 else 2 * lanes)


def check(key, x, xo, what=None):
    x = host(x) if hasattr(x, "cpu") else np.asarray(x, dtype=float)
    xo = np.asarray(xo, dtype=float)
    assert x.shape == xo.shape, (what, key, x.shape, xo.shape)
    assert np.array_equal(np.isnan(x), np.isnan(xo)), (what, key)
    m = ~np.isnan(xo)
    e = R.err(x[m], xo[m]) if m.any() and np.any(xo[m]) else (0.0 if not np.any(x[m]) else np.inf)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert e <= 1.0, (what, key, e)


def run(ops, bt, H, t_ref=0.0):
    """(T on the device, the batched restatement on the device's own d, W, Z0, the op's inputs)."""
    import torch

    t, c, a, U, V, Y0, freq = dev(*[bt[k] for k in ("t", "c", "a", "U", "V", "Y0", "freq")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    Z0 = ops.solve_lower(t, c, U, W, Y0)
    T = ops.whitened_harmonics(t, c, U, W, d, Z0, freq, H, t_ref=t_ref)
    torch.cuda.synchronize()
    B, N, J = U.shape
    full = lambda x, n: np.broadcast_to(x, (B, n)) if x.ndim == 1 else x
    want = R.whitened_harmonics_batched(full(bt["t"], N), full(bt["c"], J), bt["U"], host(W), host(d), host(Z0),
                                        full(bt["freq"], bt["freq"].shape[-1]), H, t_ref)
    return T, want, (t, c, U, W, d, Z0, freq)


def alone(H, Q0, g):
    """Where T holds what belongs to harmonic g + 1 alone, in whitened_sinusoids' order: its three products and its 2 Q0
    products with Z0."""
    NC, HEAD = 2 * H, H * (2 * H + 1)
    return ([R.tri(2 * g, 2 * g, NC), R.tri(2 * g, 2 * g + 1, NC), R.tri(2 * g + 1, 2 * g + 1, NC)]
            + list(range(HEAD + 2 * g * Q0, HEAD + (2 * g + 2) * Q0)))


@pytest.mark.parametrize("J", WIDTHS)
@pytest.mark.parametrize("H", TERMS)
def test_op_vs_restatement(ops, H, J):
    """Every width on every length at one trial more than a wavefront's, Q0 = 2; B = 1 and 3, shared and per-series t, c and
    freq rotate so that each meets each length over the widths."""
    jx, F = WIDTHS.index(J), tpw(H, J) + 1
    for i, N in enumerate(LENGTHS):
        B = (1, 3)[(i + jx) % 2]
        per_tc, per_f = bool((i // 2 + jx) % 2), bool((i + jx // 2) % 2)
        T, want, _ = run(ops, batch(10 * J + N, B, N, J, 2, F, per_tc, per_f), H)
        assert tuple(T.shape) == (B, F, R.width(H, 2))
        check("T vs restatement", T, want, (H, J, N, B, per_tc, per_f))


@pytest.mark.parametrize("J", [3, 8, 32])
@pytest.mark.parametrize("H", TERMS)
def test_lane_tail_and_columns(ops, H, J):
    """The lane tail, a second and a third wavefront and every accumulator count: F x Q0 at N = 33."""
    w = tpw(H, J)
    for F in (1, w - 1, w, w + 1, 2 * w + 2):
        for Q0 in (1, 2, 3, 8):
            B = 1 + (F + Q0) % 3
            T, want, _ = run(ops, batch(J + F + Q0, B, 33, J, Q0, F, bool(F % 2), bool(Q0 % 2)), H)
            assert tuple(T.shape) == (B, F, R.width(H, Q0))
            check("T vs restatement", T, want, (H, J, F, Q0, B))


@pytest.mark.parametrize("J", [2, 8, 16, 32])
def test_bit_for_bit_with_the_periodogram(ops, J):
    """H = 1 is whitened_sinusoids; for H = 2, 3, 4 what T holds about harmonic h alone is the whole of
    whitened_sinusoids at h * freq (formed in float64 on the device: the same single rounding) -- both lane forms, shared
    and per-series frequencies, t_ref off zero, a lane tail."""
    import torch

    Q0 = 2 + J % 3
    T1, _, ins = run(ops, batch(90 + J, 3, 33, J, Q0, 2 * tpw(2, J) + 3, True, bool(J % 3)), 1, t_ref=0.75)
    t, c, U, W, d, Z0, freq = ins
    assert torch.equal(T1, ops.whitened_sinusoids(*ins, t_ref=0.75))
    for H in TERMS:
        T = ops.whitened_harmonics(*ins, H, t_ref=0.75)
        for g in range(H):
            S = ops.whitened_sinusoids(t, c, U, W, d, Z0, (float(g + 1) * freq).contiguous(), t_ref=0.75)
            assert torch.equal(T[..., alone(H, Q0, g)], S), (J, H, g)


@pytest.mark.parametrize("J", [2, 8, 32])
@pytest.mark.parametrize("H", TERMS)
def test_phase(ops, H, J):
    """t_ref off zero; phases on both sides of kSincosFastMax = 1.6e6 in one wavefront, counting the top harmonic's phase
    (the device library's sine and cosine beyond it); times offset by 2.45e6 with t_ref at the offset."""
    F = tpw(H, J) + 1
    bt = batch(70 + J, 3, 33, J, 2, F, True, True)
    T, want, _ = run(ops, bt, H, t_ref=1.375)
    check("T vs restatement, t_ref", T, want, (H, J))
    big = dict(bt)
    big["freq"] = bt["freq"] / bt["freq"].max() * 2.0e6 / H        # the top harmonic's |x| up to 2e6 (t - t_ref)max
    T, want, _ = run(ops, big, H)
    x = np.abs(H * big["freq"][:, :, None] * bt["t"][:, None, :])
    assert float(x.max()) > 3.2e6 and float(x.min()) < 0.8e6
    check("T vs restatement, library sincos", T, want, (H, J))
    jd = batch(70 + J, 3, 33, J, 2, F, True, True, shift=2.45e6)
    T, want, _ = run(ops, jd, H, t_ref=2.45e6)
    check("T vs restatement, offset times", T, want, (H, J))


@pytest.mark.parametrize("H,J,N,F,Q0", [(2, 2, 9, 5, 1), (3, 8, 33, 65, 2), (4, 32, 20, 40, 3), (4, 16, 150, 130, 8)])
def test_plain_call_properties(ops, H, J, N, F, Q0):
    """Two calls give identical bits, a caller-owned `out` gives the same bits, inputs are unchanged, `out` may not alias an
    input, a non-contiguous or mis-shaped input is named, and nterms outside 1 .. 4 is refused."""
    import torch

    T0, want, ins = run(ops, batch(50 + J, 3, N, J, Q0, F, True, True), H)
    before = [x.clone() for x in ins]
    T1 = ops.whitened_harmonics(*ins, H)
    own = torch.full((3, F, R.width(H, Q0)), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.whitened_harmonics(*ins, H, out=own) is own
    torch.cuda.synchronize()
    assert torch.equal(T0, T1) and torch.equal(T0, own)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))
    t, c, U, W, d, Z0, freq = ins
    pool = torch.zeros(max(own.numel(), Z0.numel()), dtype=torch.float64, device="cuda")
    pool[:Z0.numel()] = Z0.reshape(-1)
    with pytest.raises(ValueError, match="out must not alias Z0"):
        ops.whitened_harmonics(t, c, U, W, d, pool[:Z0.numel()].view(Z0.shape), freq, H, out=pool[:own.numel()].view(own.shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_harmonics(t, c, U, W, d, Z0.transpose(0, 1).contiguous().transpose(0, 1), freq, H)
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_harmonics(t, c, U, W, d, Z0, torch.stack([freq, freq], dim=-1)[..., 0], H)
    with pytest.raises(ValueError, match="Invalid shape: freq"):
        ops.whitened_harmonics(t, c, U, W, d, Z0, freq[:2], H)
    with pytest.raises(ValueError, match="Invalid shape: Z0"):
        ops.whitened_harmonics(t, c, U, W, d, Z0[:, :-1].contiguous(), freq, H)
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.whitened_harmonics(*ins, H, out=own[:, :-1].contiguous())
    for bad in (0, 5, -2, 2.0):
        with pytest.raises(ValueError, match="nterms"):
            ops.whitened_harmonics(*ins, bad)
    if Q0 == 8:
        wide = torch.zeros((3, N, 9), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            ops.whitened_harmonics(t, c, U, W, d, wide, freq, H)


# ---- gp.periodogram(nterms=H) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["mean", None, "shared3", "batched3"])
@pytest.mark.parametrize("H", TERMS)
def test_gp_periodogram_vs_dense(ops, H, design):
    """All three normalisations and return_fit against two dense GLS fits per frequency on the host, for the first, second
    and last series of a batch of 3; shared and per-series frequencies, t_ref off zero, a tensor mean."""
    import torch
    from celerite2_amd import gp as G, harmonics as hm

    B, N, F = 3, 120, 40
    x, diag, A, y = gp_case(B, N)
    A[...] = A[0]                                      # (one design matrix for "shared3"; "batched3" scales it per series)
    if design == "batched3":
        A = A * (1.0 + 0.5 * np.arange(B))[:, None, None]
    xd, dd, Ad, yd = dev(x, diag, A, y)
    kernel, tn = make_kernel()
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=tn(0.3))
    use = {"mean": "mean", None: None, "shared3": Ad[0].contiguous(), "batched3": Ad}[design]
    A0 = {"mean": A[..., :1] * 0 + 1, None: A[..., :0], "shared3": A, "batched3": A}[design]
    freq = np.stack([2.0 * np.pi / 30.0 * np.linspace(1.0, 12.0, F) * (1.0 + 0.01 * b) for b in range(B)])
    for fq, t_ref in ((freq, 0.0), (freq[0], 11.5)):
        fd, = dev(fq)
        want = [R.dense_harmonics(dense_of(gp, x, b), x[b], A0[b], y[b] - 0.3, fq[b] if fq.ndim == 2 else fq, H, t_ref) for b in range(B)]
        dchi2, amp, chi2_0 = [np.stack([w[k] for w in want]) for k in range(3)]
        for nm, ref in (("standard", dchi2 / chi2_0[:, None]), ("chi2", dchi2), ("log_likelihood", 0.5 * dchi2)):
            fit = gp.periodogram(yd, fd, A=use, normalization=nm, t_ref=t_ref, return_fit=True, nterms=H)
            assert isinstance(fit, hm.Harmonics)
            assert tuple(fit.power.shape) == (B, F) and tuple(fit.amplitude.shape) == (B, F, 2 * H) and tuple(fit.chi2_null.shape) == (B,)
            for b in range(B):
                what = (H, design, nm, fq.ndim, b)
                check("gp power vs dense", fit.power[b], ref[b], what)
                check("gp amplitude vs dense", fit.amplitude[b], amp[b], what)
            check("gp chi2_null vs dense", fit.chi2_null, chi2_0, (H, design, nm))
            assert torch.equal(gp.periodogram(yd, fd, A=use, normalization=nm, t_ref=t_ref, nterms=H), fit.power)


def test_gp_one_term_is_todays_path(ops):
    """nterms = 1 returns the Periodogram tuple with the bits of the call without the keyword; anything outside 1 .. 4 is a
    ValueError that names nterms."""
    import torch
    from celerite2_amd import gp as G, periodogram as pg

    x, diag, A, y = gp_case(3, 33, seed=4)
    xd, dd, yd, fd = dev(x, diag, y, 2.0 * np.pi / 30.0 * np.linspace(1.0, 12.0, 40))
    kernel, tn = make_kernel()
    gp = G.GaussianProcess(kernel, xd, diag=dd)
    a, b = gp.periodogram(yd, fd, return_fit=True), gp.periodogram(yd, fd, return_fit=True, nterms=1)
    assert isinstance(b, pg.Periodogram) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert torch.equal(gp.periodogram(yd, fd, nterms=1), a.power)
    for bad in (0, 5, 2.0, None, "2"):
        with pytest.raises(ValueError, match="nterms"):
            gp.periodogram(yd, fd, nterms=bad)


@pytest.mark.parametrize("H", TERMS)
def test_quiet_failures(ops, H):
    """compute(quiet=True) with one series failing its factorisation: it holds NaN, its neighbours keep their bits; a
    repeated nuisance column is NaN for that series only; w = 0 beside the constant column is NaN at that frequency only."""
    import torch
    from celerite2_amd import gp as G

    B, N, F = 4, 33, 36
    x, diag, A, y = gp_case(B, N, seed=9)
    bad_diag, bad_A = diag.copy(), A.copy()
    bad_diag[1, 7] = -50.0            # not positive definite from row 7 on
    bad_A[2, :, 2] = bad_A[2, :, 1]   # rank 2
    freq = np.concatenate([[0.0], 2.0 * np.pi / 30.0 * np.linspace(1.0, 3.0, F - 1)])
    xd, dd, bdd, Ad, bAd, yd, fd = dev(x, diag, bad_diag, A, bad_A, y, freq)
    kernel, tn = make_kernel()
    clean = G.GaussianProcess(kernel, xd, diag=dd).periodogram(yd, fd, return_fit=True, nterms=H)
    assert bool(torch.isnan(clean.power[:, 0]).all()) and bool(torch.isfinite(clean.power[:, 1:]).all())
    assert bool(torch.isnan(clean.amplitude[:, 0]).all()) and bool(torch.isfinite(clean.amplitude[:, 1:]).all())
    gp = G.GaussianProcess(kernel)
    gp.compute(xd, diag=bdd, quiet=True)
    fit = gp.periodogram(yd, fd, return_fit=True, nterms=H)
    for b in range(B):
        if b == 1:
            assert bool(torch.isnan(fit.power[b]).all()) and bool(torch.isnan(fit.amplitude[b]).all()) and bool(torch.isnan(fit.chi2_null[b]))
        else:
            for got, want in zip(fit, clean):
                assert np.array_equal(host(got[b]), host(want[b]), equal_nan=True), b
    rank = G.GaussianProcess(kernel, xd, diag=dd).periodogram(yd, fd[1:].contiguous(), A=bAd, return_fit=True, nterms=H)
    full = G.GaussianProcess(kernel, xd, diag=dd).periodogram(yd, fd[1:].contiguous(), A=Ad, return_fit=True, nterms=H)
    for b in range(B):
        if b == 2:
            assert bool(torch.isnan(rank.power[b]).all()) and bool(torch.isnan(rank.amplitude[b]).all()) and bool(torch.isnan(rank.chi2_null[b]))
        else:
            assert bool(torch.isfinite(rank.power[b]).all())
            for nm, got, want in zip(rank._fields, rank, full):
                check("rank-deficient neighbour " + nm, got[b], host(want[b]), (H, b))


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
