# -*- coding: utf-8 -*-
"""GPU checks of the periodogram under correlated noise: ops.whitened_sinusoids (c2_whitened_sinusoids,
csrc/c2_periodogram.hip) and GaussianProcess.periodogram.

References: the numpy restatement of the sweep (tests/periodogram_ref.py, pinned to dense algebra by
tests/test_periodogram.py), fed with the device's own d, W and Z0, and two dense generalized-least-squares fits per
frequency on the host.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions
must coincide exactly."""
import numpy as np
import pytest

import periodogram_ref as R

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


def batch(seed, B, N, J, Q0, F, per_tc, per_f, shift=0.0):
    """B seeded draws with Y0 = [design(t, Q0 - 1) | y] and a frequency grid each.  per_tc: every series on its own grid with
    its own rates, else all on the first draw's t and c (shared (N,) and (J,) arrays); per_f: (B, F) frequencies, else the
    first draw's (F,).  shift: added to every time (the celerite matrices depend on differences only)."""
    draws = []
    for k in range(B):
        D = R.draw(1000 * seed + k, N, J, t=None if (per_tc or k == 0) else draws[0]["t"])
        D["Y0"] = np.concatenate([R.design(D["t"], Q0 - 1), D["y"][:, None]], axis=1)
        D["freq"] = R.grid(D["t"], F) * (1.0 + 0.03 * k)
        D["t"] = D["t"] + shift
        draws.append(D)
    st = lambda key: np.stack([D[key] for D in draws])
    return dict(t=st("t") if per_tc else draws[0]["t"], c=st("c") if per_tc else draws[0]["c"], a=st("a"), U=st("U"), V=st("V"),
                Y0=st("Y0"), freq=st("freq") if per_f else draws[0]["freq"])


def run(ops, bt, t_ref=0.0):
    """(T on the device, the batched restatement on the device's own d, W, Z0)."""
    import torch

    t, c, a, U, V, Y0, freq = dev(*[bt[k] for k in ("t", "c", "a", "U", "V", "Y0", "freq")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    Z0 = ops.solve_lower(t, c, U, W, Y0)
    T = ops.whitened_sinusoids(t, c, U, W, d, Z0, freq, t_ref=t_ref)
    torch.cuda.synchronize()
    B, N, J = U.shape
    full = lambda x, n: np.broadcast_to(x, (B, n)) if x.ndim == 1 else x
    want = R.whitened_sinusoids_batched(full(bt["t"], N), full(bt["c"], J), bt["U"], host(W), host(d), host(Z0),
                                        full(bt["freq"], bt["freq"].shape[-1]), t_ref)
    return T, want, (t, c, U, W, d, Z0, freq)


@pytest.mark.parametrize("J", WIDTHS)
def test_op_vs_restatement(ops, J):
    """Every width on every length at F = 65, Q0 = 2; B = 1 and 3, shared and per-series t, c and freq rotate so that each
    meets each length over the widths."""
    jx = WIDTHS.index(J)
    for i, N in enumerate(LENGTHS):
        B = (1, 3)[(i + jx) % 2]
        per_tc, per_f = bool((i // 2 + jx) % 2), bool((i + jx // 2) % 2)
        T, want, _ = run(ops, batch(10 * J + N, B, N, J, 2, 65, per_tc, per_f))
        assert tuple(T.shape) == (B, 65, 7)
        check("T vs restatement", T, want, (J, N, B, per_tc, per_f))


@pytest.mark.parametrize("J", [3, 8, 32])
def test_lane_tail_and_columns(ops, J):
    """The lane tail, a second and a third wavefront and every accumulator count: F x Q0 at N = 33.  (J = 32 takes two lanes
    per frequency, 32 frequencies a wavefront: its tails are at 31 .. 33 as well.)"""
    for F in (1, 2, 31, 33, 63, 64, 65, 130):
        for Q0 in (1, 2, 3, 8):
            B = 1 + (F + Q0) % 3
            T, want, _ = run(ops, batch(J + F + Q0, B, 33, J, Q0, F, bool(F % 2), bool(Q0 % 2)))
            assert tuple(T.shape) == (B, F, 3 + 2 * Q0)
            check("T vs restatement", T, want, (J, F, Q0, B))


@pytest.mark.parametrize("J", [2, 8, 32])
def test_phase(ops, J):
    """t_ref off zero; phases on both sides of kSincosFastMax = 1.6e6 in one wavefront (the device library's sine and cosine
    beyond it); times offset by 2.45e6 with t_ref at the offset."""
    bt = batch(70 + J, 3, 33, J, 2, 65, True, True)
    T, want, _ = run(ops, bt, t_ref=1.375)
    check("T vs restatement, t_ref", T, want, J)
    big = dict(bt)
    big["freq"] = bt["freq"] / bt["freq"].max() * 2.0e6          # |x| up to 2e6 (t - t_ref)max ~ 6e6, down to 0 at the first rows
    T, want, _ = run(ops, big)
    assert float(np.abs(big["freq"][:, :, None] * bt["t"][:, None, :]).max()) > 3.2e6
    assert float(np.abs(big["freq"][:, :, None] * bt["t"][:, None, :]).min()) < 0.8e6
    check("T vs restatement, library sincos", T, want, J)
    jd = batch(70 + J, 3, 33, J, 2, 65, True, True, shift=2.45e6)
    T, want, _ = run(ops, jd, t_ref=2.45e6)
    check("T vs restatement, offset times", T, want, J)


@pytest.mark.parametrize("J,N,F,Q0", [(2, 9, 5, 1), (8, 33, 65, 2), (32, 20, 40, 3), (16, 150, 130, 8)])
def test_plain_call_properties(ops, J, N, F, Q0):
    """Two calls give identical bits, a caller-owned `out` gives the same bits, inputs are unchanged, `out` may not alias an
    input, and a non-contiguous or mis-shaped input is refused."""
    import torch

    T0, want, ins = run(ops, batch(50 + J, 3, N, J, Q0, F, True, True))
    before = [x.clone() for x in ins]
    T1 = ops.whitened_sinusoids(*ins)
    own = torch.full((3, F, 3 + 2 * Q0), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.whitened_sinusoids(*ins, out=own) is own
    torch.cuda.synchronize()
    assert torch.equal(T0, T1) and torch.equal(T0, own)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))
    t, c, U, W, d, Z0, freq = ins
    pool = torch.zeros(max(own.numel(), Z0.numel()), dtype=torch.float64, device="cuda")
    pool[:Z0.numel()] = Z0.reshape(-1)
    with pytest.raises(ValueError, match="out must not alias Z0"):
        ops.whitened_sinusoids(t, c, U, W, d, pool[:Z0.numel()].view(Z0.shape), freq, out=pool[:own.numel()].view(own.shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_sinusoids(t, c, U, W, d, Z0.transpose(0, 1).contiguous().transpose(0, 1), freq)
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_sinusoids(t, c, U, W, d, Z0, torch.stack([freq, freq], dim=-1)[..., 0])
    with pytest.raises(ValueError, match="Invalid shape: freq"):
        ops.whitened_sinusoids(t, c, U, W, d, Z0, freq[:2])
    with pytest.raises(ValueError, match="Invalid shape: Z0"):
        ops.whitened_sinusoids(t, c, U, W, d, Z0[:, :-1].contiguous(), freq)
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.whitened_sinusoids(*ins, out=own[:, :-1].contiguous())
    if Q0 == 8:
        wide = torch.zeros((3, N, 9), dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError):
            ops.whitened_sinusoids(t, c, U, W, d, wide, freq)


# ---- gp.periodogram ---------------------------------------------------------------------------------------------------------
def gp_case(B, N, seed=1):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.3, (B, N))
    A = np.stack([np.ones_like(x), x / 30.0 - 0.5, (x / 30.0 - 0.5) ** 2], axis=2)
    y = 0.8 * np.sin(1.9 * x + 0.4) + 0.3 * rng.standard_normal((B, N)) + 0.3 + A @ np.array([0.5, -2.0, 1.0])
    return x, diag, A, y


def make_kernel():
    import torch
    from celerite2_amd import terms as T

    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    return T.SHOTerm(S0=tn(0.4), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.2), c=0.3), tn


def dense_of(gp, x, b):
    c = host(gp._c)
    return R.dense(x[b], c[b] if c.ndim == 2 else c, host(gp._a)[b], host(gp._U)[b], host(gp._V)[b])


@pytest.mark.parametrize("design", ["mean", None, "shared3", "batched3"])
def test_gp_periodogram_vs_dense(ops, design):
    """All three normalisations and return_fit against two dense GLS fits per frequency on the host, for the first, second
    and last series of a batch of 3; shared and per-series frequencies, t_ref off zero, a tensor mean."""
    import torch
    from celerite2_amd import gp as G, periodogram as pg

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
    freq = np.stack([2.0 * np.pi / 30.0 * np.linspace(1.0, 25.0, F) * (1.0 + 0.01 * b) for b in range(B)])
    for fq, t_ref in ((freq, 0.0), (freq[0], 11.5)):
        fd, = dev(fq)
        want = [R.dense_periodogram(dense_of(gp, x, b), x[b], A0[b], y[b] - 0.3, fq[b] if fq.ndim == 2 else fq, t_ref) for b in range(B)]
        dchi2, amp, chi2_0 = [np.stack([w[k] for w in want]) for k in range(3)]
        for nm, ref in (("standard", dchi2 / chi2_0[:, None]), ("chi2", dchi2), ("log_likelihood", 0.5 * dchi2)):
            fit = gp.periodogram(yd, fd, A=use, normalization=nm, t_ref=t_ref, return_fit=True)
            assert isinstance(fit, pg.Periodogram)
            assert tuple(fit.power.shape) == (B, F) and tuple(fit.amplitude.shape) == (B, F, 2) and tuple(fit.chi2_null.shape) == (B,)
            for b in range(B):
                what = (design, nm, fq.ndim, b)
                check("gp power vs dense", fit.power[b], ref[b], what)
                check("gp amplitude vs dense", fit.amplitude[b], amp[b], what)
            check("gp chi2_null vs dense", fit.chi2_null, chi2_0, (design, nm))
            assert torch.equal(gp.periodogram(yd, fd, A=use, normalization=nm, t_ref=t_ref), fit.power)
    if design == "mean":      # the injected 1.9 rad per unit time is what the periodogram finds
        peak = fq[int(torch.argmax(fit.power[0]))]
        assert abs(peak - 1.9) <= 2.0 * np.pi / 30.0, peak


def test_quiet_failures_and_argument_errors(ops):
    """compute(quiet=True) with one series failing its factorisation: it holds NaN, its neighbours keep their bits; a
    repeated nuisance column is NaN throughout; w = 0 beside the constant column is NaN at that frequency only; bad
    arguments are named."""
    import torch
    from celerite2_amd import gp as G

    B, N, F = 4, 33, 70
    x, diag, A, y = gp_case(B, N, seed=9)
    bad_diag, bad_A = diag.copy(), A.copy()
    bad_diag[1, 7] = -50.0            # not positive definite from row 7 on
    bad_A[2, :, 2] = bad_A[2, :, 1]   # rank 2
    freq = np.concatenate([[0.0], 2.0 * np.pi / 30.0 * np.linspace(1.0, 12.0, F - 1)])
    xd, dd, bdd, Ad, bAd, yd, fd = dev(x, diag, bad_diag, A, bad_A, y, freq)
    kernel, tn = make_kernel()
    clean = G.GaussianProcess(kernel, xd, diag=dd).periodogram(yd, fd, return_fit=True)
    assert bool(torch.isnan(clean.power[:, 0]).all()) and bool(torch.isfinite(clean.power[:, 1:]).all())
    assert bool(torch.isnan(clean.amplitude[:, 0]).all()) and bool(torch.isfinite(clean.amplitude[:, 1:]).all())
    gp = G.GaussianProcess(kernel)
    gp.compute(xd, diag=bdd, quiet=True)
    fit = gp.periodogram(yd, fd, return_fit=True)
    for b in range(B):
        if b == 1:
            assert bool(torch.isnan(fit.power[b]).all()) and bool(torch.isnan(fit.amplitude[b]).all()) and bool(torch.isnan(fit.chi2_null[b]))
        else:
            for got, want in zip(fit, clean):
                assert np.array_equal(host(got[b]), host(want[b]), equal_nan=True), b
    rank = G.GaussianProcess(kernel, xd, diag=dd).periodogram(yd, fd[1:].contiguous(), A=bAd, return_fit=True)
    full = G.GaussianProcess(kernel, xd, diag=dd).periodogram(yd, fd[1:].contiguous(), A=Ad, return_fit=True)
    for b in range(B):
        if b == 2:
            assert bool(torch.isnan(rank.power[b]).all()) and bool(torch.isnan(rank.amplitude[b]).all()) and bool(torch.isnan(rank.chi2_null[b]))
        else:
            assert bool(torch.isfinite(rank.power[b]).all())
            for nm, got, want in zip(rank._fields, rank, full):
                check("rank-deficient neighbour " + nm, got[b], host(want[b]), b)
    good = G.GaussianProcess(kernel, xd, diag=dd)
    for bad in (Ad[:, :-1], Ad[:-1], Ad[0, :, 0], Ad[..., None], torch.cat([Ad, Ad, Ad], dim=-1)[..., :8]):
        with pytest.raises(ValueError, match="Invalid shape: A"):
            good.periodogram(yd, fd, A=bad.contiguous())
    with pytest.raises(ValueError, match="A must be"):
        good.periodogram(yd, fd, A="ones")
    with pytest.raises(ValueError, match="Invalid shape: freq"):
        good.periodogram(yd, torch.stack([fd, fd]))
    with pytest.raises(ValueError, match="normalization"):
        good.periodogram(yd, fd, normalization="psd")
    with pytest.raises(ValueError, match="Invalid shape: y"):
        good.periodogram(yd[:, :-1], fd)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
