# -*- coding: utf-8 -*-
"""GPU checks of linear mean models: ops.whitened_gram (c2_whitened_gram, csrc/c2_gram.hip), autograd.whitened_gram / gls /
marginal_log_likelihood_kernel and GaussianProcess.fit_linear / marginal_log_likelihood[_kernel].

References: the numpy restatement of the sweep and of the composed reverse rule (tests/linear_model_ref.py, pinned to dense
algebra, to complex-step derivatives and to dense autograd by tests/test_linear_model.py), fed with the device's own d, W,
and the dense objective under torch float64 autograd on the CPU.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; a reference that is identically zero must be met exactly."""
import numpy as np
import pytest

import linear_model_ref as R
import term_params_ref as TP
from inverse_diag_ref import err as ref_err

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
LENGTHS = [1, 2, 7, 8, 9, 16, 17, 33, 150]   # the look-ahead ring (4, 8), the 16-row block and its tail, from both sides
COLUMNS = [1, 2, 3, 5, 8, 9, 16, 17, 32]     # every group size and one lane past it
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
    return None if x is None else x.detach().cpu().numpy()


def check(key, x, xo, what=None):
    x = host(x) if hasattr(x, "cpu") else np.asarray(x)
    xo = np.asarray(xo)
    if not np.any(xo):
        e = 0.0 if not np.any(x) else np.inf
    else:
        e = ref_err(x, xo)
    WORST[key] = max(WORST.get(key, 0.0), e)
    assert np.all(np.isfinite(x)) and e <= 1.0, (what, key, e)


def batch(seed, B, N, J, P, per_tc, per_A, distinct=3):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct).  per_tc: every series on its own grid
    with its own rates, else all on the first draw's t and c (shared (N,) and (J,) arrays); per_A: every series with the
    design matrix of its own grid, scaled per draw, (B, N, P), else the first draw's, (N, P)."""
    draws = []
    for k in range(min(B, distinct)):
        D = R.draw(1000 * seed + k, N, J, t=None if (per_tc or k == 0) else draws[0]["t"])
        D["A"] = R.design(D["t"], P) * (1.0 + 0.25 * k)
        draws.append(D)
    idx = [b % len(draws) for b in range(B)]
    st = lambda key: np.stack([draws[i][key] for i in idx])
    return dict(t=st("t") if per_tc else draws[0]["t"], c=st("c") if per_tc else draws[0]["c"], a=st("a"), U=st("U"), V=st("V"),
                y=st("y"), A=st("A") if per_A else draws[0]["A"])


def factored(ops, bt):
    t, c, a, U, V = dev(*[bt[k] for k in ("t", "c", "a", "U", "V")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    return [t, c, U, W, d]


def series(bt, d, W, b, with_y):
    """(t, c, U, W, d, Y) of series b on the host, d and W the device's; and the dense matrix's (t, c, a, U, V)."""
    t = bt["t"][b] if bt["t"].ndim == 2 else bt["t"]
    c = bt["c"][b] if bt["c"].ndim == 2 else bt["c"]
    A = bt["A"][b] if bt["A"].ndim == 3 else bt["A"]
    Y = np.concatenate([A, bt["y"][b][:, None]], axis=1) if with_y else A
    return (t, c, bt["U"][b], W[b], d[b], Y), (t, c, bt["a"][b], bt["U"][b], bt["V"][b])


def picks(B):
    return sorted(set(range(min(B, 3))) | {B - 2, B - 1} - {-1})


def grid(J):
    """Every length with B = 3 and B = 65 (a padded group; a second workgroup at every G); the column counts, shared /
    per-series t, c, A and y given / absent rotate so that each meets each length over the widths."""
    jx = WIDTHS.index(J)
    for i, N in enumerate(LENGTHS):
        for B in (3, 65):
            Q = COLUMNS[(i + jx + 4 * (B == 65)) % len(COLUMNS)]
            with_y = Q > 1 and (i + jx + (B == 65)) % 2 == 0
            yield N, Q, B, with_y, bool((i + (B == 65)) % 2), bool((i // 2 + jx) % 2)


@pytest.mark.parametrize("J", WIDTHS)
def test_gram_vs_restatement_and_dense(ops, J):
    import torch

    seen = set()
    for N, Q, B, with_y, per_tc, per_A in grid(J):
        P = Q - 1 if with_y else Q
        bt = batch(10 * J + N, B, N, J, P, per_tc, per_A)
        t, c, U, W, d = factored(ops, bt)
        A, y = dev(bt["A"], bt["y"])
        S = ops.whitened_gram(t, c, U, W, d, A, y if with_y else None)
        torch.cuda.synchronize()
        what = (J, N, Q, B, with_y, per_tc, per_A)
        assert tuple(S.shape) == (B, Q, Q), what
        assert torch.equal(S, S.transpose(1, 2)), what
        dh, Wh = host(d), host(W)
        for b in picks(B):
            sw, dn = series(bt, dh, Wh, b, with_y)
            check("S vs restatement", S[b], R.whitened_gram(*sw), (what, b))
            check("S vs dense", S[b], sw[5].T @ np.linalg.solve(R.dense(*dn), sw[5]), (what, b))
        if B == 65:   # a repeat of a draw: identical inputs give identical bits
            assert torch.equal(S[63], S[0]) and torch.equal(S[64], S[1]), what
        seen.add(Q)
    assert len(seen) >= 8


@pytest.mark.parametrize("J,N,Q", [(2, 9, 3), (8, 33, 9), (5, 150, 17), (32, 20, 32), (16, 17, 4)])
def test_plain_call_properties(ops, J, N, Q):
    """Bit-symmetric, two calls give identical bits, a caller-owned S gives the same bits, inputs unchanged, S may not alias
    an input; and against the composed route (ops.solve_lower + a torch Gram) on the same inputs at the standing criterion
    (not bit-equal: the summation order differs)."""
    import torch

    B, P = 37, Q - 1
    bt = batch(50 + J, B, N, J, P, True, True)
    t, c, U, W, d = factored(ops, bt)
    A, y = dev(bt["A"], bt["y"])
    ins = [t, c, U, W, d, A, y]
    before = [x.clone() for x in ins]
    S0 = ops.whitened_gram(*ins)
    S1 = ops.whitened_gram(*ins)
    own = torch.full((B, Q, Q), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.whitened_gram(*ins, S=own) is own
    torch.cuda.synchronize()
    assert torch.equal(S0, S0.transpose(1, 2)) and torch.equal(S0, S1) and torch.equal(S0, own)
    assert all(torch.equal(x, x0) for x, x0 in zip(ins, before))
    Y = torch.cat([A, y[..., None]], dim=-1).contiguous()
    Z = ops.solve_lower(t, c, U, W, Y)
    check("S vs composed", S0, host(torch.bmm(Z.transpose(1, 2), Z / d[..., None])), (J, N, Q))
    buf = torch.empty(max(B * N * P, B * P * P), dtype=torch.float64, device="cuda")
    A2 = buf[:B * N * P].view(B, N, P).copy_(A)
    with pytest.raises(ValueError, match="S must not alias A"):
        ops.whitened_gram(t, c, U, W, d, A2, None, S=buf[:B * P * P].view(B, P, P))
    with pytest.raises(ValueError, match="Invalid shape: S"):
        ops.whitened_gram(*ins, S=torch.empty((B, P, P), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="Invalid shape: A"):
        ops.whitened_gram(t, c, U, W, d, A[:, :-1].contiguous(), y)
    with pytest.raises(ValueError, match="Invalid shape: y"):
        ops.whitened_gram(t, c, U, W, d, A, y[:, :-1].contiguous())


@pytest.mark.parametrize("J,N,Q", [(3, 17, 5), (8, 33, 9)])
def test_offset_arrays(ops, J, N, Q):
    """Every array 8 bytes off a 16-byte boundary between guard words: the same bits, the guards intact."""
    import torch
    from offset_arrays import empty_off16, flanks_intact, off16

    B, P = 5, Q - 1
    bt = batch(70 + J, B, N, J, P, True, True)
    t, c, U, W, d = factored(ops, bt)
    A, y = dev(bt["A"], bt["y"])
    want = ops.whitened_gram(t, c, U, W, d, A, y)
    ins = [off16(x) for x in (t, c, U, W, d, A, y)]
    S = empty_off16((B, Q, Q))
    ops.whitened_gram(*ins, S=S)
    torch.cuda.synchronize()
    assert torch.equal(S, want)
    assert flanks_intact(S) and all(flanks_intact(x) for x in ins)


def test_batch_beyond_65535(ops):
    """B = 65537 at N = 4, J = 2, P = 1 with y: every series against the restatement (every series distinct: its own noise
    level and its own scale of y)."""
    import torch

    B, N, J = 65537, 4, 2
    base = [R.draw(900 + k, N, J) for k in range(3)]
    idx = np.arange(B) % 3
    st = lambda key: np.stack([D[key] for D in base])[idx]
    ramp = np.arange(B) / B
    t, c, U, V = st("t"), st("c"), st("U"), st("V")
    a = st("a") + 0.1 * ramp[:, None]
    y = st("y") * (1.0 + ramp)[:, None]
    A = np.stack([R.design(D["t"], 1) for D in base])[idx] * (1.0 + 0.5 * ramp)[:, None, None]
    td, cd, ad, Ud, Vd, Ad, yd = dev(t, c, a, U, V, A, y)
    d, W, flag = ops.factor(td, cd, ad, Ud, Vd)
    assert int(flag.abs().sum()) == 0
    S = ops.whitened_gram(td, cd, Ud, W, d, Ad, yd)
    torch.cuda.synchronize()
    want = R.whitened_gram_batched(t, c, U, host(W), host(d), np.concatenate([A, y[:, :, None]], axis=2))
    got = host(S)
    assert got.shape == (B, 2, 2) and np.all(np.isfinite(got))
    floor = np.abs(want).max(axis=(1, 2), keepdims=True)
    e = float(np.max(np.abs(got - want) / (1e-10 * np.abs(want) + 1e-12 * floor)))
    WORST["S, B = 65537"] = e
    assert e <= 1.0, e


GRAD_SHAPES = [(1, 1, 1), (2, 9, 3), (8, 33, 9), (8, 17, 17), (16, 40, 5), (32, 20, 32)]      # (J, N, Q)
GRAD_NAMES = ("bt", "bc", "bU", "bW", "bd", "bA", "by")


@pytest.mark.parametrize("B", [3, 65])
@pytest.mark.parametrize("J,N,Q", GRAD_SHAPES)
def test_autograd_whitened_gram(ops, J, N, Q, B):
    """Every gradient of autograd.whitened_gram against the restatement's reverse fed with the device's d, W, and of the
    chain autograd.factor -> autograd.whitened_gram against Y^T K^-1 Y under torch autograd on the CPU; t, c and A shared,
    so the batch sums are covered; y absent at Q = 1."""
    import torch
    from celerite2_amd import autograd as ag

    with_y = Q > 1
    P = Q - 1 if with_y else Q
    bt = batch(30 * J + N, B, N, J, P, False, False)
    bS = np.random.default_rng(J + N + B).standard_normal((B, Q, Q))
    bSd, = dev(bS)
    what = (J, N, Q, B)
    # (1) the op alone, on the device's factors
    t, c, U, W, d = [x.requires_grad_() for x in factored(ops, bt)]
    A, y = [x.requires_grad_() for x in dev(bt["A"], bt["y"])]
    S = ag.whitened_gram(t, c, U, W, d, A, y if with_y else None)
    assert torch.equal(S, ops.whitened_gram(*[x.detach() for x in (t, c, U, W, d, A)], y.detach() if with_y else None))
    (S * bSd).sum().backward()
    dh, Wh = host(d), host(W)
    ref = [R.whitened_gram_rev(*series(bt, dh, Wh, b, with_y)[0], bS[b]) for b in range(B)]
    sumb = lambda k: np.sum([r[k] for r in ref], axis=0)
    stk = lambda k: np.stack([r[k] for r in ref])
    check("gram bt", t.grad, sumb(0), what); check("gram bc", c.grad, sumb(1), what)
    check("gram bU", U.grad, stk(2), what); check("gram bW", W.grad, stk(3), what); check("gram bd", d.grad, stk(4), what)
    check("gram bA", A.grad, sumb(5)[:, :P], what)
    if with_y:
        check("gram by", y.grad, stk(5)[:, :, P], what)
    # (2) the chain through factor against dense autograd
    keys = ("t", "c", "a", "U", "V", "A", "y")
    leaves = [x.requires_grad_() for x in dev(*[bt[k] for k in keys])]
    t, c, a, U, V, A, y = leaves
    d, W = ag.factor(t, c, a, U, V)
    S = ag.whitened_gram(t, c, U, W, d, A, y if with_y else None)
    (S * bSd).sum().backward()
    cpu = [torch.tensor(bt[k], dtype=torch.float64, requires_grad=True) for k in keys]
    tot = 0.0
    vals = []
    for b in range(B):
        Y = torch.cat([cpu[5], cpu[6][b][:, None]], dim=1) if with_y else cpu[5]
        Sb = Y.T @ torch.linalg.solve(R.torch_dense(cpu[0], cpu[1], cpu[2][b], cpu[3][b], cpu[4][b]), Y)
        vals.append(Sb.detach().numpy())
        tot = tot + (Sb * torch.tensor(bS[b])).sum()
    grads = torch.autograd.grad(tot, cpu, allow_unused=True)
    check("chain S", S, np.stack(vals), what)
    for nm, leaf, g in zip(keys, leaves, grads):
        if nm == "y" and not with_y:
            assert leaf.grad is None
            continue
        g = np.zeros(tuple(leaf.shape)) if g is None else g.numpy()
        assert tuple(leaf.grad.shape) == g.shape, (nm, what)
        check("chain b" + nm, leaf.grad, g, (nm, what))


def prior_of(kind, P, B, rng):
    if kind == "flat":
        return None, None
    M = rng.standard_normal((P, P))
    Lam = M @ M.T + 0.5 * np.eye(P)
    if kind == "gaussian_batched":
        return rng.standard_normal((B, P)), np.stack([Lam * (1.0 + 0.1 * b) for b in range(B)])
    return rng.standard_normal(P), Lam


@pytest.mark.parametrize("prior", ["flat", "gaussian", "gaussian_batched"])
@pytest.mark.parametrize("per_A", [False, True])
def test_gls_vs_dense(ops, prior, per_A):
    """autograd.gls at the matrix level: beta, cov and both likelihoods, and the gradient of a weighted sum of all four with
    respect to t, c, a, U, V, A, y, against dense algebra under torch autograd on the CPU."""
    import torch
    from celerite2_amd import autograd as ag

    B, N, J, P = 4, 33, 5, 3
    bt = batch(61, B, N, J, P, per_A, per_A, distinct=B)
    rng = np.random.default_rng(8)
    bt["y"] = bt["y"] + np.einsum("...np,p->...n", bt["A"], rng.standard_normal(P))
    mu0, Lam = prior_of(prior, P, B, rng)
    wb, wc = rng.standard_normal((B, P)), rng.standard_normal((B, P, P))
    keys = ("t", "c", "a", "U", "V", "A", "y")
    leaves = [x.requires_grad_() for x in dev(*[bt[k] for k in keys])]
    pm, pp = [None if v is None else dev(v)[0] for v in (mu0, Lam)]
    fit = ag.gls(*leaves, prior_mean=pm, prior_precision=pp)
    assert isinstance(fit, ag.LinearFit) and tuple(fit.beta.shape) == (B, P) and tuple(fit.cov.shape) == (B, P, P)
    wbd, wcd = dev(wb, wc)
    ((fit.beta * wbd).sum() + (fit.cov * wcd).sum() + fit.log_likelihood.sum() + 0.5 * fit.marginal_log_likelihood.sum()).backward()
    cpu = [torch.tensor(bt[k], dtype=torch.float64, requires_grad=True) for k in keys]
    tot, vals = 0.0, []
    for b in range(B):
        tb, cb = (cpu[0][b], cpu[1][b]) if per_A else (cpu[0], cpu[1])
        Ab = cpu[5][b] if per_A else cpu[5]
        m0 = None if mu0 is None else torch.tensor(mu0[b] if mu0.ndim == 2 else mu0)
        Lm = None if Lam is None else torch.tensor(Lam[b] if Lam.ndim == 3 else Lam)
        K = R.torch_dense(tb, cb, cpu[2][b], cpu[3][b], cpu[4][b])
        r = cpu[6][b] if m0 is None else cpu[6][b] - Ab @ m0
        KiA = torch.linalg.solve(K, Ab)
        H = Ab.T @ KiA + (0.0 if Lm is None else Lm)
        cov = torch.linalg.inv(H)
        beta = cov @ (KiA.T @ r) + (0.0 if m0 is None else m0)
        ll = R.torch_objective(K, Ab, cpu[6][b], m0, Lm, profiled=True)
        mll = R.torch_objective(K, Ab, cpu[6][b], m0, Lm)
        vals.append([v.detach().numpy() for v in (beta, cov, ll, mll)])
        tot = tot + (beta * torch.tensor(wb[b])).sum() + (cov * torch.tensor(wc[b])).sum() + ll + 0.5 * mll
    grads = torch.autograd.grad(tot, cpu)
    what = (prior, per_A)
    for k, (nm, got) in enumerate(zip(("beta", "cov", "ll", "mll"), fit)):
        check("gls " + nm, got, np.stack([v[k] for v in vals]), what)
    for nm, leaf, g in zip(keys, leaves, grads):
        assert tuple(leaf.grad.shape) == tuple(g.shape), (nm, what)
        check("gls b" + nm, leaf.grad, g.numpy(), (nm, what))


RECS = [TP.rec("sho", (0, 1, 2), regime="under"), TP.rec("real", (3, 4))]


def dense_kernel(coefs, tau):
    """k(tau) for tau >= 0 from the celerite coefficients (torch)."""
    import torch
    ar, cr, ac, bc, cc, dc = coefs
    tau = tau[..., None]
    return (ar * torch.exp(-cr * tau)).sum(-1) + (torch.exp(-cc * tau) * (ac * torch.cos(dc * tau) + bc * torch.sin(dc * tau))).sum(-1)


def dense_matrix(coefs, x, D):
    """K + D of one series from the coefficients (torch float64, CPU); lags signed under the mask."""
    import torch
    N = x.shape[0]
    dx = x[:, None] - x[None, :]
    low = torch.tril(torch.ones(N, N, dtype=torch.bool), -1)
    Kl = torch.where(low, dense_kernel(coefs, torch.where(low, dx, torch.zeros_like(dx))), torch.zeros_like(dx))
    return Kl + Kl.T + torch.diag(coefs[0].sum() + coefs[2].sum() + D)


@pytest.mark.parametrize("profiled", [False, True])
@pytest.mark.parametrize("prior", ["flat", "gaussian"])
@pytest.mark.parametrize("N", [9, 150])
def test_marginal_log_likelihood_kernel_vs_dense(ops, N, prior, profiled):
    """SHOTerm (under) + RealTerm with (B,) tensor parameters and a 0-d RealTerm.c, a (B,) jitter, a 0-d tensor mean, yerr as
    sigma, A (B, N, P) = the powers 1 .. P of the scaled times: the value and the gradient of every tensor -- the
    parameters, jitter, mean, x, yerr, y and A."""
    import torch
    from celerite2_amd import autograd as ag, terms as T

    B, P = 4, 3
    rng = np.random.default_rng(40 + N)
    Pm = np.concatenate([TP.draw("sho", rng, B, regime="under")[1], TP.draw("real", rng, B)[1]], 1)
    Pm[:, 4] = Pm[0, 4]
    x = np.sort(rng.uniform(0, max(N, 2) / 10.0, (B, N)), axis=1)
    ye = np.sqrt(rng.uniform(0.1, 0.3, (B, N)))
    A = np.stack([R.design(x[b], P + 1)[:, 1:] for b in range(B)])   # (no constant column: it would absorb the mean, whose
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N)) + A @ np.array([0.3, -1.0, 2.0])   # derivative is then exactly zero)
    jit, mean = rng.uniform(0.05, 0.4, B), float(rng.uniform(-0.3, 0.3))
    mu0, Lam = prior_of(prior, P, B, rng)
    Pt, xd, yed, yd, Ad, jt = [v.requires_grad_() for v in dev(Pm, x, ye, y, A, jit)]
    sc, mt = [torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True) for v in (Pm[0, 4], mean)]
    kernel = T.SHOTerm(S0=Pt[:, 0], w0=Pt[:, 1], Q=Pt[:, 2], regime="under") + T.RealTerm(a=Pt[:, 3], c=sc)
    pm, pp = [None if v is None else dev(v)[0] for v in (mu0, Lam)]
    val = ag.marginal_log_likelihood_kernel(kernel, xd, yd, Ad, yerr=yed, jitter=jt, mean=mt, prior_mean=pm, prior_precision=pp,
                                            profiled=profiled)
    assert tuple(val.shape) == (B,)
    val.sum().backward()
    tn = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
    want = []
    for b in range(B):
        coefs = [tn(v[0]) for v in TP.coefficients(RECS, Pm[b][None])]
        xs, es, j, m, ys, As = [tn(v) for v in (x[b], ye[b], jit[b], mean, y[b], A[b])]
        v = R.torch_objective(dense_matrix(coefs, xs, es * es + j * j), As, ys - m, None if mu0 is None else torch.tensor(mu0),
                              None if Lam is None else torch.tensor(Lam), profiled=profiled)
        g = torch.autograd.grad(v, coefs + [xs, es, j, m, ys, As])
        bP = TP.coefficients_rev(RECS, Pm[b][None], [u.numpy()[None] for u in g[:6]])[0]
        want.append((float(v.detach()), bP) + tuple(u.numpy() for u in g[6:]))
    what = (N, prior, profiled)
    bP = np.stack([w[1] for w in want])
    check("mll", val, np.array([w[0] for w in want]), what)
    check("mll bP", Pt.grad[:, :4], bP[:, :4], what)
    assert not bool(Pt.grad[:, 4].any())
    check("mll bP shared", sc.grad, bP[:, 4].sum(), what)
    check("mll bx", xd.grad, np.stack([w[2] for w in want]), what)
    check("mll byerr", yed.grad, np.stack([w[3] for w in want]), what)
    check("mll bjitter", jt.grad, np.array([w[4] for w in want]), what)
    check("mll bmean", mt.grad, np.sum([w[5] for w in want]), what)
    check("mll by", yd.grad, np.stack([w[6] for w in want]), what)
    check("mll bA", Ad.grad, np.stack([w[7] for w in want]), what)


def gp_case(B=6, N=150, P=3, seed=12):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 0.05 * N + 5, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.4, (B, N))
    A = np.stack([R.design(x[b], P) for b in range(B)])
    y = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3 + A @ np.array([0.5, -2.0, 1.0])[:P]
    return x, diag, A, y


def test_gp_frontend(ops):
    """gp.fit_linear / gp.marginal_log_likelihood equal the autograd values on the GP's own t, diag and mean (flat and Gaussian
    prior, shared and per-series A), the residual is y - mean - A beta, and gp.marginal_log_likelihood_kernel forwards."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N, P = 6, 150, 3
    x, diag, A, y = gp_case(B, N, P)
    xd, dd, Ad, yd = dev(x, diag, A, y)
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kernel = T.SHOTerm(S0=tn(1.2), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.7), c=0.3)
    gp = G.GaussianProcess(kernel, xd, diag=dd, mean=tn(0.3))
    rng = np.random.default_rng(2)
    for prior in ("flat", "gaussian", "gaussian_batched"):
        for Ause in (Ad, Ad[0].contiguous()):
            pm, pp = [None if v is None else dev(v)[0] for v in prior_of(prior, P, B, rng)]
            fit = gp.fit_linear(yd, Ause, prior_mean=pm, prior_precision=pp)
            assert isinstance(fit, G.LinearModelFit) and tuple(fit.residual.shape) == (B, N)
            c, a, U, V = gp._c, gp._a, gp._U, gp._V
            ref = ag.gls(gp._t, c, a, U, V, Ause, yd - 0.3, prior_mean=pm, prior_precision=pp)
            what = (prior, Ause.dim())
            for nm, got, want in zip(ref._fields, fit, ref):
                check("gp " + nm, got, host(want), what)
            check("gp residual", fit.residual, host(yd - 0.3 - torch.matmul(Ause, fit.beta[..., None])[..., 0]), what)
            assert torch.equal(gp.marginal_log_likelihood(yd, Ause, prior_mean=pm, prior_precision=pp), fit.marginal_log_likelihood)
            assert torch.equal(gp.marginal_log_likelihood(yd, Ause, prior_mean=pm, prior_precision=pp, profiled=True),
                               fit.log_likelihood)
            got = gp.marginal_log_likelihood_kernel(yd, Ause, prior_mean=pm, prior_precision=pp)
            assert torch.equal(got, ag.marginal_log_likelihood_kernel(kernel, gp._t, yd, Ause, diag=gp._diag, mean=gp.mean,
                                                                      prior_mean=pm, prior_precision=pp))
            check("gp mll kernel", got, host(fit.marginal_log_likelihood), what)
    # the docstring's use: the stochastic part of the data from the residual
    fit = gp.fit_linear(yd, Ad)
    mu = gp.predict(fit.residual + gp.mean, xd)
    assert tuple(mu.shape) == (B, N) and bool(torch.isfinite(mu).all())


def test_term_convolution_kernel(ops):
    """A TermConvolution is allowed: only the factored matrix is used.  The autograd value equals the GP's on the matrices
    `compute` factored, and the dense objective on those matrices; it is differentiable in the parameters."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N, P = 3, 40, 2
    x, diag, A, y = gp_case(B, N, P, seed=5)
    y = y[:, :N]
    xd, dd, Ad, yd = dev(x, diag, A, y)
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True)
    S0 = tn(1.2)
    kernel = T.TermConvolution(T.SHOTerm(S0=S0, w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.7), c=0.3), 0.05)
    val = ag.marginal_log_likelihood_kernel(kernel, xd, yd, Ad, diag=dd)
    val.sum().backward()
    assert S0.grad is not None and bool(torch.isfinite(S0.grad))
    gp = G.GaussianProcess(kernel, xd, diag=dd)
    check("conv mll vs gp", val, host(gp.marginal_log_likelihood(yd, Ad)))
    want = []
    for b in range(B):
        K = torch.tensor(R.dense(x[b], host(gp._c)[b] if gp._c.dim() == 2 else host(gp._c), host(gp._a)[b], host(gp._U)[b], host(gp._V)[b]))
        want.append(float(R.torch_objective(K, torch.tensor(A[b]), torch.tensor(y[b]))))
    check("conv mll vs dense", val, np.array(want))


def test_quiet_failures_and_shape_errors(ops):
    """compute(quiet=True) with one series failing its factorisation and another given a repeated column: exactly those hold
    NaN / -inf, the rest are what a clean batch gives; the autograd functions raise; shape errors name A."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T

    B, N, P = 6, 33, 3
    x, diag, A, y = gp_case(B, N, P, seed=9)
    bad_diag, bad_A = diag.copy(), A.copy()
    bad_diag[1, 7] = -50.0          # not positive definite from row 7 on
    bad_A[4, :, 2] = bad_A[4, :, 1]   # rank 2
    xd, dd, bdd, Ad, bAd, yd = dev(x, diag, bad_diag, A, bad_A, y)
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kernel = T.SHOTerm(S0=tn(1.2), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.7), c=0.3)
    clean = G.GaussianProcess(kernel, xd, diag=dd).fit_linear(yd, Ad)
    gp = G.GaussianProcess(kernel)
    gp.compute(xd, diag=bdd, quiet=True)
    fit = gp.fit_linear(yd, bAd)
    mll = gp.marginal_log_likelihood(yd, bAd)
    for b in range(B):
        if b in (1, 4):
            assert bool(torch.isnan(fit.beta[b]).all()) and bool(torch.isnan(fit.cov[b]).all()) and bool(torch.isnan(fit.residual[b]).all())
            assert float(fit.log_likelihood[b]) == -np.inf and float(fit.marginal_log_likelihood[b]) == -np.inf
            assert float(mll[b]) == -np.inf
        else:
            for nm, got, want in zip(fit._fields, fit, clean):
                check("quiet " + nm, got[b], host(want[b]), b)
            check("quiet mll", mll[b], host(clean.marginal_log_likelihood[b]), b)
    with pytest.raises(ag.LinAlgError):
        ag.marginal_log_likelihood_kernel(kernel_with_grad(tn), xd, yd, Ad, diag=bdd)
    with pytest.raises(ag.LinAlgError) as e:
        ag.marginal_log_likelihood_kernel(kernel_with_grad(tn), xd, yd, bAd, diag=dd)
    assert e.value.flag.tolist() == [0, 0, 0, 0, 1, 0]
    good = G.GaussianProcess(kernel, xd, diag=dd)
    for bad in (Ad[:, :-1], Ad[:-1], Ad[0, :, 0], Ad[..., None], Ad.transpose(1, 2)):
        for call in (good.fit_linear, good.marginal_log_likelihood, good.marginal_log_likelihood_kernel):
            with pytest.raises(ValueError, match="Invalid shape: A"):
                call(yd, bad.contiguous())
    with pytest.raises(ValueError, match="Invalid shape: A"):
        ag.gls(good._t, good._c, good._a, good._U, good._V, Ad[:, :-1].contiguous(), yd)
    with pytest.raises(ValueError, match="Invalid shape: y"):
        good.fit_linear(yd[:, :-1], Ad)


def kernel_with_grad(tn):
    from celerite2_amd import terms as T
    return T.SHOTerm(S0=tn(1.2).requires_grad_(), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.7), c=0.3)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
