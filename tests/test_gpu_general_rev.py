# -*- coding: utf-8 -*-
"""The reverse of general_matmul_lower / general_matmul_upper on the device (csrc/c2_general_rev.hip) and what stands on it:
ops.general_matmul_*_rev against the dense operator under torch autograd (tests/general_rev_ref.py), autograd.general_matmul_*,
autograd.get_celerite_matrices, autograd.predict_mean against dense algebra, and predict_mean_kernel / gp.predict_kernel
against a dense restatement of the kernel.  The criterion everywhere is the project's: 1e-10 relative per element plus 1e-12
of the array's largest entry (general_rev_ref.close)."""
import numpy as np
import pytest

import general_rev_ref as R

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (2, 7), (7, 2), (8, 9), (9, 8), (33, 17), (257, 300)]   # around the ring of 8 and the unroll of 4
WIDTHS = [1, 2, 3, 8, 16, 32]
NRHS = [1, 3, 8, 9]
BATCHES = [1, 3, 70]            # 70: not a multiple of the series per wavefront
NAMES = ("bt1", "bt2", "bc", "bU", "bV", "bY")
FORWARDS = {"default": {}, "no_tile": {"general_tile": 0}, "first_round": {"general_tile": 0, "generalk": 0}}
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


def check(key, got, want, what=None):
    got = host(got) if hasattr(got, "cpu") else np.asarray(got)
    WORST[key] = max(WORST.get(key, 0.0), R.close(got, want, "%s %s" % (key, what)))


def case_of(J, N, M):
    """The right-hand sides and the batch size that go with a width and a shape: they rotate, so that every value meets
    every width and every shape; the dense reference of 70 series is kept to the shapes where it is small."""
    iw, ish = WIDTHS.index(J), SHAPES.index((N, M))
    B = BATCHES[(iw + 2 * ish) % 3]
    if B == 70 and N * M > 1000:
        B = 3
    return NRHS[(iw + ish) % 4], B


class forward_kernels:
    """The dispatch options that select the forward kernel writing F, set for a block and put back."""

    def __init__(self, which):
        self.opts = FORWARDS[which]

    def __enter__(self):
        from celerite2_amd import _lib
        for k, v in self.opts.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from celerite2_amd import _lib
        for k in self.opts:
            _lib.set_option(k, None)


def nan_out(B, N, M, J, K):
    import torch
    return tuple(torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
                 for s in ((B, N), (B, M), (B, J), (B, N, J), (B, M, J), (B, M, K)))


def run(ops, arrs, lower, which="default"):
    """Forward with its workspace (by the chosen forward kernel), then the reverse into NaN-filled outputs."""
    t1, t2, c, U, V, Y, bZ = dev(*arrs)
    fwd = ops.general_matmul_lower if lower else ops.general_matmul_upper
    rev = ops.general_matmul_lower_rev if lower else ops.general_matmul_upper_rev
    with forward_kernels(which):
        Z, F = fwd(t1, t2, c, U, V, Y, workspace=True, zero_z=True)
    B, N, J = U.shape
    out = rev(t1, t2, c, U, V, Y, F, bZ, out=nan_out(B, N, V.shape[1], J, Y.shape[2]))
    return Z, F, out


@pytest.mark.parametrize("which", list(FORWARDS))
@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("J", WIDTHS)
def test_reverse_against_dense_autograd(ops, J, N, M, which):
    """Both variants, every grid kind: the forward value and the six cotangents against the dense operator under torch
    autograd; outputs prefilled with NaN come back fully written; every t1 in front of t2[0] gives exact zeros; F written by
    each forward kernel that can write one."""
    K, B = case_of(J, N, M)
    for lower in (True, False):
        for ik, kind in enumerate(R.GRID_KINDS):
            arrs = R.inputs(kind, B, N, M, J, K, 100 * J + 10 * N + ik, lower)
            Z, F, got = run(ops, arrs, lower, which)
            Zd, want = R.dense(*arrs, lower)
            what = (kind, "lower" if lower else "upper", B, K)
            check("Z " + which, Z, Zd, what)
            for nm, g, w in zip(NAMES, got, want):
                check(nm + " " + which, g, w, what)
            if kind == "t1_before":
                assert not bool(Z.any()) and all(not bool(g.any()) for g in got), what


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_shared_grids_and_rates(ops, lower):
    """t1 (N,), t2 (M,), c (J,) shared by the batch: the same per-series cotangents as the batched call on expanded copies."""
    import torch
    B, N, M, J, K = 5, 33, 17, 3, 3
    t1, t2, c, U, V, Y, bZ = R.inputs("ties", B, N, M, J, K, 77, lower)
    t1d, t2d, cd, Ud, Vd, Yd, bZd = dev(t1[0], t2[0], c[0], U, V, Y, bZ)
    fwd = ops.general_matmul_lower if lower else ops.general_matmul_upper
    rev = ops.general_matmul_lower_rev if lower else ops.general_matmul_upper_rev
    Z, F = fwd(t1d, t2d, cd, Ud, Vd, Yd, workspace=True, zero_z=True)
    got = rev(t1d, t2d, cd, Ud, Vd, Yd, F, bZd)
    full = [t1d[None].expand(B, N).contiguous(), t2d[None].expand(B, M).contiguous(), cd[None].expand(B, J).contiguous()]
    Zb, Fb = fwd(*full, Ud, Vd, Yd, workspace=True, zero_z=True)
    want = rev(*full, Ud, Vd, Yd, Fb, bZd)
    assert torch.equal(Z, Zb) and all(torch.equal(g, w) for g, w in zip(got, want))
    _, dense = R.dense(np.repeat(t1[:1], B, 0), np.repeat(t2[:1], B, 0), np.repeat(c[:1], B, 0), U, V, Y, bZ, lower)
    for nm, g, w in zip(NAMES, got, dense):
        check("shared " + nm, g, w)


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_time_cotangents_are_the_local_identities(ops, lower):
    """bt1 == -+ (U o bU) c and bt2 == +- (V o bV) c (upper sign: lower)."""
    for kind in R.GRID_KINDS:
        arrs = R.inputs(kind, 3, 33, 17, 8, 3, 5, lower)
        _, _, (bt1, bt2, bc, bU, bV, bY) = run(ops, arrs, lower)
        t1, t2, c, U, V, Y, bZ = arrs
        sg = 1.0 if lower else -1.0
        check("identity bt1", bt1, -sg * np.einsum("bnj,bj->bn", U * host(bU), c), kind)
        check("identity bt2", bt2, sg * np.einsum("bmj,bj->bm", V * host(bV), c), kind)


@pytest.mark.parametrize("J,K", [(2, 1), (8, 9), (32, 3)])
def test_two_calls_give_identical_bits(ops, J, K):
    import torch
    for lower in (True, False):
        t1, t2, c, U, V, Y, bZ = dev(*R.inputs("interleaved", 130, 200, 170, J, K, 21, lower))
        fwd = ops.general_matmul_lower if lower else ops.general_matmul_upper
        rev = ops.general_matmul_lower_rev if lower else ops.general_matmul_upper_rev
        Z, F = fwd(t1, t2, c, U, V, Y, workspace=True, zero_z=True)
        g1 = rev(t1, t2, c, U, V, Y, F, bZ)
        g2 = rev(t1, t2, c, U, V, Y, F, bZ)
        assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_seventy_thousand_series(ops):
    """B = 70 000 x N = 5 x M = 4 x J = 2: every series against the dense operator."""
    B, N, M, J, K = 70000, 5, 4, 2, 1
    rng = np.random.default_rng(3)
    t1 = np.sort(rng.uniform(0, 10, (B, N)), axis=1)
    t2 = np.sort(rng.uniform(0, 10, (B, M)), axis=1)
    arrs = (t1, t2, rng.uniform(0.05, 1.5, (B, J)), rng.normal(size=(B, N, J)), rng.normal(size=(B, M, J)),
            rng.normal(size=(B, M, K)), rng.normal(size=(B, N, K)))
    for lower in (True, False):
        Z, F, got = run(ops, arrs, lower)
        Zd, want = R.dense(*arrs, lower)
        check("70000 Z", Z, Zd)
        for nm, g, w in zip(NAMES, got, want):
            check("70000 " + nm, g, w, lower)


def test_graph_capture_of_the_reverse(ops):
    """One torch.cuda.graph capture of the reverse on caller-owned outputs (a single stream) replays correctly on a new bZ."""
    import torch
    B, N, M, J, K = 12, 257, 190, 8, 1
    t1, t2, c, U, V, Y, bZ = dev(*R.inputs("interleaved", B, N, M, J, K, 31, True))
    Z, F = ops.general_matmul_lower(t1, t2, c, U, V, Y, workspace=True, zero_z=True)
    out = nan_out(B, N, M, J, K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        ops.general_matmul_lower_rev(t1, t2, c, U, V, Y, F, bZ, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.general_matmul_lower_rev(t1, t2, c, U, V, Y, F, bZ, out=out)
    bZ2 = torch.from_numpy(np.random.default_rng(32).standard_normal(tuple(bZ.shape))).cuda()
    bZ.copy_(bZ2)
    for o in out:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    expect = ops.general_matmul_lower_rev(t1, t2, c, U, V, Y, F, bZ2)
    assert all(torch.equal(a, b) for a, b in zip(out, expect))
    _, want = R.dense(*[host(x) for x in (t1, t2, c, U, V, Y, bZ2)], True)
    for nm, g, w in zip(NAMES, out, want):
        check("graph " + nm, g, w)


def test_shape_and_aliasing_errors(ops):
    import torch
    B, N, M, J, K = 2, 5, 4, 2, 3
    t1, t2, c, U, V, Y, bZ = dev(*R.inputs("interleaved", B, N, M, J, K, 1, True))
    Z, F = ops.general_matmul_lower(t1, t2, c, U, V, Y, workspace=True, zero_z=True)
    good = dict(t1=t1, t2=t2, c=c, U=U, V=V, Y=Y, F=F, bZ=bZ)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    bad = dict(t1=z(B, N + 1), t2=z(M + 1), c=z(B, J + 1), V=z(B, M, J + 1), Y=z(B, M + 1, K), F=z(B, M, J, K + 1), bZ=z(B, N, K + 1))
    for rev in (ops.general_matmul_lower_rev, ops.general_matmul_upper_rev):
        for name, v in bad.items():
            with pytest.raises(ValueError, match="Invalid shape: %s" % name):
                rev(**dict(good, **{name: v}))
        for i, name in enumerate(NAMES):
            out = list(nan_out(B, N, M, J, K))
            out[i] = z(*[d + 1 for d in out[i].shape])
            with pytest.raises(ValueError, match="Invalid shape: %s" % name):
                rev(**good, out=tuple(out))
        out = list(nan_out(B, N, M, J, K))
        out[5] = Y
        with pytest.raises(ValueError, match="bY must not alias Y"):
            rev(**good, out=tuple(out))
        out = list(nan_out(B, N, M, J, K))
        out[4] = out[3].view(-1)[:B * M * J].view(B, M, J)
        with pytest.raises(ValueError, match="bV must not alias bU"):
            rev(**good, out=tuple(out))
        with pytest.raises(ValueError, match="width not supported"):
            rev(t1, t2, z(B, 33), z(B, N, 33), z(B, M, 33), Y, z(B, M, 33, K), bZ)


# ---- autograd ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["batched", "shared"])
@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_autograd_general_matmul(ops, lower, shared):
    from celerite2_amd import autograd as ag
    B, N, M, J, K = 4, 33, 17, 3, 3
    t1, t2, c, U, V, Y, bZ = R.inputs("ties", B, N, M, J, K, 9, lower)
    if shared:
        t1, t2, c = t1[0], t2[0], c[0]
    args = [x.requires_grad_() for x in dev(t1, t2, c, U, V, Y)]
    Z = (ag.general_matmul_lower if lower else ag.general_matmul_upper)(*args)
    Z.backward(dev(bZ)[0])
    Zd, want = R.dense(t1, t2, c, U, V, Y, bZ, lower)
    check("autograd Z", Z, Zd)
    for nm, x, w in zip(NAMES, args, want):
        check("autograd " + nm, x.grad, w, shared)


def torch_celerite_matrices(ar, ac, bc, dc, x, diag):
    """The celerite matrices in torch, columns [real terms, (cos, sin) pairs]: a = diag + sum ar + sum ac,
    U = [ar, ac cos + bc sin, ac sin - bc cos], V = [1, cos, sin] at the phases dc x."""
    import torch
    B, N = diag.shape
    ex = lambda v: v if v.dim() == 2 else v[None].expand(B, v.shape[0])
    ar, ac, bc, dc, x = ex(ar), ex(ac), ex(bc), ex(dc), ex(x)
    arg = dc[:, None, :] * x[:, :, None]
    cs, sn = torch.cos(arg), torch.sin(arg)
    a = diag + ar.sum(-1, keepdim=True) + ac.sum(-1, keepdim=True)
    Uc = torch.stack([ac[:, None] * cs + bc[:, None] * sn, ac[:, None] * sn - bc[:, None] * cs], -1).reshape(B, N, -1)
    Vc = torch.stack([cs, sn], -1).reshape(B, N, -1)
    U = torch.cat([ar[:, None, :].expand(B, N, ar.shape[-1]), Uc], -1)
    V = torch.cat([torch.ones((B, N, ar.shape[-1]), dtype=diag.dtype), Vc], -1)
    return a, U, V


@pytest.mark.parametrize("shared", [False, True], ids=["batched", "shared"])
def test_autograd_get_celerite_matrices(ops, shared):
    import torch
    from celerite2_amd import autograd as ag
    B, N, Jr, Jc = 4, 33, 1, 2
    rng = np.random.default_rng(4)
    sh = (lambda n: (n,)) if shared else (lambda n: (B, n))
    arrs = [rng.uniform(0.5, 1.5, sh(Jr)), rng.uniform(0.5, 2.0, sh(Jc)), rng.uniform(0.1, 0.5, sh(Jc)), rng.uniform(0.2, 3.0, sh(Jc)),
            np.sort(rng.uniform(0, 5, sh(N)), axis=-1), rng.uniform(0.1, 0.3, (B, N))]
    cots = [rng.normal(size=(B, N)), rng.normal(size=(B, N, Jr + 2 * Jc)), rng.normal(size=(B, N, Jr + 2 * Jc))]
    args = [x.requires_grad_() for x in dev(*arrs)]
    outs = ag.get_celerite_matrices(*args)
    torch.autograd.backward(outs, dev(*cots))
    cpu = [torch.tensor(x, requires_grad=True) for x in arrs]
    ref = torch_celerite_matrices(*cpu)
    torch.autograd.backward(ref, [torch.tensor(x) for x in cots])
    for nm, o, r in zip(("a", "U", "V"), outs, ref):
        check("matrices " + nm, o, r.detach().numpy())
    for nm, x, r in zip(("ar", "ac", "bc", "dc", "x", "diag"), args, cpu):
        check("matrices b" + nm, x.grad, r.grad.numpy(), shared)


def predict_case(N, M, J, B=3):
    """B series of tests/test_exact_gradients.series with their coefficients (the draw replayed), and queries inside and
    beyond the data span with the kernel's rows there."""
    from oracle import dense
    from test_exact_gradients import series
    out = []
    for b in range(B):
        seed = 50 + b
        t, c, a, U, V, y = series(N, J, seed=seed)
        rng = np.random.default_rng(seed)
        rng.uniform(0, 1, N); rng.uniform(0, 1, N)
        co = dense.sho_sum_coeffs(J - J % 2, rng.uniform(-1, 1)) if J >= 2 else None
        if J % 2:
            co = dense.real_term(1.3, 0.4) if co is None else dense.real_term(1.3, 0.4) + co
        c2, _, U2, V2 = dense.celerite_matrices(co, t, np.zeros(N))
        assert np.array_equal(c2, c) and np.array_equal(U2, U) and np.array_equal(V2, V)
        span = t[-1] - t[0]
        ts = np.sort(np.random.default_rng(seed + 1000).uniform(t[0] - 0.1 * span, t[-1] + 0.1 * span, M))
        ts[M // 2] = t[N // 2]   # a query at a data time
        ts = np.sort(ts)
        _, _, Us, Vs = dense.celerite_matrices(co, ts, np.zeros(M))
        out.append((t, c, a, U, V, y, ts, Us, Vs))
    return [np.stack(x) for x in zip(*out)]


def dense_predict_mean(t, c, a, U, V, y, ts, Us, Vs):
    """K from the semiseparable form, linalg.solve, the cross-covariance through the two dense operators (torch, batched)."""
    import torch
    low = R.dense_operator(t, t, c, U, V, True)
    strict = torch.tril(torch.ones(low.shape[-2:], dtype=torch.bool), -1)
    low = torch.where(strict, low, torch.zeros_like(low))
    K = low + low.transpose(-1, -2) + torch.diag_embed(a)
    alpha = torch.linalg.solve(K, y[..., None])
    return ((R.dense_operator(ts, t, c, Us, V, True) + R.dense_operator(ts, t, c, Vs, U, False)) @ alpha)[..., 0]


@pytest.mark.parametrize("N,M,J", [(9, 7, 2), (33, 17, 3), (65, 40, 8), (300, 257, 8), (300, 100, 16)])
def test_predict_mean_against_dense_autograd(ops, N, M, J):
    """autograd.predict_mean: the mean and all nine gradients against the dense route under torch autograd."""
    import torch
    from celerite2_amd import autograd as ag
    arrs = predict_case(N, M, J)
    w = np.random.default_rng(N).normal(size=(arrs[0].shape[0], M))
    args = [x.requires_grad_() for x in dev(*arrs)]
    mu = ag.predict_mean(*args)
    mu.backward(dev(w)[0])
    cpu = [torch.tensor(x, requires_grad=True) for x in arrs]
    ref = dense_predict_mean(*cpu)
    ref.backward(torch.tensor(w))
    check("predict_mean", mu, ref.detach().numpy(), (N, M, J))
    for nm, x, r in zip(("bt", "bc", "ba", "bU", "bV", "by", "bts", "bUs", "bVs"), args, cpu):
        check("predict_mean " + nm, x.grad, r.grad.numpy(), (N, M, J))


def test_predict_mean_raises_on_a_failed_factorisation(ops):
    from celerite2_amd import autograd as ag
    arrs = predict_case(9, 7, 2)
    arrs[2] = -np.abs(arrs[2])   # a negative diagonal: no factorisation
    with pytest.raises(ag.LinAlgError):
        ag.predict_mean(*dev(*arrs))


def torch_kernel(p, tau):
    """k(tau) of RealTerm(a, c) + ComplexTerm(a, b, c, d) + SHOTerm(S0, w0, Q) (underdamped), tau >= 0; p: 9 (B,) columns."""
    import torch
    ar, cr, ac, bc, cc, dc, S0, w0, Q = [v[:, None, None] for v in p]
    f = torch.sqrt(4.0 * Q * Q - 1.0)
    a, cs = S0 * w0 * Q, 0.5 * w0 / Q
    return (ar * torch.exp(-cr * tau) + torch.exp(-cc * tau) * (ac * torch.cos(dc * tau) + bc * torch.sin(dc * tau))
            + torch.exp(-cs * tau) * (a * torch.cos(cs * f * tau) + (a / f) * torch.sin(cs * f * tau)))


def test_predict_mean_kernel_and_gp_predict_kernel(ops):
    """RealTerm + ComplexTerm + underdamped SHOTerm with tensor parameters ((B,) and 0-d mixed), a (B,) jitter and a 0-d
    tensor mean: the value and every gradient against the dense kernel in torch; without jitter the value is gp.predict's."""
    import torch
    from celerite2_amd import autograd as ag, gp as G, terms as T
    B, N, M = 3, 65, 40
    rng = np.random.default_rng(8)
    x = np.sort(rng.uniform(0, 8, (B, N)), axis=1)
    t = np.sort(rng.uniform(-1, 9, (B, M)), axis=1)
    t[:, M // 2] = x[:, N // 2]
    t = np.sort(t, axis=1)
    diag = rng.uniform(0.05, 0.3, (B, N))
    y = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3
    jit = rng.uniform(0.05, 0.3, B)
    P = np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(0.1, 0.5, B), rng.uniform(0.5, 1.5, B), rng.uniform(0.005, 0.02, B),
                  rng.uniform(0.1, 0.4, B), rng.uniform(0.5, 2.0, B), rng.uniform(0.5, 2.0, B), rng.uniform(1.0, 3.0, B),
                  rng.uniform(1.0, 4.0, B)])
    P[1] = P[1, 0]; P[7] = P[7, 0]          # the real term's rate and the oscillator's frequency: 0-d, shared by the batch
    w = rng.normal(size=(B, M))

    def build(dv):
        mk = lambda k: torch.tensor(P[k, 0] if k in (1, 7) else P[k], dtype=torch.float64, device=dv, requires_grad=True)
        p = [mk(k) for k in range(9)]
        rest = [torch.tensor(v, dtype=torch.float64, device=dv, requires_grad=True) for v in (x, t, diag, y, jit, 0.3)]
        return p, rest

    p, (xd, td, dd, yd, jd, md) = build("cuda")
    kernel = (T.RealTerm(a=p[0], c=p[1]) + T.ComplexTerm(a=p[2], b=p[3], c=p[4], d=p[5])
              + T.SHOTerm(S0=p[6], w0=p[7], Q=p[8], regime="under"))
    mu = ag.predict_mean_kernel(kernel, xd, yd, td, diag=dd, jitter=jd, mean=md)
    mu.backward(dev(w)[0])

    q, (xc, tc, dc_, yc, jc, mc) = build("cpu")
    qb = [v if v.dim() == 1 else v.expand(B) for v in q]
    lag = xc[:, :, None] - xc[:, None, :]
    Kd = torch_kernel(qb, torch.where(lag >= 0, lag, -lag)) + torch.diag_embed(dc_ + (jc * jc)[:, None])
    cross = tc[:, :, None] - xc[:, None, :]
    Ks = torch_kernel(qb, torch.where(cross >= 0, cross, -cross))
    ref = (Ks @ torch.linalg.solve(Kd, (yc - mc)[..., None]))[..., 0] + mc
    ref.backward(torch.tensor(w))
    check("kernel mean", mu, ref.detach().numpy())
    for k, (a_, b_) in enumerate(zip(p, q)):
        check("kernel bP", a_.grad, b_.grad.numpy(), k)
    for nm, a_, b_ in zip(("bx", "bt", "bdiag", "by", "bjitter", "bmean"), (xd, td, dd, yd, jd, md), (xc, tc, dc_, yc, jc, mc)):
        check("kernel " + nm, a_.grad, b_.grad.numpy())

    gp = G.GaussianProcess(kernel, xd.detach(), diag=dd.detach(), mean=md.detach())
    plain = gp.predict(yd.detach(), td.detach())
    with torch.no_grad():
        check("gp.predict_kernel", gp.predict_kernel(yd.detach(), td.detach()), host(plain))
    again = gp.predict_kernel(yd.detach(), td.detach(), jitter=jd.detach())
    check("gp.predict_kernel jitter", again, host(mu))


def test_worst_case_report():
    for k in sorted(WORST):
        print("%-32s %.3g of the criterion" % (k, WORST[k]))
