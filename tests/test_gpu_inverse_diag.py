# -*- coding: utf-8 -*-
"""GPU checks of the linear-time inverse diagonal: ops.inverse_diag (c2_inverse_diag, csrc/c2_invdiag.hip) at every
width (the group kernels up to J = 32, the workgroup kernel beyond), and GaussianProcess.inverse_diagonal / predict_observed / leave_one_out on top of it.

References: the numpy restatement of the recurrence (tests/inverse_diag_ref.py, pinned to np.linalg.inv by
tests/test_inverse_diag.py) and, up to 150 rows, the dense inverse itself.  Criterion: the standing one,
|x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (variances: the floor relative to max(k(0), max D)).  Every dense input has a
condition number <= 1e6, asserted per draw."""
import numpy as np
import pytest

import inverse_diag_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 40, 128]


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


def check(key, x, xo, floor=None, what=None):
    e = R.err(host(x) if hasattr(x, "cpu") else x, xo, floor)
    assert e <= 1.0, (what, key, e)


def batch(seed, B, N, J, *, per_series_t, gap=False, distinct=5):
    """B series from `distinct` seeded draws (series b repeats draw b mod distinct), each on its own grid or all on the
    first draw's."""
    draws = [R.draw(1000 * seed, N, J, gap=gap)]
    for k in range(1, min(B, distinct)):
        draws.append(R.draw(1000 * seed + k, N, J, gap=gap, t=None if per_series_t else draws[0]["t"]))
    idx = [b % len(draws) for b in range(B)]
    stack = lambda key: np.stack([draws[i][key] for i in idx])
    return dict(draws=draws, idx=idx, t=stack("t") if per_series_t else draws[0]["t"], c=stack("c"), a=stack("a"),
                U=stack("U"), V=stack("V"), diag=stack("diag"), y=stack("y"))


def run_case(ops, bt, *, dense, what):
    """ops.inverse_diag without z, with z, and with alpha aliasing z, against the restatement fed with the SAME d, W (the
    device's factorisation) and, if `dense`, against the dense inverse / solve of every distinct draw."""
    import torch

    B = bt["a"].shape[0]
    t, c, a, U, V, y = dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0, what
    z = ops.solve_lower(t, c, U, W, y[..., None].contiguous())[..., 0]
    q0 = ops.inverse_diag(t, c, U, W, d)
    q1, alpha1 = ops.inverse_diag(t, c, U, W, d, z=z)
    z2 = z.clone()
    q2, alpha2 = ops.inverse_diag(t, c, U, W, d, z=z2, alpha=z2)
    torch.cuda.synchronize()
    assert alpha2.data_ptr() == z2.data_ptr()
    assert torch.equal(q0, q1) and torch.equal(q1, q2) and torch.equal(alpha1, alpha2), what   # one pass, same bits
    dh, Wh, zh = host(d), host(W), host(z)
    seen = set()
    for b in range(B):
        k = bt["idx"][b]
        if k in seen:   # a repeat of a draw already compared: identical inputs give identical bits
            b0 = bt["idx"].index(k)
            assert torch.equal(q1[b], q1[b0]) and torch.equal(alpha1[b], alpha1[b0]), (what, b)
            continue
        seen.add(k)
        dr = bt["draws"][k]
        tb = bt["t"][b] if bt["t"].ndim == 2 else bt["t"]
        qr, ar = R.inverse_diag(tb, dr["c"], dr["U"], Wh[b], dh[b], z=zh[b])
        check("q", q1[b], qr, what=(what, b, "restatement"))
        check("alpha", alpha1[b], ar, what=(what, b, "restatement"))
        if dense:
            K = R.dense(tb, dr["c"], dr["a"], dr["U"], dr["V"])
            cond = np.linalg.cond(K)
            assert cond <= 1e6, (what, b, cond)
            check("q", q1[b], np.diag(np.linalg.inv(K)), what=(what, b, "dense"))
            check("alpha", alpha1[b], np.linalg.solve(K, dr["y"]), what=(what, b, "dense"))


@pytest.mark.parametrize("J", WIDTHS)
def test_inverse_diag_vs_restatement_and_dense(ops, J):
    """Every width, N = 1, 2, 33, 150, shared and per-series times, a padded last wavefront (B = 70: not a multiple of 64
    series, nor of 64 / G groups), with and without z, alpha aliasing z, one draw with a gap in time."""
    for i, N in enumerate((1, 2, 33, 150)):
        for B in (3, 70):
            per_series_t = bool((i + (B == 70)) % 2)
            bt = batch(10 * J + i, B, N, J, per_series_t=per_series_t, gap=(N == 150 and B == 3))
            run_case(ops, bt, dense=True, what=(J, N, B, per_series_t))


@pytest.mark.parametrize("J", WIDTHS)
def test_inverse_diag_long_series(ops, J):
    """N = 4096 (256 blocks of 16 rows) against the restatement; at widths 8, 32, 128 also N = 4097: a first block of one
    row."""
    for N, per_series_t in ((4096, True), (4097, False)) if J in (8, 32, 128) else ((4096, J % 2 == 0),):
        bt = batch(77 + J, 2, N, J, per_series_t=per_series_t, distinct=2)
        run_case(ops, bt, dense=False, what=(J, N))


def _gp_inputs(seed, B, N):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0, 0.05 * N + 5, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.4, (B, N))
    y = np.sin(x) + 0.2 * rng.standard_normal((B, N)) + 0.3
    return x, diag, y


def test_fused_alpha_equals_apply_inverse(ops):
    from celerite2_amd import gp as G, terms as T

    x, diag, y = _gp_inputs(3, 6, 300)
    xd, dd, yd = dev(x, diag, y)
    gp = G.GaussianProcess(T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3), xd, diag=dd, mean=0.3)
    q, alpha = gp._q_alpha(yd)
    check("alpha", alpha, host(gp.apply_inverse(yd - 0.3)), what="alpha vs apply_inverse")


def test_predict_observed_equals_predict(ops):
    """8 x 512, a non-convolved kernel with host-float and with tensor hyper-parameters, a tensor mean: mean and variance
    of predict_observed against the existing O(N^2) predict(return_var=True)."""
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N = 8, 512
    x, diag, y = _gp_inputs(4, B, N)
    xd, dd, yd = dev(x, diag, y)
    t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kf = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3) + T.Matern32Term(sigma=0.5, rho=2.0)
    kt = (T.SHOTerm(S0=t(1.2), w0=t(0.9), Q=t(2.5), regime="under") + T.RealTerm(a=t(0.7), c=0.3)
          + T.Matern32Term(sigma=t(0.5), rho=t(2.0)))
    for kernel in (kf, kt):
        gp = G.GaussianProcess(kernel, xd, diag=dd, mean=t(0.3))
        mu_o, var_o = gp.predict(yd, return_var=True)
        k0 = gp.condition(yd)._k0()
        k0 = float(k0.max()) if torch.is_tensor(k0) else float(k0)
        floor = max(k0, float(dd.max()))
        for include_mean in (True, False):
            mu, var = gp.predict_observed(yd, return_var=True, include_mean=include_mean)
            mo = gp.predict(yd, include_mean=include_mean)
            check("mean", mu, host(mo), what=("mean", include_mean))
            check("var", var, host(var_o), floor, what="variance")
            assert torch.equal(gp.predict_observed(yd, include_mean=include_mean), mu)
        assert tuple(var.shape) == (B, N) and bool((var > 0).all()) and bool((var < dd).all())
        q = gp.inverse_diagonal()   # against the old path's variance: q = (D - var_o) / D^2, the identity read backwards
        assert tuple(q.shape) == (B, N) and torch.equal(q, ops.inverse_diag(gp._t, gp._c, gp._U, gp._W, gp._d))


def _dense_of_gp(gp, b):
    t = host(gp._t)
    return R.dense(t[b] if t.ndim == 2 else t, host(gp._c)[b] if gp._c.dim() == 2 else host(gp._c), host(gp._a)[b],
                   host(gp._U)[b], host(gp._V)[b])


def test_term_convolution_variance_is_the_factored_matrix(ops):
    """Under a TermConvolution predict_observed is the variance under the FACTORED (semiseparable) matrix: compared with
    the dense inverse of the matrix rebuilt from the GP's own celerite matrices."""
    from celerite2_amd import gp as G, terms as T

    B, N = 4, 150
    x, diag, y = _gp_inputs(5, B, N)
    xd, dd, yd = dev(x, diag, y)
    gp = G.GaussianProcess(T.TermConvolution(T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3), 0.05), xd,
                           diag=dd, mean=0.3)
    mu, var = gp.predict_observed(yd, return_var=True)
    q = gp.inverse_diagonal()
    for b in range(B):
        K = _dense_of_gp(gp, b)
        assert np.linalg.cond(K) <= 1e6
        Ki = np.linalg.inv(K)
        qo = np.diag(Ki)
        check("q", q[b], qo, what=("conv q", b))
        D = diag[b]
        floor = max(float(np.max(np.diag(K) - D)), float(D.max()))
        check("var", var[b], D - D * D * qo, floor, what=("conv var", b))
        check("mean", mu[b], y[b] - D * (Ki @ (y[b] - 0.3)), what=("conv mean", b))


def test_leave_one_out_vs_deleting_the_point(ops):
    from celerite2_amd import gp as G, terms as T

    B, N = 4, 33
    x, diag, y = _gp_inputs(6, B, N)
    xd, dd, yd = dev(x, diag, y)
    gp = G.GaussianProcess(T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3), xd, diag=dd, mean=0.3)
    mu, var = gp.leave_one_out(yd)
    assert tuple(mu.shape) == tuple(var.shape) == (B, N)
    for b in range(B):
        K = _dense_of_gp(gp, b)
        assert np.linalg.cond(K) <= 1e6
        ref = np.array([R.delete_one(K, y[b] - 0.3, n) for n in range(N)])
        check("loo", var[b], ref[:, 1], what=("loo var", b))
        check("loo", mu[b], ref[:, 0] + 0.3, what=("loo mean", b))


def test_seventy_thousand_series(ops):
    """B = 70 000 (beyond what a grid's y dimension takes) x N = 16: runs, and the first and last series agree with the
    same series computed alone."""
    import torch

    B, N, J = 70000, 16, 4
    rng = np.random.default_rng(8)
    base = R.draw(8, N, J)
    scale = rng.uniform(0.5, 2.0, B)
    a = base["k0"] * scale[:, None] + base["diag"][None] * rng.uniform(0.5, 2.0, (B, 1))
    U = base["U"][None] * scale[:, None, None]
    V = np.broadcast_to(base["V"][None], (B, N, J))
    y = rng.standard_normal((B, N))
    t, c, ad, Ud, Vd, yd = dev(base["t"], base["c"], a, U, V, y)
    d, W, flag = ops.factor(t, c, ad, Ud, Vd)
    z = ops.solve_lower(t, c, Ud, W, yd[..., None].contiguous())[..., 0]
    q, alpha = ops.inverse_diag(t, c, Ud, W, d, z=z)
    torch.cuda.synchronize()
    assert int(flag.abs().sum()) == 0 and bool(torch.isfinite(q).all()) and bool(torch.isfinite(alpha).all())
    for b in (0, B - 1):
        s = slice(b, b + 1)
        q1, a1 = ops.inverse_diag(t, c, Ud[s].contiguous(), W[s].contiguous(), d[s].contiguous(), z=z[s].contiguous())
        check("q", q[b], host(q1[0]), what=("70000", b))
        check("alpha", alpha[b], host(a1[0]), what=("70000", b))
        K = R.dense(base["t"], base["c"], a[b], U[b], V[b])
        check("q", q[b], np.diag(np.linalg.inv(K)), what=("70000 dense", b))


def test_failed_series_gives_nan_and_leaves_its_neighbours_alone(ops):
    import torch
    from celerite2_amd import gp as G, terms as T

    B, N = 9, 100
    x, diag, y = _gp_inputs(9, B, N)
    bad = diag.copy()
    bad[4, 37] = -50.0   # not positive definite from row 37 on
    kernel = T.SHOTerm(S0=1.2, w0=0.9, Q=2.5) + T.RealTerm(a=0.7, c=0.3)
    xd, dd, bd, yd = dev(x, diag, bad, y)
    good = G.GaussianProcess(kernel, xd, diag=dd, mean=0.3)
    gp = G.GaussianProcess(kernel, mean=0.3).compute(xd, diag=bd, quiet=True)
    assert host(gp._flag).tolist() == [0, 0, 0, 0, 37, 0, 0, 0, 0]
    ok = [b for b in range(B) if b != 4]
    for fn in (lambda g: (g.inverse_diagonal(),), lambda g: g.predict_observed(yd, return_var=True),
               lambda g: g.leave_one_out(yd)):
        for got, want in zip(fn(gp), fn(good)):
            assert bool(torch.isnan(got[4]).all())
            assert torch.equal(got[ok], want[ok])   # bit-identical to the same batch without the failure
            assert bool(torch.isfinite(want).all())


@pytest.mark.parametrize("J", [8, 2, 32, 40])
def test_two_calls_give_identical_bits(ops, J):
    import torch

    bt = batch(21, 130, 200, J, per_series_t=True, distinct=130 if J <= 8 else 6)
    t, c, a, U, V, y = dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
    d, W, flag = ops.factor(t, c, a, U, V)
    z = ops.solve_lower(t, c, U, W, y[..., None].contiguous())[..., 0]
    q1, a1 = ops.inverse_diag(t, c, U, W, d, z=z)
    q2, a2 = ops.inverse_diag(t, c, U, W, d, z=z)
    assert torch.equal(q1, q2) and torch.equal(a1, a2)


def test_graph_capture_of_solve_lower_and_inverse_diag(ops):
    """One torch.cuda.graph capture of solve_lower -> inverse_diag on caller-owned buffers replays correctly on new data."""
    import torch

    bt = batch(31, 12, 257, 8, per_series_t=True, distinct=12)
    t, c, a, U, V, y = dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"], bt["y"])
    d, W, flag = ops.factor(t, c, a, U, V)
    Y = y[..., None].contiguous()
    Z, q = torch.empty_like(Y), torch.empty_like(d)
    alpha = torch.empty_like(d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture
        ops.solve_lower(t, c, U, W, Y, Z=Z)
        ops.inverse_diag(t, c, U, W, d, z=Z[..., 0], q=q, alpha=alpha)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.solve_lower(t, c, U, W, Y, Z=Z)
        ops.inverse_diag(t, c, U, W, d, z=Z[..., 0], q=q, alpha=alpha)
    y2 = torch.from_numpy(np.random.default_rng(32).standard_normal(tuple(y.shape))).cuda()
    Y.copy_(y2[..., None])
    q.zero_(); alpha.zero_()
    graph.replay()
    torch.cuda.synchronize()
    z_e = ops.solve_lower(t, c, U, W, y2[..., None].contiguous())[..., 0]
    q_e, alpha_e = ops.inverse_diag(t, c, U, W, d, z=z_e)
    assert torch.equal(q, q_e) and torch.equal(alpha, alpha_e)
    for b in (0, 11):
        dr = bt["draws"][b]
        K = R.dense(dr["t"], dr["c"], dr["a"], dr["U"], dr["V"])
        check("alpha", alpha[b], np.linalg.solve(K, host(y2[b])), what=("graph", b))


def test_shape_errors(ops):
    import torch

    bt = batch(41, 2, 10, 3, per_series_t=False)
    t, c, a, U, V = dev(bt["t"], bt["c"], bt["a"], bt["U"], bt["V"])
    d, W, flag = ops.factor(t, c, a, U, V)
    with pytest.raises(ValueError, match="Invalid shape: d"):
        ops.inverse_diag(t, c, U, W, d[:, :-1].contiguous())
    with pytest.raises(ValueError, match="Invalid shape: z"):
        ops.inverse_diag(t, c, U, W, d, z=torch.zeros((2, 10, 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="alpha"):
        ops.inverse_diag(t, c, U, W, d, alpha=torch.empty_like(d))
    with pytest.raises(ValueError, match="alias"):
        ops.inverse_diag(t, c, U, W, d, q=d)
    z = torch.zeros_like(d)
    for kw in (dict(z=z, q=z), dict(z=z, alpha=d), dict(z=z, q=(buf := torch.empty_like(d)), alpha=buf)):
        with pytest.raises(ValueError, match="alias"):
            ops.inverse_diag(t, c, U, W, d, **kw)
