# -*- coding: utf-8 -*-
"""GPU checks of the tabulated-shape search under correlated noise: ops.whitened_shapes (c2_whitened_shapes,
csrc/c2_shapes.hip), ops.shape_projections (c2_shape_projections, csrc/c2_trial_project.hip),
GaussianProcess.shape_search and GaussianProcess.shape_search_significance.

References: the numpy restatement of the rule, the sweep and the projection (tests/shapes_ref.py, pinned to dense algebra by
tests/test_shapes.py), fed with the device's own d, W, Z0 and alpha, and two dense generalized-least-squares fits per trial on
the host.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| per element; NaN positions must coincide
exactly.  The restatement takes the kernel's discrete decisions bit for bit, so samples may sit exactly on edges, nodes and
folds."""
import numpy as np
import pytest

import shapes_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = [1, 4, 5, 8, 9, 16, 17, 32]
LENGTHS = [1, 2, 15, 16, 17, 33, 150]   # the 16-row staged block and its tails, from both sides
WORST = {}
RB = 32                                 # C2_SHAPE_DRAWS


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available() and o.SHAPE_DRAWS == RB
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


def batch(seed, B, N, J, Q0, K, per_tc, per_tr, per_sh=False, NS=3, S=9, shift=0.0, **kw):
    """B seeded draws with Y0 = [design(t, Q0 - 1) | y], a trial set and an asymmetric bank each.  per_tc: every series on
    its own grid with its own rates, else all on the first draw's t and c; per_tr: (B, K, 4) trials, else the first draw's;
    per_sh: a (B, NS, S) bank, else the first draw's (NS, S).  shift: added to every time before the trials are made."""
    draws = []
    for k in range(B):
        D = R.draw(1000 * seed + k, N, J, t=None if (per_tc or k == 0) else draws[0]["t"])
        D["Y0"] = np.concatenate([R.design(D["t"], Q0 - 1), D["y"][:, None]], axis=1)
        D["t"] = D["t"] + shift
        D["trials"] = R.trials_for(D["t"], K, NS, seed=seed + k, **kw)
        D["shapes"] = R.bank(NS, S, seed + k)
        draws.append(D)
    st = lambda key: np.stack([D[key] for D in draws])
    return dict(t=st("t") if per_tc else draws[0]["t"], c=st("c") if per_tc else draws[0]["c"], a=st("a"), U=st("U"), V=st("V"),
                Y0=st("Y0"), trials=st("trials") if per_tr else draws[0]["trials"],
                shapes=st("shapes") if per_sh else draws[0]["shapes"])


def run(ops, bt):
    """(T on the device, the batched restatement on the device's own d, W, Z0, the op's device arguments)."""
    import torch

    t, c, a, U, V, Y0, trials, shapes = dev(*[bt[k] for k in ("t", "c", "a", "U", "V", "Y0", "trials", "shapes")])
    d, W, flag = ops.factor(t, c, a, U, V)
    assert int(flag.abs().sum()) == 0
    Z0 = ops.solve_lower(t, c, U, W, Y0)
    T = ops.whitened_shapes(t, c, U, W, d, Z0, trials, shapes)
    torch.cuda.synchronize()
    B, N, J = U.shape
    full = lambda x, n: np.broadcast_to(x, (B,) + x.shape) if x.ndim == n else x
    want = R.whitened_shapes_batched(full(bt["t"], 1), full(bt["c"], 1), bt["U"], host(W), host(d), host(Z0),
                                     full(bt["trials"], 2), bt["shapes"])
    return T, want, (t, c, U, W, d, Z0, trials, shapes)


@pytest.mark.parametrize("J", WIDTHS)
def test_op_vs_restatement(ops, J):
    """Every width on every length at K = 65, Q0 = 2, folded and single events and three asymmetric shapes lane by lane;
    B = 1 and 3, shared and per-series t, c, trials and banks, S = 2, 3, 65 and NS = 1, 3 rotate so that each meets each
    length over the widths."""
    jx = WIDTHS.index(J)
    for i, N in enumerate(LENGTHS):
        B = (1, 3)[(i + jx) % 2]
        per_tc, per_tr, per_sh = bool((i // 2 + jx) % 2), bool((i + jx // 2) % 2), bool((i + jx // 4) % 2)
        S, NS = (2, 3, 65)[(i + jx) % 3], (1, 3)[(i // 3 + jx) % 2]
        T, want, _ = run(ops, batch(10 * J + N, B, N, J, 2, 65, per_tc, per_tr, per_sh, NS=NS, S=S))
        assert tuple(T.shape) == (B, 65, 3)
        check("T vs restatement", T, want, (J, N, B, per_tc, per_tr, per_sh, NS, S))


@pytest.mark.parametrize("J", [3, 32])
def test_lane_tail_and_columns(ops, J):
    """The lane tail, a second and a third wavefront and every accumulator count: K x Q0 at N = 33."""
    for K in (1, 63, 64, 65, 130):
        for Q0 in (1, 2, 3, 8):
            B = 1 + (K + Q0) % 3
            T, want, _ = run(ops, batch(J + K + Q0, B, 33, J, Q0, K, bool(K % 2), bool(Q0 % 2), bool((K + Q0) % 2), S=(3, 65)[Q0 % 2]))
            assert tuple(T.shape) == (B, K, 1 + Q0)
            check("T vs restatement", T, want, (J, K, Q0, B))


def test_bank_limits(ops):
    """NS S = 1024 exactly, as one long shape and as many short ones, shared and per series; NS S = 1025 raises."""
    import torch

    for NS, S, per_sh in ((1, 1024, False), (4, 256, True), (512, 2, False)):
        T, want, ins = run(ops, batch(NS + S, 2, 33, 4, 2, 130, True, True, per_sh, NS=NS, S=S))
        assert set(np.unique(host(ins[6])[..., 3])) == set(range(min(NS, 130)))
        check("T vs restatement, NS S = 1024", T, want, (NS, S))
    t, c, U, W, d, Z0, trials, shapes = ins
    for bank in (torch.ones((1, 1025), dtype=torch.float64, device="cuda"), torch.ones((5, 205), dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match=r"NS \* S <= 1024"):
            ops.whitened_shapes(t, c, U, W, d, Z0, trials, bank)
        with pytest.raises(ValueError, match=r"NS \* S <= 1024"):
            ops.shape_projections(t, Z0, trials, bank)


def exact_case(shift):
    """Times on a grid of eighths and hand-made trials with samples exactly on both edges, on nodes and on a fold, w = P,
    single events before, inside and after the series; asymmetric shapes (a ramp up, a ramp down, a skewed bump)."""
    N, J = 48, 4
    D = R.draw(77, N, J)
    t = np.arange(N) * 0.125 + shift                                                 # (exact beside 2.45e6 as well)
    bank = np.array([[0.0, 0.25, 0.5, 0.75, 1.0], [1.0, 0.5, 0.25, 0.125, 0.0], [0.0, 1.0, 0.5, 0.25, 0.125]])
    tr = [(2.0, 1.0, 0.5, 0.0), (2.0, 1.0, 2.0, 1.0), (0.0, 3.0, 1.0, 2.0), (1.0, 0.5, 0.25, 1.0), (3.0, 0.125, 1.0, 2.0),
          (0.0, 100.0, 1.0, 0.0), (4.0, 0.0, 4.0, 2.0), (0.0, -50.0, 1.0, 1.0), (0.0, 2.5, 6.0, 0.0), (1.5, 0.75, 0.5, 1.0),
          (0.0, 3.0, 1.0, 0.0), (0.0, 3.0, 1.0, 1.0), (1.0, 0.0, 1.0, 0.0), (2.0, 0.5, 1.0, 2.0)]
    trials = np.array(tr * 5)[:65]
    trials[:, 1] += shift
    Y0 = np.concatenate([R.design(t, 1), D["y"][:, None]], axis=1)
    return dict(t=t, c=D["c"], a=D["a"][None], U=D["U"][None], V=D["V"][None], Y0=Y0[None], trials=trials, shapes=bank)


@pytest.mark.parametrize("shift", [0.0, 2.45e6])
def test_exact_edges_nodes_and_folds(ops, shift):
    """Samples exactly on both edges, on nodes and on a fold, w = P, single events, asymmetric shapes (a left / right mix-up
    would swap the two ramps), on times offset by 2.45e6 as well: the restatement takes the same decisions bit for bit, so
    the criterion holds without a margin; and the offset changes no bit."""
    import torch

    bt = exact_case(shift)
    b = R.column(bt["t"], bt["trials"], bt["shapes"])
    x = bt["t"][:, None] - bt["trials"][None, :, 1]
    assert np.any(x[:, 2] == -0.5) and np.any(x[:, 2] == 0.5) and b[x[:, 2] == 0.5, 2][0] == 0.125 and b[x[:, 2] == -0.5, 2][0] == 0.0
    assert np.any(x[:, 10] == -0.25) and b[x[:, 10] == -0.25, 10][0] == 0.25 and b[x[:, 11] == -0.25, 11][0] == 0.5     # on node 1
    assert np.all(b[:, 5] == 0.0) and np.all(b[:, 7] == 0.0) and np.all(b[:, 1] >= 0.0)
    T, want, ins = run(ops, bt)
    check("T vs restatement, exact edges", T, want, shift)
    assert bool((T[:, 5] == 0).all()) and bool((T[:, 7] == 0).all())
    if shift:
        T0, _, _ = run(ops, exact_case(0.0))
        assert torch.equal(T, T0)


@pytest.mark.parametrize("J", [2, 8, 32])
def test_box_bank_meets_whitened_transits(ops, J):
    """With the all-ones S = 2 bank the op meets ops.whitened_transits(tau = 0) within the criterion (the column is the same
    to the bit; whether the sums are is reported)."""
    import torch

    bt = batch(40 + J, 3, 150, J, 2, 130, True, True, NS=1, S=2, shift=2.45e6 if J == 8 else 0.0)
    bt["shapes"] = np.ones((1, 2))
    T, want, ins = run(ops, bt)
    check("T vs restatement, box bank", T, want, J)
    assert bool((ins[6][..., 3] == 0).all())                                         # (s = 0 doubles as tau = 0)
    Tt = ops.whitened_transits(*ins[:7])
    torch.cuda.synchronize()
    check("box bank vs whitened_transits", T, host(Tt), J)
    print("box bank vs whitened_transits(tau = 0), J = %d: bit-identical = %s" % (J, bool(torch.equal(T, Tt))))


@pytest.mark.parametrize("J,N,K,Q0", [(2, 9, 5, 1), (8, 33, 65, 2), (32, 150, 130, 8)])
def test_plain_call_properties_and_graph(ops, J, N, K, Q0):
    """Two calls give identical bits, a caller-owned `out` gives the same bits, so does a call captured in a graph and
    replayed (both ops); inputs are unchanged; `out` may not alias an input; a mis-shaped input is refused."""
    import torch

    T0, want, ins = run(ops, batch(50 + J, 3, N, J, Q0, K, True, True, True, S=65))
    before = [x.clone() for x in ins]
    T1 = ops.whitened_shapes(*ins)
    own = torch.full((3, K, 1 + Q0), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.whitened_shapes(*ins, out=own) is own
    t, c, U, W, d, Z0, trials, shapes = ins
    alpha = Z0                                                  # (any (B, N, R) array serves the projection)
    P0 = ops.shape_projections(t, alpha, trials, shapes)
    P1 = ops.shape_projections(t, alpha, trials, shapes)
    pown = torch.full((3, K, 1, Q0), float("nan"), dtype=torch.float64, device="cuda")
    assert ops.shape_projections(t, alpha, trials, shapes, out=pown) is pown
    torch.cuda.synchronize()
    assert torch.equal(T0, T1) and torch.equal(T0, own) and torch.equal(P0, P1) and torch.equal(P0, pown)
    assert all(torch.equal(x, y) for x, y in zip(ins, before))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.whitened_shapes(*ins, out=own)                      # (warm-up on the capturing stream)
        ops.shape_projections(t, alpha, trials, shapes, out=pown)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                   # (two kernel nodes in sequence: no parallel branches)
        ops.whitened_shapes(*ins, out=own)
        ops.shape_projections(t, alpha, trials, shapes, out=pown)
    torch.cuda.synchronize()
    for _ in range(2):
        own.zero_()
        pown.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(own, T0) and torch.equal(pown, P0)
    pool = torch.zeros(max(own.numel(), Z0.numel()), dtype=torch.float64, device="cuda")
    pool[:Z0.numel()] = Z0.reshape(-1)
    with pytest.raises(ValueError, match="out must not alias Z0"):
        ops.whitened_shapes(t, c, U, W, d, pool[:Z0.numel()].view(Z0.shape), trials, shapes, out=pool[:own.numel()].view(own.shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.whitened_shapes(t, c, U, W, d, Z0, trials, shapes.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match="Invalid shape: trials"):
        ops.whitened_shapes(t, c, U, W, d, Z0, trials[:2], shapes)
    with pytest.raises(ValueError, match="Invalid shape: shapes"):
        ops.whitened_shapes(t, c, U, W, d, Z0, trials, shapes[:2])
    with pytest.raises(ValueError, match="Invalid shape: out"):
        ops.shape_projections(t, alpha, trials, shapes, out=pown[..., :-1].contiguous())


def test_unsupported_sizes(ops):
    """J = 33 and Q0 = 9 return C2_ERR_UNSUPPORTED through ops (a ValueError naming the op), before any launch."""
    import torch

    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="whitened_shapes: width not supported"):
        ops.whitened_shapes(z(5), z(33), z(1, 5, 33), z(1, 5, 33), z(1, 5) + 1, z(1, 5, 2), z(3, 4), z(1, 2))
    with pytest.raises(ValueError, match="whitened_shapes: width not supported"):
        ops.whitened_shapes(z(5), z(2), z(1, 5, 2), z(1, 5, 2), z(1, 5) + 1, z(1, 5, 9), z(3, 4), z(1, 2))


# ---- the front end ---------------------------------------------------------------------------------------------------------
MEAN = 0.3


def gp_case(B, N, seed=1, K=40, NS=3, S=17):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 30.0, (B, N)), axis=1)
    diag = rng.uniform(0.05, 0.3, (B, N))
    A = np.stack([np.ones_like(x), x / 30.0 - 0.5, (x / 30.0 - 0.5) ** 2], axis=2)
    trials = np.stack([R.trials_for(x[b], K, NS, seed=seed + b) for b in range(B)])
    bank = R.bank(NS, S, seed)
    dip = np.stack([R.column(x[b], trials[b, :1], bank)[:, 0] for b in range(B)])
    y = -1.5 * dip + 0.3 * rng.standard_normal((B, N)) + MEAN + A @ np.array([0.5, -2.0, 1.0])
    return x, diag, A, y, trials, bank


def make_gp(xd, dd, J=3, **kw):
    import torch
    from celerite2_amd import gp as G, terms as T

    tn = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")
    kernel = T.SHOTerm(S0=tn(0.4), w0=tn(0.9), Q=tn(2.5), regime="under") + T.RealTerm(a=tn(0.2), c=0.3)         # J = 3
    if J == 8:
        kernel = kernel + T.SHOTerm(S0=tn(0.2), w0=tn(2.3), Q=tn(4.0), regime="under") + T.SHOTerm(S0=tn(0.1), w0=tn(4.1), Q=tn(1.5), regime="under") \
            + T.RealTerm(a=tn(0.1), c=1.1)
    gp = G.GaussianProcess(kernel, mean=tn(MEAN))
    gp.compute(xd, diag=dd, **kw)
    assert gp._U.shape[-1] == J
    return gp


def dense_of(gp, x, b):
    c = host(gp._c)
    return R.dense(x[b], c[b] if c.ndim == 2 else c, host(gp._a)[b], host(gp._U)[b], host(gp._V)[b])


def test_index_safety(ops):
    """The shape index is clamped, never trusted.  The bank sits inside a larger allocation between NaN guard words; single
    trials carry the indices -1, NS, 0.5 and NaN (no huge values).  Their T is finite -- they read shape 0, and a read of the
    guards would show as NaN, without any fault -- and equals shape 0's; shape_search masks them to NaN; every other trial
    keeps the bits of a run without them."""
    import torch

    B, N, K, NS, S = 2, 150, 70, 3, 9
    x, diag, A, y, trials, bank = gp_case(B, N, seed=3, K=K, NS=NS, S=S)
    pool = torch.full((64 + NS * S + 64,), float("nan"), dtype=torch.float64, device="cuda")
    guarded = pool[64:64 + NS * S].view(NS, S)
    guarded.copy_(torch.from_numpy(bank))
    assert guarded.is_contiguous() and guarded.data_ptr() == pool.data_ptr() + 64 * 8
    odd = {5: -1.0, 17: float(NS), 40: 0.5, 66: float("nan")}
    bad, zero = trials.copy(), trials.copy()
    for k, s in odd.items():
        bad[:, k, 3], zero[:, k, 3] = s, 0.0
    xd, dd, yd, td, bd, zd = dev(x, diag, y, trials, bad, zero)
    gp = make_gp(xd, dd)
    Z0 = gp._whitened_columns(yd, "mean")
    sweep = lambda tr: ops.whitened_shapes(gp._t, gp._c, gp._U, gp._W, gp._d, Z0, tr, guarded)
    T, Tb, Tz = sweep(td), sweep(bd), sweep(zd)
    alpha = gp.apply_inverse(yd - MEAN)[..., None].contiguous()
    Pb, Pz = ops.shape_projections(xd, alpha, bd, guarded), ops.shape_projections(xd, alpha, zd, guarded)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Tb).all()) and bool(torch.isfinite(Pb).all())
    assert torch.equal(Tb, Tz) and torch.equal(Pb, Pz)                               # clamped to shape 0, to the bit
    keep = np.array([k not in odd for k in range(K)])
    assert torch.equal(Tb[:, keep], T[:, keep])
    assert bool(torch.isnan(pool[:64]).all()) and bool(torch.isnan(pool[64 + NS * S:]).all())
    clean = gp.shape_search(yd, td, guarded, return_fit=True)
    got = gp.shape_search(yd, bd, guarded, return_fit=True)
    for f, g in zip(got[:4], clean[:4]):
        assert bool(torch.isnan(f[:, ~keep]).all()) and bool(torch.isfinite(g).all())
        assert torch.equal(f[:, keep], g[:, keep])
    assert torch.equal(got.chi2_null, clean.chi2_null)


def test_nan_trials_and_failed_series(ops):
    """A NaN P, t0 or w in a trial, and a series failing its factorisation under compute(quiet=True): NaN there, the
    neighbours keep their bits."""
    import torch

    B, N, K = 3, 33, 40
    x, diag, A, y, trials, bank = gp_case(B, N, seed=9, K=K)
    bad_tr, bad_diag = trials.copy(), diag.copy()
    bad_tr[:, 4, 0], bad_tr[:, 11, 1], bad_tr[:, 30, 2] = np.nan, np.nan, np.nan
    bad_diag[1, 7] = -50.0                                                           # not positive definite from row 7 on
    xd, dd, bdd, yd, td, btd, sd = dev(x, diag, bad_diag, y, trials, bad_tr, bank)
    clean = make_gp(xd, dd).shape_search(yd, td, sd, return_fit=True)
    assert all(bool(torch.isfinite(v).all()) for v in clean)
    got = make_gp(xd, dd).shape_search(yd, btd, sd, return_fit=True)
    keep = np.array([k not in (4, 11, 30) for k in range(K)])
    for f, g in zip(got[:4], clean[:4]):
        assert bool(torch.isnan(f[:, ~keep]).all()) and torch.equal(f[:, keep], g[:, keep])
    fit = make_gp(xd, bdd, quiet=True).shape_search(yd, td, sd, return_fit=True)
    for f, g in zip(fit, clean):
        assert bool(torch.isnan(f[1]).all()) and torch.equal(f[0], g[0]) and torch.equal(f[2], g[2])
    normals = torch.randn((B, N, 6), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    sig_clean = make_gp(xd, dd).shape_search_significance(yd, td, sd, normals=normals)
    sig = make_gp(xd, bdd, quiet=True).shape_search_significance(yd, td, sd, normals=normals)
    for f, g in zip(sig, sig_clean):
        assert bool(torch.isnan(f[1]).all()) and bool(torch.isfinite(g).all())
        assert torch.equal(f[0], g[0]) and torch.equal(f[2], g[2])


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 17, 150])
def test_projections_vs_restatement(ops, N):
    """ops.shape_projections against the restatement (np.longdouble sums) fed the device's own alpha: K x R around the 16
    trials and the RB draws of a wavefront, B = 1 and 3, shared and per-series t, trials and banks, S = 2, 9, 65."""
    import torch

    for i, K in enumerate((1, 15, 16, 17, 33)):
        for j, Rn in enumerate((1, 15, 16, 17, RB - 1, RB, RB + 1)):
            B = (1, 3)[(i + j) % 2]
            per_tc, per_tr, per_sh = bool((i + j // 2) % 2), bool((i // 2 + j) % 2), bool((i + j // 4) % 2)
            bt = batch(100 * N + 10 * i + j, B, N, 3, 1, K, per_tc, per_tr, per_sh, S=(2, 9, 65)[(i + j) % 3],
                       shift=2.45e6 if (i + j) % 4 == 3 else 0.0)
            t, c, a, U, V, trials, shapes = dev(*[bt[k] for k in ("t", "c", "a", "U", "V", "trials", "shapes")])
            d, W, flag = ops.factor(t, c, a, U, V)
            nrm = torch.from_numpy(np.random.default_rng(N + i + j).normal(size=(B, N, Rn))).cuda()
            alpha = ops.solve_upper(t, c, U, W, (nrm * torch.rsqrt(d)[..., None]).contiguous())
            P = ops.shape_projections(t, alpha, trials, shapes)
            assert tuple(P.shape) == (B, K, 1, Rn)
            check("P vs restatement", P, R.projections_batched(bt["t"], host(alpha), bt["trials"], bt["shapes"]), (N, K, Rn, B))


def test_projection_is_the_sweeps_gty(ops):
    """With alpha = apply_inverse(y - mean), P[..., 0] is the entry gty of the sweep's own T."""
    B, N, K = 3, 120, 40
    x, diag, A, y, trials, bank = gp_case(B, N, K=K, S=65)
    xd, dd, yd, td, Ad, sd = dev(x, diag, y, trials, A, bank)
    gp = make_gp(xd, dd)
    alpha = gp.apply_inverse(yd - MEAN)[..., None].contiguous()
    P = ops.shape_projections(xd, alpha, td, sd)
    T = ops.whitened_shapes(gp._t, gp._c, gp._U, gp._W, gp._d, gp._whitened_columns(yd, Ad), td, sd)
    check("P vs the sweep's gty", P[:, :, 0, 0], host(T[:, :, 1 + 3]))
    for b in range(B):
        Y0 = np.concatenate([A[b], (y[b] - MEAN)[:, None]], axis=1)
        want = R.dense_products(dense_of(gp, x, b), x[b], Y0, trials[b], bank)
        check("P vs dense gty", P[b, :, 0, 0], want[:, 4], b)
        check("T vs dense products", T[b], want, b)


@pytest.mark.parametrize("J", [3, 8])
@pytest.mark.parametrize("design", ["mean", None, "batched3"])
def test_gp_shape_search_vs_dense(ops, design, J):
    """gp.shape_search with return_fit against two dense GLS fits per trial on the host at B = 3, N = 150, P0 = 1, 0 and 3;
    shared and per-series trials and banks, a tensor mean; the plain call returns delta_chi2."""
    import torch
    from celerite2_amd import shapes as sh

    B, N, K = 3, 150, 40
    x, diag, A, y, trials, bank = gp_case(B, N)
    x[...] = x[0]                                      # (one time grid, so that a shared trial set has midpoint edges everywhere)
    trials[...] = trials[0]
    if design == "batched3":
        A = A * (1.0 + 0.5 * np.arange(B))[:, None, None]
    xd, dd, Ad, yd = dev(x, diag, A, y)
    gp = make_gp(xd, dd, J)
    use = {"mean": "mean", None: None, "batched3": Ad}[design]
    A0 = {"mean": A[..., :1] * 0 + 1, None: A[..., :0], "batched3": A}[design]
    for trs, bnk in ((trials, bank), (trials[0], np.stack([bank] * B))):
        td, sd = dev(trs, bnk)
        want = [R.dense_search(dense_of(gp, x, b), x[b], A0[b], y[b] - MEAN, trials[0], bank) for b in range(B)]
        dchi2, amp, aerr, chi2_0 = [np.stack([w[k] for w in want]) for k in range(4)]
        fit = gp.shape_search(yd, td, sd, A=use, return_fit=True)
        assert isinstance(fit, sh.ShapeSearch)
        assert all(tuple(v.shape) == (B, K) for v in fit[:4]) and tuple(fit.chi2_null.shape) == (B,)
        what = (design, J, trs.ndim)
        check("gp delta_chi2 vs dense", fit.delta_chi2, dchi2, what)
        check("gp amplitude vs dense", fit.amplitude, amp, what)
        check("gp amplitude_err vs dense", fit.amplitude_err, aerr, what)
        check("gp snr vs dense", fit.snr, amp / aerr, what)
        check("gp chi2_null vs dense", fit.chi2_null, chi2_0, what)
        assert torch.equal(gp.shape_search(yd, td, sd, A=use), fit.delta_chi2)


@pytest.mark.parametrize("nm", ["standard", "chi2", "log_likelihood"])
def test_significance_vs_loop(ops, nm):
    """Eight given normals: null_maxima against the loop y_r = mean + L D^1/2 n_r (dot_tril) -> shape_search -> the largest
    normalised delta_chi2; the statistic is shape_search's, to the bit; fap is the count."""
    import torch
    from celerite2_amd import significance as sg

    B, N, K, Rn = 2, 60, 20, 8
    x, diag, A, y, trials, bank = gp_case(B, N, seed=3, K=K)
    normals = np.random.default_rng(5).normal(size=(B, N, Rn))
    xd, dd, yd, td, nd, sd = dev(x, diag, y, trials, normals, bank)
    gp = make_gp(xd, dd)
    norm = lambda fit: {"standard": fit.delta_chi2 / fit.chi2_null[:, None], "chi2": fit.delta_chi2, "log_likelihood": 0.5 * fit.delta_chi2}[nm]
    got = gp.shape_search_significance(yd, td, sd, normalization=nm, normals=nd)
    assert isinstance(got, sg.Significance) and tuple(got.statistic.shape) == tuple(got.fap.shape) == (B, K)
    assert tuple(got.null_maxima.shape) == (B, Rn)
    assert torch.equal(got.statistic, norm(gp.shape_search(yd, td, sd, return_fit=True)))
    loop = []
    for r in range(Rn):
        yr = MEAN + gp.dot_tril(nd[..., r].contiguous())
        stat = norm(gp.shape_search(yr, td, sd, return_fit=True))
        assert bool(torch.isfinite(stat).all())
        loop.append(host(stat).max(axis=1))
    check("null_maxima vs the loop of shape_search", got.null_maxima, np.stack(loop, axis=1), nm)
    stat = host(got.statistic)
    want = (1 + (host(got.null_maxima)[:, None, :] >= (stat - 1e-10 * np.abs(stat))[:, :, None]).sum(-1)) / (Rn + 1)
    assert np.array_equal(host(got.fap), want)


def test_significance_injected_chunking_and_box(ops):
    """A strong injected event has fap = 1 / (R + 1) at its peak; max_trials gives the same bits and max_draws the criterion;
    dips_only zeroes the positive amplitudes; with the box bank the result meets search_significance("transit", ...) on
    the same normals."""
    import torch

    B, N, K, Rn = 2, 80, 37, 70
    x, diag, A, y, trials, bank = gp_case(B, N, seed=6, K=K)
    y = y - 30.0 * np.stack([R.column(x[b], trials[b, 11:12], bank)[:, 0] for b in range(B)])
    xd, dd, yd, td, sd, Ad = dev(x, diag, y, trials, bank, A)
    gp = make_gp(xd, dd)
    normals = torch.randn((B, N, Rn), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    whole = gp.shape_search_significance(yd, td, sd, normals=normals)
    assert host(whole.statistic).argmax(axis=1).tolist() == [11, 11]
    assert host(whole.fap)[:, 11].tolist() == [1.0 / (Rn + 1)] * B
    assert bool(torch.isfinite(whole.null_maxima).all())
    drawn = gp.shape_search_significance(yd, td, sd, draws=19, generator=torch.Generator(device="cuda").manual_seed(1))
    assert tuple(drawn.null_maxima.shape) == (B, 19) and host(drawn.fap)[:, 11].tolist() == [1.0 / 20] * B
    for max_trials in (1, 16, K - 1, K, 10 ** 6):
        part = gp.shape_search_significance(yd, td, sd, normals=normals, max_trials=max_trials)
        assert all(torch.equal(a, b) for a, b in zip(part, whole)), max_trials
    for max_draws in (1, 33, Rn - 1):
        part = gp.shape_search_significance(yd, td, sd, normals=normals, max_draws=max_draws, max_trials=20)
        assert torch.equal(part.statistic, whole.statistic)
        check("null_maxima under max_draws", part.null_maxima, host(whole.null_maxima), max_draws)
    dips = gp.shape_search_significance(yd, td, sd, normals=normals, dips_only=True, normalization="chi2")
    fit = gp.shape_search(yd, td, sd, return_fit=True)
    assert torch.equal(dips.statistic, torch.where(fit.amplitude > 0, torch.zeros_like(fit.delta_chi2), fit.delta_chi2))
    assert bool((dips.statistic[fit.amplitude > 0] == 0).all()) and bool((fit.amplitude > 0).any())
    # the box bank against the transit branch (s = 0 doubles as tau = 0)
    boxes = td.clone()
    boxes[..., 3] = 0.0
    ones = torch.ones((1, 2), dtype=torch.float64, device="cuda")
    for kw in (dict(), dict(A=Ad, normalization="chi2", dips_only=True)):
        a = gp.shape_search_significance(yd, boxes, ones, normals=normals, **kw)
        b = gp.search_significance("transit", yd, boxes, normals=normals, **kw)
        check("box bank vs search_significance(transit): statistic", a.statistic, host(b.statistic))
        check("box bank vs search_significance(transit): null_maxima", a.null_maxima, host(b.null_maxima))
        assert torch.equal(a.fap, b.fap)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
