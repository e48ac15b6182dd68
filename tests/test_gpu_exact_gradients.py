# -*- coding: utf-8 -*-
"""Every device gradient path against the EXACT gradient (oracle/exact.py), not against the CPU restatement: closed forms
on the dense matrix up to N = 1000, complex-step derivatives of analytic forwards below that and, on long series where
dense algebra is out of reach, complex-step directional derivatives of the O(N) recursions.

Tolerance: the project's `close` -- 1e-10 relative per element plus a floor of 1e-12 of the array's largest entry.  The
worst |err| / max |g| of each path is collected in WORST (written to the JSON file named by C2_EXACT_REPORT, if set)."""
import json
import os

import numpy as np
import pytest

from oracle import dense
from oracle import exact as ex
from test_exact_gradients import coeffs, series

pytestmark = pytest.mark.gpu
TOL, FLOOR = 1e-10, 1e-12
MAT = ("bt", "bc", "ba", "bU", "bV", "by")
COEF = ("bar", "bcr", "bac", "bbc", "bcc", "bdc", "bx", "bdiag", "by")
SWEEPS = ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper")
KNOBS = ("C2_LANES", "C2_LOGLIK_BACK", "C2_TIMEPAR_GRAD", "C2_TPG_ROWS", "C2_REV_LONG", "C2_KRON_BANDED", "C2_TERMS_FUSED",
         "C2_TERMS_TWO_LANES", "C2_TERMS_FOUR_LANES", "C2_TERMS_EIGHT_LANES")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("C2_EXACT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(WORST.items())), f, indent=1)


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture
def env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def set_(**kv):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in kv.items():
            monkeypatch.setenv(k, v)
    return set_


def dev(*xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def close(path, got, want, names):
    """The project's criterion, element by element; the worst distance relative to the largest entry is recorded."""
    for nm, g, w in zip(names, got, want):
        g, w = host(g), np.asarray(w)
        if w.size == 0:
            continue
        WORST[path] = max(WORST.get(path, 0.0), ex.relerr(g, w))
        np.testing.assert_allclose(g, w, rtol=TOL, atol=FLOOR * max(1.0, float(np.abs(w).max())), err_msg="%s %s" % (path, nm))


# ---- inputs and their exact gradients -------------------------------------------------------------------------
DISTINCT = 7   # series drawn per batch; series b is draw b % 7, so neighbours in a wavefront always differ


def batch(B, N, J, seed=0, distinct=DISTINCT):
    k = min(B, distinct)
    draws = [series(N, J, seed=1000 * seed + 31 * N + J + i) for i in range(k)]
    return [np.ascontiguousarray(np.stack([draws[b % k][i] for b in range(B)])) for i in range(6)], k


_EXACT = {}


def _exact_one(args):
    key = b"".join(np.ascontiguousarray(x).tobytes() for x in args)
    if key not in _EXACT:
        _EXACT[key] = ex.loglik_grad(*args)
    return _EXACT[key]


def exact_batch(arrs, k):
    """Exact ll (B,) and gradients (B, ...) of a batch whose series repeat with period k (memoised: the same draws run on
    every path)."""
    B = arrs[0].shape[0]
    res = [_exact_one([x[i] for x in arrs]) for i in range(k)]
    ll = np.array([res[b % k][0] for b in range(B)])
    return ll, [np.stack([res[b % k][1][i] for b in range(B)]) for i in range(6)]


def run_loglik_grad(ops, path, arrs, k, shared=False):
    t, c, a, U, V, y = arrs
    if shared:
        t0, c0 = t[0].copy(), c[0].copy()
        ll, grads, flag = ops.loglik_grad(*dev(t0, c0, a, U, V, y))
    else:
        ll, grads, flag = ops.loglik_grad(*dev(t, c, a, U, V, y))
    assert int(flag.abs().sum()) == 0
    llx, gx = exact_batch(arrs, k)
    close(path, [ll], [llx], ["ll"])
    close(path, grads, gx, MAT)


SHAPES = [(1, 1), (7, 2), (7, 3), (65, 8), (70, 9), (7, 16), (65, 17), (7, 31), (70, 32), (7, 33), (7, 63), (65, 64),
          (7, 65), (7, 127), (7, 300), (2, 1000)]
LANES = {"1": (2, 4, 6, 8), "2": (8,), "4": (8,), "8": (1, 2, 3, 4, 5, 6, 7, 8)}


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("lanes,J", [(l, j) for l, js in LANES.items() for j in js])
def test_loglik_grad_lane_mappings_vs_exact(ops, env, lanes, J, B, N):
    arrs, k = batch(B, N, J)
    env(C2_LANES=lanes, C2_TIMEPAR_GRAD="0")
    run_loglik_grad(ops, "loglik_grad C2_LANES=%s" % lanes, arrs, k)
    if lanes == "8":      # the replay instead of the backward recursion
        env(C2_LANES=lanes, C2_TIMEPAR_GRAD="0", C2_LOGLIK_BACK="0")
        run_loglik_grad(ops, "loglik_grad C2_LANES=8 C2_LOGLIK_BACK=0", arrs, k)


@pytest.mark.parametrize("B,N", [(1, 1), (2, 2), (3, 63), (2, 64), (2, 65), (1, 127), (7, 129), (2, 300), (1, 1000)])
@pytest.mark.parametrize("J", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("rows", ["16", "32", "64"])
def test_loglik_grad_time_parallel_vs_exact(ops, env, rows, J, B, N):
    arrs, k = batch(B, N, J, seed=1)
    env(C2_TIMEPAR_GRAD="1", C2_TPG_ROWS=rows)
    run_loglik_grad(ops, "loglik_grad C2_TIMEPAR_GRAD=1", arrs, k)


@pytest.mark.parametrize("B,N", [(1, 1), (7, 9), (65, 33), (3, 300), (1, 1000)])
@pytest.mark.parametrize("J", [1, 2, 3, 5, 8, 12, 16, 32])
def test_loglik_grad_default_and_composite_vs_exact(ops, env, J, B, N):
    arrs, k = batch(B, N, J, seed=2)
    env()
    run_loglik_grad(ops, "loglik_grad default dispatch", arrs, k)
    ll, grads, flag = ops._loglik_grad_composite(*dev(*arrs))
    assert int(flag.abs().sum()) == 0
    llx, gx = exact_batch(arrs, k)
    close("loglik_grad composite", [ll], [llx], ["ll"])
    close("loglik_grad composite", grads, gx, MAT)


# ---- inputs where kernels go wrong -----------------------------------------------------------------------------
EDGE_PATHS = {"default": {}, "lanes8": dict(C2_LANES="8", C2_TIMEPAR_GRAD="0"),
              "lanes8 replay": dict(C2_LANES="8", C2_TIMEPAR_GRAD="0", C2_LOGLIK_BACK="0"),
              "lanes4": dict(C2_LANES="4", C2_TIMEPAR_GRAD="0"), "lanes2": dict(C2_LANES="2", C2_TIMEPAR_GRAD="0"),
              "lanes1": dict(C2_LANES="1", C2_TIMEPAR_GRAD="0"), "timepar": dict(C2_TIMEPAR_GRAD="1")}


def _edge(case, B, N, J):
    """A batch of 7 distinct series (repeated to B) on a grid with the named difficulty; the matrices follow the grid."""
    k = min(B, DISTINCT)
    rng = np.random.default_rng(11)
    t, c, a, U, V, y = (np.empty((B, N)), np.empty((B, J)), np.empty((B, N)), np.empty((B, N, J)), np.empty((B, N, J)),
                        np.empty((B, N)))
    for i in range(k):
        co = dense.sho_sum_coeffs(J, 0.1 * i)
        cmax = float(np.max(co.cc))
        ti = np.sort(rng.uniform(0, N / 10.0, N))
        if case == "ties":
            for n0 in (1, 8, 31, 32, 63, 64, N - 1):
                ti[n0] = ti[n0 - 1]
        elif case == "underflow gap":
            ti[N // 3:] += 1e6                 # exp(-c * gap) underflows to zero: independent blocks
            if i % 2:
                ti[2 * N // 3:] += 5e5
        elif case.startswith("guard"):
            # a uniform grid whose segments of 32 (or 8) rows have max_j c_j * span just inside / just outside 2.0
            g, rows = {"guard 1.9/32": (1.9, 32), "guard 2.1/32": (2.1, 32), "guard 1.9/8": (1.9, 8),
                       "guard 2.1/8": (2.1, 8)}[case]
            dt = 1.9 / (cmax * rows) if g < 2 else 2.1 / (cmax * (rows - 1))
            ti = dt * (np.arange(N) + 0.02 * rng.uniform(-1, 1, N))
        else:
            raise ValueError(case)
        ci, ai, Ui, Vi = dense.celerite_matrices(co, ti, rng.uniform(0.1, 0.3, N))
        yi = np.sin(ti) + 0.1 * rng.standard_normal(N)
        for b in range(i, B, k):
            t[b], c[b], a[b], U[b], V[b], y[b] = ti, ci, ai + 1.0, Ui, Vi, yi
    return [t, c, a, U, V, y], k


@pytest.mark.parametrize("case", ["ties", "underflow gap", "guard 1.9/32", "guard 2.1/32", "guard 1.9/8", "guard 2.1/8"])
@pytest.mark.parametrize("path", sorted(EDGE_PATHS))
def test_loglik_grad_hard_inputs_vs_exact(ops, env, path, case):
    J = 8
    arrs, k = _edge(case, 70, 300, J)
    env(**EDGE_PATHS[path])
    run_loglik_grad(ops, "loglik_grad %s (hard inputs)" % path, arrs, k)
    if path in ("lanes1", "default"):       # widths the one-lane mapping takes besides 8
        arrs4, k4 = _edge(case, 70, 300, 4)
        run_loglik_grad(ops, "loglik_grad %s (hard inputs)" % path, arrs4, k4)


@pytest.mark.parametrize("path", sorted(EDGE_PATHS))
@pytest.mark.parametrize("B,N", [(70, 33), (7, 300)])
def test_loglik_grad_shared_grid_vs_exact(ops, env, path, B, N):
    """1-D t and c: one grid and one set of rates for the batch, a data vector per series."""
    J = 8
    arrs, _ = batch(1, N, J, seed=4)
    rng = np.random.default_rng(N)
    t, c, a, U, V, y = (np.repeat(x, B, axis=0) for x in arrs)
    y0 = y[:DISTINCT] + 0.3 * rng.standard_normal((DISTINCT, N))
    y = np.ascontiguousarray(y0[np.arange(B) % DISTINCT])
    env(**EDGE_PATHS[path])
    run_loglik_grad(ops, "loglik_grad %s (shared t, c)" % path, [t, c, a, U, V, y], DISTINCT, shared=True)


@pytest.mark.parametrize("path", ["default", "lanes8", "lanes4", "lanes2", "lanes1", "timepar"])
def test_loglik_grad_bench_generator_vs_exact(ops, env, path):
    """The benchmark's own series (celerite2_amd.synth.host_inputs), a third of them with a gap."""
    from celerite2_amd import synth
    B, N, J = 70, 200, 8
    t, diag, y, ac, bc, cc, dc = synth.host_inputs(0, DISTINCT, N, J, gap_fraction=0.3)
    rows = [dense.celerite_matrices(dense.Coeffs(ac=ac[i], bc=bc[i], cc=cc[i], dc=dc[i]), t[i], diag[i]) for i in range(DISTINCT)]
    pick = np.arange(B) % DISTINCT
    arrs = [np.ascontiguousarray(x) for x in (t[pick], np.stack([r[0] for r in rows])[pick],
                                              np.stack([r[1] for r in rows])[pick], np.stack([r[2] for r in rows])[pick],
                                              np.stack([r[3] for r in rows])[pick], y[pick])]
    env(**EDGE_PATHS[path])
    run_loglik_grad(ops, "loglik_grad %s (bench generator)" % path, arrs, DISTINCT)


# ---- anchored to the reference's fixtures ----------------------------------------------------------------------
FIXTURES = ["cpp_%s_" % k for k in ("real", "complex", "sho1", "sho2", "sum1", "sum2", "sum3", "sum4")] + \
           ["py_", "gp8a_", "gp8b_", "gprot_"]


def _fixture(golden, p):
    g = {k[len(p):]: v for k, v in golden.items() if k.startswith(p)}
    x, c, a, U, V = (np.ascontiguousarray(g[k]) for k in ("x", "c", "a", "U", "V"))
    if "K" in g:
        y = np.ascontiguousarray(g["Y"][:, 0]); K = g["K"]
    else:
        y = np.ascontiguousarray(g["y"] - g["mean"])
        K = ex.terms_dense(*[np.atleast_1d(g["coef_" + n]) for n in ("ar", "cr", "ac", "bc", "cc", "dc")], x, g["diag"])
    return (x, c, a, U, V, y), K


@pytest.mark.parametrize("path", sorted(EDGE_PATHS) + ["composite"])
@pytest.mark.parametrize("p", FIXTURES)
def test_loglik_grad_reference_fixtures_vs_exact(ops, env, golden, p, path):
    """70 copies (whole and partial groups of 64) against the gradient from the reference's own K where it is stored, else
    from K built on the reference term classes' coefficients."""
    one, K = _fixture(golden, p)
    llx, gx = ex.loglik_grad_from_K(K, one[5], one[0], one[1], one[3], one[4])
    B = 70
    arrs = [np.ascontiguousarray(np.repeat(x[None], B, axis=0)) for x in one]
    if path == "composite":
        ll, grads, flag = ops._loglik_grad_composite(*dev(*arrs))
    else:
        env(**EDGE_PATHS[path])
        ll, grads, flag = ops.loglik_grad(*dev(*arrs))
    assert int(flag.abs().sum()) == 0
    name = "loglik_grad %s (reference fixtures)" % path
    close(name, [ll], [np.full(B, llx)], ["ll"])
    close(name, grads, [np.repeat(g[None], B, axis=0) for g in gx], MAT)


# ---- the coefficient level ------------------------------------------------------------------------------------
TERMS_PATHS = {"composed": {}, "one": dict(C2_TERMS_FUSED="1"), "two": dict(C2_TERMS_TWO_LANES="1"),
               "four": dict(C2_TERMS_FOUR_LANES="1"), "eight": dict(C2_TERMS_EIGHT_LANES="1")}


def _force_terms(env, which):
    kv = {k: "0" for k in ("C2_TERMS_FUSED", "C2_TERMS_TWO_LANES", "C2_TERMS_FOUR_LANES", "C2_TERMS_EIGHT_LANES")}
    kv.update(TERMS_PATHS[which])
    env(**kv)


def _terms_exact(co, x, diag, y, k):
    B = len(y)
    res = [ex.terms_grad(*[v[i] for v in co], x[i], diag[i], y[i]) for i in range(k)]
    return np.array([res[b % k][0] for b in range(B)]), [np.stack([res[b % k][1][i] for b in range(B)]) for i in range(9)]


@pytest.mark.parametrize("B,N", [(1, 1), (65, 33), (70, 64), (7, 300)])
@pytest.mark.parametrize("Jr,Jc", [(0, 4), (2, 3), (0, 2), (2, 1), (0, 1), (2, 0), (1, 1), (3, 1), (1, 2)])
@pytest.mark.parametrize("which", sorted(TERMS_PATHS))
def test_loglik_terms_grad_vs_exact(ops, env, which, Jr, Jc, B, N):
    rng = np.random.default_rng(100 * Jr + 10 * Jc + N)
    k = min(B, DISTINCT)
    draws = [coeffs(Jr, Jc, rng) for _ in range(k)]
    co = [np.ascontiguousarray(np.stack([draws[b % k][i] for b in range(B)])) for i in range(6)]
    x0 = np.sort(rng.uniform(0, N / 10.0, (k, N)), axis=1)
    d0 = rng.uniform(0.1, 0.3, (k, N)) + 0.5
    y0 = np.sin(x0) + 0.1 * rng.standard_normal((k, N))
    pick = np.arange(B) % k
    x, diag, y = x0[pick], d0[pick], y0[pick]
    _force_terms(env, which)
    ll, grads, flag = ops.loglik_terms_grad(*dev(*co, x, diag, y))
    assert int(flag.abs().sum()) == 0
    llx, gx = _terms_exact(co, x, diag, y, k)
    path = "loglik_terms_grad %s" % which
    close(path, [ll], [llx], ["ll"])
    close(path, grads, gx, COEF)


# ---- Kronecker -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("banded", ["0", "1"])
@pytest.mark.parametrize("method", ["collapsed", "interleaved"])
@pytest.mark.parametrize("N,M,J", [(16, 3, 2), (40, 4, 4), (64, 2, 6), (7, 1, 2), (30, 5, 3), (100, 3, 8)])
def test_kron_loglik_grad_vs_exact(ops, env, N, M, J, method, banded):
    B = 3
    t, c, a, U, V, alpha, diag, y, _ = dense.kron_synthetic(B, N, M, J)
    env(C2_KRON_BANDED=banded)
    ll, grads, flag = ops.kron_loglik_grad(*dev(t, c, a, U, V, alpha, diag, y), method=method)
    assert int(flag.abs().sum()) == 0
    res = [ex.kron_grad(t[b], c[b], a[b], U[b], V[b], alpha[b], diag[b], y[b]) for b in range(B)]
    gx = [np.stack([r[1][i] for r in res]) for i in range(8)]
    path = "kron_loglik_grad %s" % method
    close(path, [ll], [np.array([r[0] for r in res])], ["ll"])
    tot = lambda g: [g[0], g[1], host(g[3]) + host(g[2])[..., None] * V, host(g[4]) + host(g[2])[..., None] * U, g[5], g[6], g[7]]
    if method == "collapsed":
        close(path, grads, gx, ("bt", "bc", "ba", "bU", "bV", "balpha", "bdiag", "by"))
    else:
        close(path, tot(grads), tot(gx), ("bt", "bc", "bU+baV", "bV+baU", "balpha", "bdiag", "by"))


# ---- per-op reverses -----------------------------------------------------------------------------------------
def _factor_phi(bd, bW):
    def f(t, c, a, U, V):
        d, W = ex.factor_fwd(t, c, a, U, V)
        return np.sum(bd * d, axis=-1) + np.sum(bW * W, axis=(-1, -2))
    return f


@pytest.mark.parametrize("B,N", [(1, 1), (7, 2), (7, 17), (65, 33), (3, 100)])
@pytest.mark.parametrize("J", [1, 2, 3, 5, 8, 12])
def test_factor_rev_vs_complex_step(ops, env, J, B, N):
    arrs, k = batch(B, N, J, seed=5)
    t, c, a, U, V, _ = arrs
    rng = np.random.default_rng(N + J)
    bd0 = rng.standard_normal((k, N)); bW0 = rng.standard_normal((k, N, J))
    pick = np.arange(B) % k
    bd, bW = bd0[pick], bW0[pick]
    env()
    td, cd, ad, Ud, Vd, bdd, bWd = dev(t, c, a, U, V, bd, bW)
    d, W, S, flag = ops.factor(td, cd, ad, Ud, Vd, workspace=True)
    assert int(flag.abs().sum()) == 0
    got = ops.factor_rev(td, cd, ad, Ud, Vd, d, W, S, bdd, bWd)
    want = [ex.cstep_grad(_factor_phi(bd0[i], bW0[i]), [t[i], c[i], a[i], U[i], V[i]]) for i in range(k)]
    close("factor_rev row by row", got, [np.stack([want[b % k][i] for b in range(B)]) for i in range(5)],
          ("bt", "bc", "ba", "bU", "bV"))


def _dirs(rng, shapes, N, chunk=64):
    """Directions for one argument each: random +-1 over everything, and +-1 windows of ~100 rows over the first rows,
    the last rows and two chunk boundaries."""
    out = []
    for i, s in enumerate(shapes):
        full = [rng.choice([-1.0, 1.0], size=s) for _ in range(2)]
        wins = []
        if len(s) and s[0] == N and N > 200:
            for lo in (0, N - 100, chunk * (N // (3 * chunk)) - 50, chunk * (2 * N // (3 * chunk)) - 37):
                v = np.zeros(s)
                v[lo:lo + 100] = rng.choice([-1.0, 1.0], size=(min(100, N - lo),) + s[1:])
                wins.append(v)
        for v in full + wins:
            d = [None] * len(shapes)
            d[i] = v
            out.append(d)
    return out


def _jvp_close(path, grads, f, args, dirs, tol=1e-11):
    want = ex.cstep_jvp(f, args, dirs)
    worst = 0.0
    for k, dvec in enumerate(dirs):
        i = next(j for j, v in enumerate(dvec) if v is not None)
        g = host(grads[i])
        dot, scale = float(np.sum(g * dvec[i])), float(np.sum(np.abs(g * dvec[i])))
        err = abs(dot - float(want[k]))
        worst = max(worst, err / max(scale, 1e-300))
        assert err <= tol * scale, (path, i, k, dot, float(want[k]), scale)
    WORST[path + " (directional, / sum|g v|)"] = max(WORST.get(path + " (directional, / sum|g v|)", 0.0), worst)


@pytest.mark.parametrize("rows", [None, "32", "64"])
@pytest.mark.parametrize("N,J", [(300, 8), (600, 4), (2048, 8)])
def test_factor_rev_time_parallel_vs_complex_step(ops, env, N, J, rows):
    """factor_rev parallel along time (small batches, N >= 512, C2_TIMEPAR_GRAD=1) and row by row: directional
    derivatives of <bd, d> + <bW, W> by complex step of the O(N) factor recursion."""
    arrs, _ = batch(1, N, J, seed=6)
    t, c, a, U, V, _ = (x[0] for x in arrs)
    rng = np.random.default_rng(N)
    bd, bW = rng.standard_normal(N), rng.standard_normal((N, J))
    td, cd, ad, Ud, Vd, bdd, bWd = dev(t[None], c[None], a[None], U[None], V[None], bd[None], bW[None])
    dirs = _dirs(rng, [(N,), (J,), (N,), (N, J), (N, J)], N)
    for grad in ("1", "0"):
        kv = dict(C2_TIMEPAR_GRAD=grad)
        if rows:
            kv["C2_TPG_ROWS"] = rows
        env(**kv)
        d, W, S, flag = ops.factor(td, cd, ad, Ud, Vd, workspace=True)
        assert int(flag.abs().sum()) == 0
        got = [g[0] for g in ops.factor_rev(td, cd, ad, Ud, Vd, d, W, S, bdd, bWd)]
        _jvp_close("factor_rev C2_TIMEPAR_GRAD=%s" % grad, got, _factor_phi(bd, bW), [t, c, a, U, V], dirs)


@pytest.mark.parametrize("nrhs", [1, 2, 5, 8, 9, 16, 17, 25, 32, 33, 70, 128])
@pytest.mark.parametrize("B,N,J", [(3, 9, 8), (7, 65, 4), (2, 300, 8), (2, 300, 3)])
@pytest.mark.parametrize("op", SWEEPS)
def test_sweep_rev_vs_dense_vjp(ops, env, op, B, N, J, nrhs):
    arrs, k = batch(B, N, J, seed=7, distinct=B)
    t, c, a, U, V, _ = arrs
    W = np.stack([ex.factor_fwd(t[b], c[b], a[b], U[b], V[b])[1] for b in range(B)]) if op.startswith("solve") else V
    rng = np.random.default_rng(N + nrhs)
    Y = rng.standard_normal((B, N, nrhs)); bZ = rng.standard_normal((B, N, nrhs))
    env()
    td, cd, Ud, Wd, Yd, bZd = dev(t, c, U, W, Y, bZ)
    fwd = getattr(ops, op)
    Z, F = fwd(td, cd, Ud, Wd, Yd, workspace=True, zero_z=True) if "matmul" in op else fwd(td, cd, Ud, Wd, Yd, workspace=True)
    res = [ex.sweep_vjp(op, t[b], c[b], U[b], W[b], Y[b], bZ[b]) for b in range(B)]
    close("%s forward" % op, [Z], [np.stack([r[0] for r in res])], ["Z"])
    got = getattr(ops, op + "_rev")(td, cd, Ud, Wd, Yd, Z, F, bZd)
    close("%s_rev" % op, got, [np.stack([r[1][i] for r in res]) for i in range(5)], ("bt", "bc", "bU", "bW", "bY"))


@pytest.mark.parametrize("nrhs", [1, 3, 8])
@pytest.mark.parametrize("op", SWEEPS)
def test_sweep_rev_long_form_vs_dense_vjp(ops, env, op, nrhs):
    """The reverse sweeps as opposite sweep + per-row pass (C2_REV_LONG=1) and row by row (=0) on series of 600 rows."""
    B, N, J = 2, 600, 8
    arrs, _ = batch(B, N, J, seed=8, distinct=B)
    t, c, a, U, V, _ = arrs
    W = np.stack([ex.factor_fwd(t[b], c[b], a[b], U[b], V[b])[1] for b in range(B)]) if op.startswith("solve") else V
    rng = np.random.default_rng(nrhs)
    Y = rng.standard_normal((B, N, nrhs)); bZ = rng.standard_normal((B, N, nrhs))
    res = [ex.sweep_vjp(op, t[b], c[b], U[b], W[b], Y[b], bZ[b]) for b in range(B)]
    want = [np.stack([r[1][i] for r in res]) for i in range(5)]
    td, cd, Ud, Wd, Yd, bZd = dev(t, c, U, W, Y, bZ)
    fwd = getattr(ops, op)
    for long_ in ("1", "0"):
        env(C2_REV_LONG=long_)
        Z, F = fwd(td, cd, Ud, Wd, Yd, workspace=True, zero_z=True) if "matmul" in op else fwd(td, cd, Ud, Wd, Yd, workspace=True)
        got = getattr(ops, op + "_rev")(td, cd, Ud, Wd, Yd, Z, F, bZd)
        close("%s_rev C2_REV_LONG=%s" % (op, long_), got, want, ("bt", "bc", "bU", "bW", "bY"))


# ---- long series: directional derivatives ---------------------------------------------------------------------
@pytest.mark.parametrize("N,J", [(16500, 8), (40000, 4), (20001, 3)])
def test_loglik_grad_long_series_directional(ops, env, N, J):
    """The default dispatch of a small batch of long series (the time-parallel gradient): <g, v> against the complex-step
    derivative of the O(N) log-likelihood along v."""
    arrs, _ = batch(2, N, J, seed=9, distinct=2)
    env()
    ll, grads, flag = ops.loglik_grad(*dev(*arrs))
    assert int(flag.abs().sum()) == 0
    for b in range(2):
        args = [x[b] for x in arrs]
        rng = np.random.default_rng(N + b)
        dirs = _dirs(rng, [x.shape for x in args], N)
        llr = float(np.real(ex.recursive_loglik_fwd(*args)))
        assert abs(float(ll[b]) - llr) <= 1e-10 * abs(llr)
        _jvp_close("loglik_grad long series (default)", [g[b] for g in grads], ex.recursive_loglik_fwd, args, dirs)


def test_factor_rev_long_series_directional(ops, env):
    N, J = 16500, 8
    arrs, _ = batch(1, N, J, seed=10)
    t, c, a, U, V, _ = (x[0] for x in arrs)
    rng = np.random.default_rng(1)
    bd, bW = rng.standard_normal(N), rng.standard_normal((N, J))
    env()
    td, cd, ad, Ud, Vd, bdd, bWd = dev(t[None], c[None], a[None], U[None], V[None], bd[None], bW[None])
    d, W, S, flag = ops.factor(td, cd, ad, Ud, Vd, workspace=True)
    assert int(flag.abs().sum()) == 0
    got = [g[0] for g in ops.factor_rev(td, cd, ad, Ud, Vd, d, W, S, bdd, bWd)]
    _jvp_close("factor_rev long series", got, _factor_phi(bd, bW), [t, c, a, U, V],
               _dirs(rng, [(N,), (J,), (N,), (N, J), (N, J)], N))


@pytest.mark.parametrize("op", SWEEPS)
def test_sweep_rev_long_series_directional(ops, env, op):
    N, J, nrhs = 16500, 8, 2
    arrs, _ = batch(1, N, J, seed=11)
    t, c, a, U, V, _ = (x[0] for x in arrs)
    W = ex.factor_fwd(t, c, a, U, V)[1] if op.startswith("solve") else V
    rng = np.random.default_rng(2)
    Y, bZ = rng.standard_normal((N, nrhs)), rng.standard_normal((N, nrhs))
    f = lambda t_, c_, U_, W_, Y_: np.sum(bZ * ex.sweep_fwd(op, t_, c_, U_, W_, Y_), axis=(-1, -2))
    dirs = _dirs(rng, [(N,), (J,), (N, J), (N, J), (N, nrhs)], N)
    td, cd, Ud, Wd, Yd, bZd = dev(t[None], c[None], U[None], W[None], Y[None], bZ[None])
    fwd = getattr(ops, op)
    for long_ in (None, "0"):
        env(**({} if long_ is None else dict(C2_REV_LONG=long_)))
        Z, F = fwd(td, cd, Ud, Wd, Yd, workspace=True, zero_z=True) if "matmul" in op else fwd(td, cd, Ud, Wd, Yd, workspace=True)
        got = [g[0] for g in getattr(ops, op + "_rev")(td, cd, Ud, Wd, Yd, Z, F, bZd)]
        _jvp_close("%s_rev long series" % op, got, f, [t, c, U, W, Y], dirs)


# ---- torch adapters ------------------------------------------------------------------------------------------
def test_autograd_log_likelihood_vs_exact(ops, env):
    import torch
    from celerite2_amd import autograd as ag
    B, N, J = 5, 120, 4
    arrs, k = batch(B, N, J, seed=12, distinct=B)
    w = np.linspace(0.5, 1.5, B)
    _, gx = exact_batch(arrs, k)
    env()
    for shared in (False, True):
        t, c, a, U, V, y = arrs
        if shared:       # one grid and one set of rates: every series is series 0 with its own data
            t, c = t[0].copy(), c[0].copy()
            a, U, V = (np.repeat(x[:1], B, axis=0) for x in (a, U, V))
            one = [ex.loglik_grad(t, c, a[0], U[0], V[0], y[b]) for b in range(B)]
            gx_ = [np.stack([r[1][i] for r in one]) for i in range(6)]
        else:
            gx_ = gx
        xs = [v.requires_grad_() for v in dev(t, c, a, U, V, y)]
        ll = ag.log_likelihood(*xs)
        (ll * torch.from_numpy(w).cuda()).sum().backward()
        want = [g * (w.reshape((B,) + (1,) * (g.ndim - 1))) for g in gx_]
        if shared:
            want[0], want[1] = want[0].sum(0), want[1].sum(0)
        close("autograd.log_likelihood", [x.grad for x in xs], want, MAT)


def test_autograd_log_likelihood_terms_vs_exact(ops, env):
    import torch
    from celerite2_amd import autograd as ag
    B, N, Jr, Jc = 4, 90, 1, 2
    rng = np.random.default_rng(3)
    co = coeffs(Jr, Jc, rng)
    x = np.sort(rng.uniform(0, N / 10.0, N))
    diag = rng.uniform(0.1, 0.3, (B, N)) + 0.5
    y = np.sin(x)[None] + 0.1 * rng.standard_normal((B, N))
    w = np.linspace(0.5, 1.5, B)
    res = [ex.terms_grad(*co, x, diag[b], y[b]) for b in range(B)]
    want = [sum(w[b] * res[b][1][i] for b in range(B)) for i in range(7)] + \
           [np.stack([w[b] * res[b][1][i] for b in range(B)]) for i in (7, 8)]
    env()
    xs = [v.requires_grad_() for v in dev(*co, x, diag, y)]
    ll = ag.log_likelihood_terms(*xs)
    close("autograd.log_likelihood_terms", [ll], [np.array([r[0] for r in res])], ["ll"])
    (ll * torch.from_numpy(w).cuda()).sum().backward()
    close("autograd.log_likelihood_terms", [v.grad for v in xs], want, COEF)


def test_autograd_factor_and_sweeps_vs_exact(ops, env):
    import torch
    from celerite2_amd import autograd as ag
    B, N, J, nrhs = 3, 40, 4, 2
    arrs, k = batch(B, N, J, seed=13, distinct=B)
    t, c, a, U, V, _ = arrs
    rng = np.random.default_rng(4)
    bd, bW = rng.standard_normal((B, N)), rng.standard_normal((B, N, J))
    env()
    xs = [v.requires_grad_() for v in dev(t, c, a, U, V)]
    d, W = ag.factor(*xs)
    ((d * torch.from_numpy(bd).cuda()).sum() + (W * torch.from_numpy(bW).cuda()).sum()).backward()
    want = [ex.cstep_grad(_factor_phi(bd[b], bW[b]), [t[b], c[b], a[b], U[b], V[b]]) for b in range(B)]
    close("autograd.factor", [x.grad for x in xs], [np.stack([r[i] for r in want]) for i in range(5)],
          ("bt", "bc", "ba", "bU", "bV"))
    Y, bZ = rng.standard_normal((B, N, nrhs)), rng.standard_normal((B, N, nrhs))
    for op in SWEEPS:
        Wn = np.stack([ex.factor_fwd(t[b], c[b], a[b], U[b], V[b])[1] for b in range(B)]) if op.startswith("solve") else V
        for shared in (False, True):
            tt, cc = (t[0].copy(), c[0].copy()) if shared else (t, c)
            Us, Ws = (np.repeat(U[:1], B, 0), np.repeat(Wn[:1], B, 0)) if shared else (U, Wn)
            xs = [v.requires_grad_() for v in dev(tt, cc, Us, Ws, Y)]
            Z = getattr(ag, op)(*xs)
            (Z * torch.from_numpy(bZ).cuda()).sum().backward()
            res = [ex.sweep_vjp(op, tt if shared else t[b], cc if shared else c[b], Us[b], Ws[b], Y[b], bZ[b])[1]
                   for b in range(B)]
            want = [np.stack([r[i] for r in res]) for i in range(5)]
            if shared:
                want[0], want[1] = want[0].sum(0), want[1].sum(0)
            close("autograd.%s" % op, [x.grad for x in xs], want, ("bt", "bc", "bU", "bW", "bY"))
