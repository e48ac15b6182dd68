# -*- coding: utf-8 -*-
"""The staging layer of the host drop-in (celerite2_amd/csrc/c2_host.hip) under `celerite2_amd.driver` / `.backprop`:
the per-thread arena, the pinned bounce buffer, address-keyed aliasing, outputs that are never uploaded, the direct path
beyond 64 MiB, the trim beyond 256 MiB and c2h_release_thread_cache.

The kernels underneath are tested through ops.py; what is tested here is that a call on HOST arrays hands them the right
bytes at the right places and brings the right bytes back -- at every shape class, in place, after a larger call, after
a failed one, on views of one array.  One process, no environment switches.  Expected values: the CPU oracle (and the
dense matrix for general_matmul); the two standing criteria of test_fuzz_drop_in_ops_on_small_batches_of_mid_length_series:
    forward results   |got - want| <= 1e-10 |want| + 1e-12 max(1, max|want|)   per element   (fclose)
    reverse results   |got - want| <= 1e-10 max|want|                          per array     (gclose)
and, to tell a staging mistake from rounding, bit identity with ops.<same op> on device copies of the same arrays
(B = 1, t and c one-dimensional: the batch strides c2_host.hip passes)."""
import functools
import threading

import numpy as np
import pytest

import host_layout as H
from oracle import dense
from test_gpu_fuzz import problem        # J <= 32: columns dropped from an SHO sum, diagonal lifted by 1
from test_gpu_ops import wide_batch      # 33 <= J <= 128

pytestmark = pytest.mark.gpu

SWEEPS = ("solve_lower", "solve_upper", "matmul_lower", "matmul_upper")


@pytest.fixture(scope="module")
def mods():
    import torch
    from celerite2_amd import backprop, driver, ops
    assert torch.cuda.is_available()
    return driver, backprop, ops


# ----------------------------------------------------------------------------- criteria
def fclose(g, w):
    g, w = np.asarray(g), np.asarray(w)
    assert g.shape == w.shape and np.isfinite(g).all()
    np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-12 * max(1.0, np.abs(w).max(initial=0.0)))


def gclose(g, w):
    g, w = np.asarray(g), np.asarray(w)
    assert g.shape == w.shape and np.isfinite(g).all()
    np.testing.assert_allclose(g, w, rtol=0.0, atol=1e-10 * max(np.abs(w).max(initial=0.0), 1e-300))


def same_bits(g, w):
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    assert g.shape == w.shape and g.dtype == w.dtype == np.float64
    differ = g.view(np.uint64) != w.view(np.uint64)
    if differ.any():
        raise AssertionError("%d of %d elements differ in bits, largest difference %.3e"
                             % (int(differ.sum()), g.size, float(np.nanmax(np.abs(g - w)))))


class Soft:
    """Collects the failed checks of one case, so that one run shows all of them."""
    def __init__(self):
        self.failed = []

    def __call__(self, label, check, *args):
        try:
            check(*args)
        except AssertionError as e:
            self.failed.append("%s: %s" % (label, " ".join(str(e).split())[:400]))

    def done(self):
        assert not self.failed, "\n".join(["%d checks failed" % len(self.failed)] + self.failed)


# ----------------------------------------------------------------------------- inputs and expected values, computed once
@functools.lru_cache(maxsize=None)
def model(N, J):
    """(t, c, a, U, V) of one positive definite series, read-only."""
    t, c, a, U, V, _ = problem(None, 1, N, J) if J <= 32 else wide_batch(1, N, J)
    out = tuple(np.ascontiguousarray(x[0]) for x in (t, c, a, U, V))
    for x in out:
        x.flags.writeable = False
    return out


def _ro(*xs):
    for x in xs:
        x.flags.writeable = False
    return xs


_ORACLE = []


@functools.lru_cache(maxsize=None)
def expected(N, J, nrhs):
    """Everything the oracle says about one (N, J, nrhs) case, read-only: the factorisation with its workspace, the four
    sweeps with theirs, right-hand sides and adjoints."""
    oracle = _ORACLE[0]
    t, c, a, U, V = model(N, J)
    rng = np.random.default_rng(1000003 * N + 1009 * J + nrhs)
    e = dict(d=np.empty(N), W=np.empty((N, J)), S=np.empty((N, J, J)))
    assert oracle.factor_flag(t, c, a, U, V, e["d"], e["W"], e["S"]) == 0
    e["Y"], e["bZ"], e["Z0"] = (rng.standard_normal((N, nrhs)) for _ in range(3))
    e["bd"], e["bW"] = rng.standard_normal(N), rng.standard_normal((N, J))
    for op in SWEEPS:
        A = e["W"] if op.startswith("solve") else V
        Z, F = np.empty((N, nrhs)), np.empty((N, J, nrhs))
        getattr(oracle, op + "_fwd")(t, c, U, A, e["Y"], Z, F)
        e[op] = _ro(Z, F)
    _ro(*[v for v in e.values() if isinstance(v, np.ndarray)])
    return e


@pytest.fixture(scope="module", autouse=True)
def _oracle_for_expected(oracle):
    _ORACLE[:] = [oracle]


def grads(N, J, nrhs=None):
    """Empty gradient arrays of factor_rev (nrhs None) or of a sweep's reverse."""
    if nrhs is None:
        return [np.empty(N), np.empty(J), np.empty(N), np.empty((N, J)), np.empty((N, J))]
    return [np.empty(N), np.empty(J), np.empty((N, J)), np.empty((N, J)), np.empty((N, nrhs))]


def general_dense(lower, t1, t2, c, U, V, Y, rows):
    """Rows `rows` of the matrix general_matmul_lower / _upper applies (general.hpp: row n of the lower form takes the
    columns m with t2[m] <= t1[n], the upper form the others), times Y: sum_j U[n,j] V[m,j] exp(-c_j |t1[n] - t2[m]|)."""
    dt = t1[rows, None] - t2[None, :]
    mask = dt >= 0 if lower else dt < 0
    K = np.zeros(dt.shape)
    for j in range(len(c)):
        K += np.outer(U[rows, j], V[:, j]) * np.exp(-c[j] * np.abs(dt))
    return (K * mask) @ Y


# ----------------------------------------------------------------------------- one call through the drop-in
def bits(x):
    return np.ascontiguousarray(x).view(np.uint64).copy()


def call(soft, label, fn, args, n_out):
    """fn(*args), whose last n_out arguments are its outputs: (b) every returned object is the array passed, (c) every
    argument that is not an output has the bits it had.  Returns the outputs."""
    outs = args[len(args) - n_out:]
    pure = [x for x in args[:len(args) - n_out] if not any(x is o for o in outs)]
    before = [bits(x) for x in pure]
    res = fn(*args)
    res = res if isinstance(res, tuple) else (res,)
    soft(label + " returns its arguments", lambda: _same_objects(res, outs))
    soft(label + " leaves its inputs alone", lambda: _unchanged(pure, before))
    return outs


def _same_objects(res, outs):
    assert len(res) == len(outs) and all(r is o for r, o in zip(res, outs))


def _unchanged(pure, before):
    for i, (x, b) in enumerate(zip(pure, before)):
        assert np.array_equal(bits(x), b), "input %d changed" % i


def dev(*xs):
    import torch
    return [torch.from_numpy(np.array(x, dtype=np.float64, order="C")).cuda() for x in xs]   # (a copy: the cached inputs are read-only)


def host(x):
    return x.cpu().numpy()


# ----------------------------------------------------------------------------- D1: the shape sweep
CORNERS = [(1, 1, 1), (1, 128, 1), (2, 33, 3), (3, 5, 2), (31, 7, 9), (32, 8, 1), (33, 32, 33), (100, 128, 3), (511, 8, 1),
           (512, 8, 1), (513, 8, 9), (600, 40, 2), (1300, 3, 2), (2049, 4, 2), (2049, 16, 1)]


def _shapes():
    """The corners, then 25 draws of one seeded generator over the boundary values: 512 rows is where a single series moves
    to the time-parallel forms, width 33 where the workgroup-per-series kernels start, the rest are lane-group and block
    boundaries.  A draw whose workspaces would make the case slow (S beyond 32 MiB, F beyond 16 MiB) is drawn again."""
    rng = np.random.default_rng(20240607)
    Ns, Js, Ks = [1, 2, 3, 31, 32, 33, 100, 511, 512, 513, 1300, 2049], [1, 2, 3, 4, 5, 7, 8, 16, 31, 32, 33, 64, 128], [1, 2, 3, 8, 9, 33]
    out = list(CORNERS)
    while len(out) < 40:
        s = (int(rng.choice(Ns)), int(rng.choice(Js)), int(rng.choice(Ks)))
        if s not in out and 8 * s[0] * s[1] * s[1] <= 32 << 20 and 8 * s[0] * s[1] * s[2] <= 16 << 20:
            out.append(s)
    return out


SHAPES = _shapes()
# (the (N, J, nrhs) of a case and the M of its general_matmul_*: the N of the next case)
CASES = [(N, J, nrhs, SHAPES[(i + 1) % len(SHAPES)][0]) for i, (N, J, nrhs) in enumerate(SHAPES)]
# cases whose bits legitimately differ from ops.<same op> (D1 e): none known; a case listed here keeps every other check
BITS_DIFFER = {}
# (d) for factor: out of place, a single series of width 2, 4 or 8 and some hundred rows is factorised parallel along time;
# in place (d is a or W is V) it stays on the row-by-row kernel, because the fallback of the time-parallel form would read
# what that form overwrote (c2_loglik.hip: c2_internal_factor_fused).  Two kernels, two roundings: at these shapes the
# in-place result is held to the oracle and to the bits of ops.factor IN PLACE, not to the bits of the out-of-place call.
FACTOR_IN_PLACE_IS_ANOTHER_KERNEL = {s for s in SHAPES if s[1] in (2, 4, 8) and s[0] >= 511}


def check_factor(soft, mods, oracle, N, J, nrhs, tag=""):
    driver, backprop, ops = mods
    t, c, a, U, V = model(N, J)
    e = expected(N, J, nrhs)
    td, cd, ad, Ud, Vd = dev(t, c, a[None], U[None], V[None])
    # driver.factor, out of place
    d, W = call(soft, tag + "factor", driver.factor, [t, c, a, U, V, np.full(N, 7.0), np.full((N, J), 7.0)], 2)
    soft(tag + "factor d", fclose, d, e["d"]); soft(tag + "factor W", fclose, W, e["W"])
    gd, gW, flag = ops.factor(td, cd, ad, Ud, Vd)
    assert int(flag[0]) == 0
    soft(tag + "factor d bits", same_bits, d, host(gd)[0]); soft(tag + "factor W bits", same_bits, W, host(gW)[0])
    # (d) in place: d is a alone, W is V alone, both
    for da, wv in ((True, False), (False, True), (True, True)):
        lab = tag + "factor in place %d%d" % (da, wv)
        a2, V2 = a.copy(), V.copy()
        d2, W2 = call(soft, lab, driver.factor, [t, c, a2, U, V2, a2 if da else np.empty(N), V2 if wv else np.empty((N, J))], 2)
        soft(lab + " d", fclose, d2, e["d"]); soft(lab + " W", fclose, W2, e["W"])
        if (N, J, nrhs) not in FACTOR_IN_PLACE_IS_ANOTHER_KERNEL:
            soft(lab + " d as out of place", same_bits, d2, d); soft(lab + " W as out of place", same_bits, W2, W)
        a2d, V2d = dev(a[None], V[None])
        gd, gW, flag = ops.factor(td, cd, a2d, Ud, V2d, d=a2d if da else None, W=V2d if wv else None)
        soft(lab + " d bits", same_bits, d2, host(gd)[0]); soft(lab + " W bits", same_bits, W2, host(gW)[0])
        if not da:
            soft(lab + ": a kept", same_bits, a2, a)
        if not wv:
            soft(lab + ": V kept", same_bits, V2, V)
    # backprop.factor_fwd
    d, W, S = call(soft, tag + "factor_fwd", backprop.factor_fwd, [t, c, a, U, V, np.empty(N), np.empty((N, J)), np.empty((N, J, J))], 3)
    for nm, g in (("d", d), ("W", W), ("S", S)):
        soft(tag + "factor_fwd " + nm, fclose, g, e[nm])
    gd, gW, gS, flag = ops.factor(td, cd, ad, Ud, Vd, workspace=True)
    for nm, g, w in (("d", d, gd), ("W", W, gW), ("S", S, gS)):
        soft(tag + "factor_fwd %s bits" % nm, same_bits, g, host(w)[0])
    # backprop.factor_rev on what factor_fwd returned; the oracle gets the same d, W, S
    got = call(soft, tag + "factor_rev", backprop.factor_rev, [t, c, a, U, V, d, W, S, e["bd"], e["bW"]] + grads(N, J), 5)
    want = oracle.factor_rev(t, c, a, U, V, d, W, S, e["bd"], e["bW"], *[np.zeros_like(g) for g in got])
    on_dev = ops.factor_rev(td, cd, ad, Ud, Vd, *dev(d[None], W[None], S[None], e["bd"][None], e["bW"][None]))
    for nm, g, w, o in zip(("bt", "bc", "ba", "bU", "bV"), got, want, on_dev):
        soft(tag + "factor_rev " + nm, gclose, g, w)
        soft(tag + "factor_rev %s bits" % nm, same_bits, g, host(o)[0])


def check_sweeps(soft, mods, oracle, N, J, nrhs, tag=""):
    driver, backprop, ops = mods
    t, c, a, U, V = model(N, J)
    e = expected(N, J, nrhs)
    Y, bZ = e["Y"], e["bZ"]
    td, cd, Ud, Yd = dev(t, c, U[None], Y[None])
    for op in SWEEPS:
        solve = op.startswith("solve")
        A = e["W"] if solve else V       # (the oracle's W: the same inputs on both sides)
        Ad, = dev(A[None])
        Zf, Ff = e[op]
        lab = tag + op
        # driver form: a solve overwrites Z, a product adds to it
        Z0 = np.full((N, nrhs), 7.0) if solve else e["Z0"].copy()
        want = Zf if solve else oracle_accumulate(oracle, op, t, c, U, A, Y, e["Z0"])
        Z, = call(soft, lab, getattr(driver, op), [t, c, U, A, Y, Z0.copy()], 1)
        soft(lab + " Z", fclose, Z, want)
        Zd, = dev(Z0[None])
        soft(lab + " Z bits", same_bits, Z, host(getattr(ops, op)(td, cd, Ud, Ad, Yd, Z=Zd))[0])
        if solve:   # (d) Z is Y
            Y2 = Y.copy()
            Z2, = call(soft, lab + " in place", getattr(driver, op), [t, c, U, A, Y2, Y2], 1)
            soft(lab + " in place Z", same_bits, Z2, Z)
        # backprop *_fwd: Z is zeroed first, F is the workspace
        Z, F = call(soft, lab + "_fwd", getattr(backprop, op + "_fwd"), [t, c, U, A, Y, np.full((N, nrhs), 7.0), np.empty((N, J, nrhs))], 2)
        soft(lab + "_fwd Z", fclose, Z, Zf); soft(lab + "_fwd F", fclose, F, Ff)
        gZ, gF = getattr(ops, op)(td, cd, Ud, Ad, Yd, workspace=True, **({} if solve else dict(zero_z=True)))
        soft(lab + "_fwd Z bits", same_bits, Z, host(gZ)[0]); soft(lab + "_fwd F bits", same_bits, F, host(gF)[0])
        # backprop *_rev on what *_fwd returned; the oracle gets the same Z, F
        got = call(soft, lab + "_rev", getattr(backprop, op + "_rev"), [t, c, U, A, Y, Z, F, bZ] + grads(N, J, nrhs), 5)
        want = getattr(oracle, op + "_rev")(t, c, U, A, Y, Z, F, bZ, *[np.zeros_like(g) for g in got])
        on_dev = getattr(ops, op + "_rev")(td, cd, Ud, Ad, Yd, *dev(Z[None], F[None], bZ[None]))
        for nm, g, w, o in zip(("bt", "bc", "bU", "bW", "bY"), got, want, on_dev):
            soft("%s_rev %s" % (lab, nm), gclose, g, w)
            soft("%s_rev %s bits" % (lab, nm), same_bits, g, host(o)[0])


def oracle_accumulate(oracle, op, t, c, U, A, Y, Z0):
    Z = Z0.copy()
    getattr(oracle, op)(t, c, U, A, Y, Z)
    return Z


def check_general(soft, mods, oracle, N, J, nrhs, M, tag=""):
    """general_matmul_lower / _upper and their *_fwd forms: N rows at times t1 drawn over the span of t2 extended by half a
    unit on each side (as test_fuzz_general_matmul draws them), the M-row model on the t2 side."""
    driver, backprop, ops = mods
    t2, c, _, _, V = model(M, J)
    rng = np.random.default_rng(77 + 1000003 * N + 1009 * J + 7 * nrhs + 13 * M)
    t1 = np.sort(t2[0] - 0.5 + (t2[-1] - t2[0] + 1.0) * rng.random(N))
    U = rng.standard_normal((N, J)); Y = rng.standard_normal((M, nrhs)); Z0 = rng.standard_normal((N, nrhs))
    # the dense product on every row while that stays cheap, otherwise on a stride of rows with both ends
    step = max(1, -(-N * M * J // 30000000))
    rows = np.unique(np.concatenate([np.arange(0, N, step), [N - 1]]))
    t1d, t2d, cd, Ud, Vd, Yd = dev(t1, t2, c, U[None], V[None], Y[None])
    for name in ("general_matmul_lower", "general_matmul_upper"):
        lab = tag + name
        KY = general_dense(name.endswith("lower"), t1, t2, c, U, V, Y, rows)
        Z, = call(soft, lab, getattr(driver, name), [t1, t2, c, U, V, Y, Z0.copy()], 1)
        soft(lab + " Z", fclose, Z, getattr(oracle, name)(t1, t2, c, U, V, Y, Z0.copy()))
        soft(lab + " Z dense", fclose, Z[rows], Z0[rows] + KY)
        Zd, = dev(Z0[None])
        soft(lab + " Z bits", same_bits, Z, host(getattr(ops, name)(t1d, t2d, cd, Ud, Vd, Yd, Z=Zd))[0])
        # *_fwd: Z zeroed first; F keeps the caller's contents on the rows the sweep never absorbs
        Z, F = call(soft, lab + "_fwd", getattr(backprop, name + "_fwd"),
                    [t1, t2, c, U, V, Y, np.full((N, nrhs), 3.0), np.full((M, J, nrhs), -1.0)], 2)
        Zo, Fo = getattr(oracle, name + "_fwd")(t1, t2, c, U, V, Y, np.full((N, nrhs), 3.0), np.full((M, J, nrhs), -1.0))
        soft(lab + "_fwd Z", fclose, Z, Zo); soft(lab + "_fwd F", fclose, F, Fo)
        soft(lab + "_fwd Z dense", fclose, Z[rows], KY)
        Zd, Fd = dev(np.full((1, N, nrhs), 3.0), np.full((1, M, J, nrhs), -1.0))
        gZ, gF = getattr(ops, name)(t1d, t2d, cd, Ud, Vd, Yd, Z=Zd, F=Fd, zero_z=True)
        soft(lab + "_fwd Z bits", same_bits, Z, host(gZ)[0]); soft(lab + "_fwd F bits", same_bits, F, host(gF)[0])


@pytest.mark.parametrize("N,J,nrhs,M", CASES, ids=["%d-%d-%d" % s[:3] for s in CASES])
def test_every_drop_in_function_at_every_shape_class(mods, oracle, N, J, nrhs, M):
    """D1.  The 8 functions of `driver` and the 12 of `backprop` (each *_rev on what its *_fwd returned) at 40 shapes, run in
    list order on one thread, so the arena grows and then serves smaller calls after larger ones."""
    soft = Soft()
    check_factor(soft, mods, oracle, N, J, nrhs)
    check_sweeps(soft, mods, oracle, N, J, nrhs)
    check_general(soft, mods, oracle, N, J, nrhs, M)
    if (N, J, nrhs) in BITS_DIFFER:
        soft.failed = [f for f in soft.failed if " bits:" not in f]
    soft.done()


def term_mix(Jr, Jc, seed):
    rng = np.random.default_rng(seed)
    return dense.Coeffs(ar=rng.uniform(0.1, 2.0, Jr), cr=rng.uniform(0.1, 2.0, Jr), ac=rng.uniform(0.1, 2.0, Jc),
                        bc=rng.uniform(-1.0, 1.0, Jc), cc=rng.uniform(0.1, 2.0, Jc), dc=rng.uniform(0.1, 2.0, Jc))


def matrices_case(N, Jr, Jc, seed=5):
    co = term_mix(Jr, Jc, seed + 100 * Jr + Jc)
    rng = np.random.default_rng(seed + N)
    x = np.sort(rng.uniform(0, 10, N)); diag = rng.uniform(0.1, 0.3, N)
    ins = [np.ascontiguousarray(v, dtype=np.float64) for v in (co.ar, co.ac, co.bc, co.dc, x, diag)]
    return co, ins, dense.celerite_matrices(co, x, diag)[1:]


def matrices_close(got, want):
    """The tolerances of test_gpu_driver.py::test_get_celerite_matrices."""
    assert all(np.isfinite(g).all() for g in got)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-14)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (0, 1), (3, 0), (0, 3), (2, 2), (5, 7), (1, 16), (32, 0), (0, 16), (4, 18), (0, 64), (128, 0)])
def test_get_celerite_matrices_on_term_mixes(mods, Jr, Jc):
    """D1, driver.get_celerite_matrices: random mixes of real and complex terms -- Jr = 0 and Jc = 0 (empty coefficient
    arrays) among them -- against dense.celerite_matrices, and bit for bit against ops.get_celerite_matrices."""
    driver, _, ops = mods
    soft = Soft()
    for N in (1, 5, 100, 513):
        co, ins, want = matrices_case(N, Jr, Jc)
        J = Jr + 2 * Jc
        got = call(soft, "N = %d" % N, driver.get_celerite_matrices, ins + [np.empty(N), np.empty((N, J)), np.empty((N, J))], 3)
        soft("N = %d" % N, matrices_close, got, want)
        ar, ac, bc, dc, x, diag = dev(*ins)
        for nm, g, o in zip("aUV", got, ops.get_celerite_matrices(ar, ac, bc, dc, x, diag[None])):
            soft("N = %d %s bits" % (N, nm), same_bits, g, host(o)[0])
    soft.done()


# ----------------------------------------------------------------------------- D2: outputs that are never uploaded
POISON_SHAPES = [(1, 1, 1), (2, 33, 3), (33, 8, 3), (513, 8, 2), (600, 40, 2), (2049, 4, 1)]
TARGETS = ["factor_fwd", "factor_rev", "get_celerite_matrices"] + [op + sfx for op in SWEEPS for sfx in ("_fwd", "_rev")]


def poisoned(fn, op, args):
    """fn(*args) right behind a call that left NaN on every byte its never-uploaded outputs will occupy."""
    lay = H.layout(H.entries(op, *args))
    assert lay["fresh"] > 0
    H.poison(lay["upload"], lay["total"])
    return fn(*args)


@pytest.mark.parametrize("N,J,nrhs", POISON_SHAPES, ids=["%d-%d-%d" % s for s in POISON_SHAPES])
@pytest.mark.parametrize("target", TARGETS)
def test_fresh_outputs_are_written_completely(mods, oracle, target, N, J, nrhs):
    """D2.  S, F, the gradients of the *_rev ops and a, U, V of get_celerite_matrices are never uploaded: what an element the
    kernels do not write returns is what the arena held.  With NaN there (host_layout.poison) every element must come
    back finite and right -- at a single row, two rows of a wide model, a ragged block, either side of a chunk boundary."""
    driver, backprop, _ = mods
    t, c, a, U, V = model(N, J)
    e = expected(N, J, nrhs)
    if target == "factor_fwd":
        d, W, S = poisoned(backprop.factor_fwd, "factor", [t, c, a, U, V, np.empty(N), np.empty((N, J)), np.empty((N, J, J))])
        fclose(d, e["d"]); fclose(W, e["W"]); fclose(S, e["S"])
    elif target == "factor_rev":
        ins = [t, c, a, U, V, e["d"], e["W"], e["S"], e["bd"], e["bW"]]
        got = poisoned(backprop.factor_rev, "factor_rev", ins + grads(N, J))
        for g, w in zip(got, oracle.factor_rev(*ins, *[np.zeros_like(g) for g in got])):
            gclose(g, w)
    elif target == "get_celerite_matrices":
        Jc = J // 2
        co, ins, want = matrices_case(N, J - 2 * Jc, Jc)
        got = poisoned(driver.get_celerite_matrices, "get_celerite_matrices", ins + [np.empty(N), np.empty((N, J)), np.empty((N, J))])
        matrices_close(got, want)
    else:
        op = target[:-4]
        A = e["W"] if op.startswith("solve") else V
        Zf, Ff = e[op]
        if target.endswith("_fwd"):
            Z, F = poisoned(getattr(backprop, target), "sweep", [t, c, U, A, e["Y"], np.full((N, nrhs), 7.0), np.empty((N, J, nrhs))])
            fclose(Z, Zf); fclose(F, Ff)
        else:
            ins = [t, c, U, A, e["Y"], Zf, Ff, e["bZ"]]
            got = poisoned(getattr(backprop, target), "sweep_rev", ins + grads(N, J, nrhs))
            for g, w in zip(got, getattr(oracle, target)(*ins, *[np.zeros_like(g) for g in got])):
                gclose(g, w)


# ----------------------------------------------------------------------------- D3: the life of the arena
def factor_total(N, J):
    """The staging total of backprop.factor_fwd at (N, J), from the layout rule."""
    sizes = dict(t=N, c=J, a=N, U=N * J, V=N * J, d=N, W=N * J, S=N * J * J, flag=1)
    return H.layout([(name, 8 * sizes[name], kind) for name, kind in H.ORDER["factor"]])["total"]


def rows_below(limit, J):
    """The largest N whose factor_fwd stages no more than `limit` bytes."""
    lo, hi = 1, 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if factor_total(mid, J) <= limit else (lo, mid)
    return lo


def factor_fwd_checked(mods, oracle, N, J):
    _, backprop, _ = mods
    t, c, a, U, V = model(N, J)
    d, W, S = backprop.factor_fwd(t, c, a, U, V, np.empty(N), np.empty((N, J)), np.empty((N, J, J)))
    do, Wo, So = np.empty(N), np.empty((N, J)), np.empty((N, J, J))
    assert oracle.factor_flag(t, c, a, U, V, do, Wo, So) == 0
    fclose(d, do); fclose(W, Wo); fclose(S, So)


def small_call(mods, oracle):
    _, backprop, _ = mods
    t, c, a, U, V = model(33, 8)
    e = expected(33, 8, 3)
    d, W, S = backprop.factor_fwd(t, c, a, U, V, np.empty(33), np.empty((33, 8)), np.empty((33, 8, 8)))
    fclose(d, e["d"]); fclose(W, e["W"]); fclose(S, e["S"])


@pytest.mark.parametrize("J", [8, 32])
def test_either_side_of_the_bounce_limit(mods, oracle, J):
    """D3.  backprop.factor_fwd at the last length that goes through the pinned bounce buffer and at the first that goes up
    argument by argument, each followed by a small call on the arena the large one left."""
    N = rows_below(H.BOUNCE_MAX, J)
    assert factor_total(N, J) <= H.BOUNCE_MAX < factor_total(N + 1, J)
    for n in (N, N + 1):
        factor_fwd_checked(mods, oracle, n, J)
        small_call(mods, oracle)


def test_beyond_the_kept_size(mods, oracle):
    """D3.  A call that stages more than 256 MiB (the arena is given back behind it), then a small one."""
    N = rows_below(H.KEEP_MAX, 32) + 1
    assert factor_total(N, 32) > H.KEEP_MAX
    factor_fwd_checked(mods, oracle, N, 32)
    small_call(mods, oracle)


def test_release_and_short_lived_threads(mods, oracle):
    """D3.  c2h_release_thread_cache in front of and behind a call; eight threads one after another, each making one call
    and exiting (its arena goes with it); then the main thread again."""
    from celerite2_amd import _lib
    lib = _lib.load()
    small_call(mods, oracle)
    lib.c2h_release_thread_cache()
    small_call(mods, oracle)
    lib.c2h_release_thread_cache()
    lib.c2h_release_thread_cache()   # (nothing held: a no-op)
    errors = []

    def work():
        try:
            small_call(mods, oracle)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    expected(33, 8, 3)   # (computed here, not in a thread)
    for _ in range(8):
        th = threading.Thread(target=work)
        th.start()
        th.join()
    assert not errors, errors[:3]
    small_call(mods, oracle)


# ----------------------------------------------------------------------------- D4: failure, then recovery
@pytest.mark.parametrize("N,J", [(3, 2), (100, 8), (513, 8), (600, 40)])
def test_failed_factorisation_then_a_good_call(mods, oracle, N, J):
    """D4.  LinAlgError exactly where oracle.factor_flag is non-zero -- a bad pivot at row 1, at a middle row, at the last
    row, and none -- from driver.factor and backprop.factor_fwd; behind every failure a good call on the same arena."""
    driver, backprop, _ = mods
    t, c, a, U, V = model(N, J)
    e = expected(N, J, 1)
    soft = Soft()
    for row in (1, N // 2, N - 1, None):
        bad = a.copy()
        if row is not None:
            bad[row] = -1.0
        flag = oracle.factor_flag(t, c, bad, U, V, np.empty(N), np.empty((N, J)), np.empty((N, J, J)))
        assert (flag != 0) == (row is not None), (row, flag)
        for name, mod, extra in (("factor", driver, []), ("factor_fwd", backprop, [np.empty((N, J, J))])):
            raised = False
            try:
                getattr(mod, name)(t, c, bad, U, V, np.empty(N), np.empty((N, J)), *extra)
            except mod.LinAlgError:
                raised = True
            soft("%s, bad row %s: raised %s, oracle flag %d" % (name, row, raised, flag), lambda: _is(raised == (flag != 0)))
            # the good call behind it
            out = getattr(mod, name)(t, c, a, U, V, np.empty(N), np.empty((N, J)), *[np.empty_like(x) for x in extra])
            for nm, g in zip(("d", "W", "S"), out):
                soft("%s after bad row %s: %s" % (name, row, nm), fclose, g, e[nm])
    soft.done()


def _is(x):
    assert x


def test_converted_arguments_land_in_the_returned_copy(mods):
    """D4.  An int64 Y and a float32 Z are converted on the way in (pybind11 forcecast, as in the reference): the result is
    in the float64 array the call returns, the caller's Z keeps its bits, the numbers are those of the float64 call."""
    driver, _, _ = mods
    N, J, nrhs = 100, 8, 3
    t, c, a, U, V = model(N, J)
    W = expected(N, J, nrhs)["W"]
    rng = np.random.default_rng(3)
    Yi = rng.integers(-5, 6, (N, nrhs)).astype(np.int64)
    Zs = rng.standard_normal((N, nrhs)).astype(np.float32)
    for op, A in (("solve_lower", W), ("matmul_lower", V)):
        kept = Zs.copy()
        got = getattr(driver, op)(t, c, U, A, Yi, Zs)
        assert got is not Zs and got.dtype == np.float64 and np.array_equal(Zs.view(np.uint32), kept.view(np.uint32))
        want = getattr(driver, op)(t, c, U, A, Yi.astype(np.float64), Zs.astype(np.float64))
        same_bits(got, want)


# ----------------------------------------------------------------------------- D5: views of one array
@pytest.mark.parametrize("n,J,k", [(100, 2, 37), (600, 8, 300)])
def test_views_of_one_array(mods, oracle, n, J, k):
    """D5.  Conditioning on x and predicting at a view of x (and the reverse): t1 = x[:k] shares its address with t2 = x and
    is shorter, x[k:] overlaps it from another address, x[::1] is x; t2 = x[:k] under t1 = x puts the longer one first.
    lower + upper is K_star Y, each is what the oracle gives, and each has the bits of the same call on copies."""
    driver, backprop, _ = mods
    co = dense.sho_sum_coeffs(J)
    rng = np.random.default_rng(8 + n)
    x = np.sort(rng.uniform(0, n / 10.0, n))
    c, _, U, V = dense.celerite_matrices(co, x, np.zeros(n))
    nrhs = 3
    soft = Soft()
    for lab, s1, s2 in (("x[:k] over x", slice(0, k), slice(None)), ("x[k:] over x", slice(k, None), slice(None)),
                        ("x[::1] over x", slice(None, None, 1), slice(None)), ("x over x[:k]", slice(None), slice(0, k))):
        t1, t2 = x[s1], x[s2]
        assert t1.flags.c_contiguous and t2.flags.c_contiguous
        N, M = len(t1), len(t2)
        Y = rng.standard_normal((M, nrhs))
        KY = dense.kernel_value(co, t1[:, None] - t2[None, :]) @ Y
        total = np.zeros((N, nrhs))
        for name, Ua, Va in (("general_matmul_lower", U[s1], V[s2]), ("general_matmul_upper", V[s1], U[s2])):
            assert Ua.flags.c_contiguous and Va.flags.c_contiguous
            Z, = call(soft, "%s %s" % (name, lab), getattr(driver, name), [t1, t2, c, Ua, Va, Y, np.zeros((N, nrhs))], 1)
            soft("%s %s oracle" % (name, lab), fclose, Z, getattr(oracle, name)(t1.copy(), t2.copy(), c, Ua.copy(), Va.copy(), Y, np.zeros((N, nrhs))))
            soft("%s %s copies" % (name, lab), same_bits, Z,
                 getattr(driver, name)(t1.copy(), t2.copy(), c, Ua.copy(), Va.copy(), Y, np.zeros((N, nrhs))))
            total += Z
            Zf, Ff = call(soft, "%s_fwd %s" % (name, lab), getattr(backprop, name + "_fwd"),
                          [t1, t2, c, Ua, Va, Y, np.full((N, nrhs), 3.0), np.full((M, J, nrhs), -1.0)], 2)
            Zo, Fo = getattr(oracle, name + "_fwd")(t1.copy(), t2.copy(), c, Ua.copy(), Va.copy(), Y, np.full((N, nrhs), 3.0),
                                                    np.full((M, J, nrhs), -1.0))
            soft("%s_fwd %s oracle Z" % (name, lab), fclose, Zf, Zo); soft("%s_fwd %s oracle F" % (name, lab), fclose, Ff, Fo)
            Zc, Fc = getattr(backprop, name + "_fwd")(t1.copy(), t2.copy(), c, Ua.copy(), Va.copy(), Y, np.full((N, nrhs), 3.0),
                                                      np.full((M, J, nrhs), -1.0))
            soft("%s_fwd %s copies Z" % (name, lab), same_bits, Zf, Zc); soft("%s_fwd %s copies F" % (name, lab), same_bits, Ff, Fc)
        soft("lower + upper = K_star Y, %s" % lab, fclose, total, KY)
    soft.done()
