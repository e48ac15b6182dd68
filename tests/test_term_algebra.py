# -*- coding: utf-8 -*-
"""Term algebra (TermProduct, TermDiff, TermConvolution), pinned on the CPU: the host classes of celerite2_amd/terms.py and
the numpy restatement of the device expression program (tests/term_algebra_ref.py) against what the REFERENCE's term
classes produced (tests/golden/algebra_golden.npz, written by tests/golden/make_golden_algebra.py); the hand-written
reverse against the exact complex-step Jacobian of the restatement; the expression builder; and the C entry points'
validation, which runs before any launch and therefore without a GPU.

Bands.  1e-14 of the largest expected entry, the figure tests/test_term_params.py uses -- except under a convolution: the
reference's cosh(z) - 1, z - sinh z and cosh(cd) cos(dd) - 1 lose kappa = 2 / |z|^2 in relative accuracy at small
z = (c + i d) delta (a perturbation eps of cosh z is eps cosh z / (cosh z - 1) ~ 2 eps / |z|^2 of the result), so there the
band is 1e-14 max(1, kappa) with kappa computed from the case's own rates.  This implementation sums power series at small
z; it sits closer to the truth and inside that band of the reference."""
import os

import numpy as np
import pytest

import term_algebra_ref as A
import term_params_ref as R
from oracle import exact

NAMES = ("ar", "cr", "ac", "bc", "cc", "dc")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixtures():
    with np.load(os.path.join(HERE, "golden", "algebra_golden.npz")) as z:
        return {k: z[k] for k in z.files}


def host_kernel(name):
    from celerite2_amd import terms as T

    return A.build_cases(T, float)[name]()


def tensor_kernel(name, device="cpu"):
    import torch
    from celerite2_amd import terms as T

    return A.build_cases(T, lambda x: torch.tensor(x, dtype=torch.float64, device=device))[name]()


def kappa_host(kernel):
    """max(1, 2 / |z|^2) over the terms a TermConvolution convolves (its inner term's rates), 1 for any other kernel."""
    from celerite2_amd import terms as T

    if not isinstance(kernel, T.TermConvolution):
        return 1.0
    _, cr, _, _, cc, dc = kernel.term.get_coefficients()
    z2 = np.concatenate([cr**2, cc**2 + dc**2]) * kernel.delta**2
    return max(1.0, float(np.max(2.0 / z2)))


def close(got, want, band, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size:
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print("%s: err %.2e  band %.2e" % (what, err, band))
        assert err <= band, (what, err, band)


# ---- 1. the host classes against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.CASES)
def test_host_classes_reproduce_the_reference(fixtures, name):
    k = host_kernel(name)
    band = 1e-14 * kappa_host(k)
    co = k.get_coefficients()
    for cn, g in zip(NAMES, co):
        close(g, fixtures["%s_%s" % (name, cn)], band, name + " " + cn)     # array by array: this pins the ORDER
    assert k.width == fixtures[name + "_c"].size
    shift = k.get_delta_diag() if hasattr(k, "get_delta_diag") else 0.0
    assert (shift != 0.0) == name.startswith("conv")
    close(fixtures["diag"] + np.sum(co[0]) + np.sum(co[2]) + shift, fixtures[name + "_a"], band, name + " a")
    lags = fixtures[name + "_lags"]
    close(k.get_value(lags), fixtures[name + "_value"], band, name + " value")   # lags 0, delta / 3: the piecewise branch
    x = fixtures["x"]
    K = k.get_value(x[:, None] - x[None, :]) + np.diag(fixtures["diag"])
    close(K, fixtures[name + "_K"], band, name + " K")
    close(k.get_psd(fixtures["omega"]), fixtures[name + "_psd"], band, name + " psd")


def test_host_classes_batch_like_the_existing_ones():
    """(J,) shared or (B, J) per series: a per-series parameter anywhere makes every array of the result (B, J)."""
    from celerite2_amd import terms as T

    a = np.array([1.3, 0.7, 2.0])
    k = T.TermConvolution(T.SHOTerm(S0=np.array([5.0, 4.0, 3.0]), w0=0.8, Q=3.45) * T.RealTerm(a=a, c=0.4)
                          + T.TermDiff(T.Matern32Term(sigma=0.5, rho=2.0)), np.array([0.05, 0.02, 0.08]))
    co = k.get_coefficients()
    assert [v.shape for v in co] == [(3, 0)] * 2 + [(3, 2)] * 4 and k.get_delta_diag().shape == (3, 1)
    for b in range(3):
        kb = T.TermConvolution(T.SHOTerm(S0=[5.0, 4.0, 3.0][b], w0=0.8, Q=3.45) * T.RealTerm(a=a[b], c=0.4)
                               + T.TermDiff(T.Matern32Term(sigma=0.5, rho=2.0)), [0.05, 0.02, 0.08][b])
        for v, w in zip(co, kb.get_coefficients()):
            assert np.array_equal(v[b], w)
        assert k.get_delta_diag()[b, 0] == kb.get_delta_diag()
    assert k.get_psd([0.1, 1.0]).shape == (3, 2)


# ---- 2. the restatement against the reference, and the hand-written reverse against the exact Jacobian --------------------
@pytest.mark.parametrize("name", A.CASES)
def test_restatement_reproduces_the_reference(fixtures, name):
    k = tensor_kernel(name)
    prog = k.program
    expr = (prog.records, prog.operations)
    P = k.parameter_matrix().numpy()
    band = 1e-14 * float(A.kappa(expr, P))
    assert float(A.kappa(expr, P)) == pytest.approx(kappa_host(host_kernel(name)), rel=1e-12)
    got = A.coefficients(expr, P)
    for cn, g in zip(NAMES, got):
        close(g, fixtures["%s_%s" % (name, cn)], band, name + " " + cn)
    a = fixtures["diag"] + np.sum(got[0]) + np.sum(got[2]) + got[6]
    close(a, fixtures[name + "_a"], band, name + " a")
    # resolve() of the hand-written form gives the builder's records back
    assert A.resolve(prog.records, [dict(op=o["op"], a=o["a"], b=o["b"], col=o["col"]) for o in prog.operations]) == prog.operations


def without_delta(expr, want, got):
    """delta is data, not a hyper-parameter: the kernel depends on it (the exact derivative is not zero), but its gradient
    is not built -- its column of bP is exactly zero -- so the column leaves the comparison."""
    last = expr[1][-1]
    if last["op"] == "convolve":
        assert np.all(got[:, last["col"]] == 0.0) and np.all(want[:, last["col"]] != 0.0)
        want = want.copy()
        want[:, last["col"]] = 0.0
    return want


def jacobian_check(expr, P, rng, tol=1e-12):
    """bP of the hand-written reverse for random cotangents (coefficients AND shift) vs the complex-step gradient, series by
    series, relative to the largest entry of each series' exact gradient: test_term_params.jacobian_check's criterion."""
    P = np.asarray(P, dtype=np.float64)
    co = A.coefficients(expr, P)
    cots = A.zero_inactive_rate_cotangents(expr, P, [rng.standard_normal(c.shape) for c in co[:6]])
    bshift = rng.standard_normal(P.shape[0])
    got = A.coefficients_rev(expr, P, cots, bshift)
    want = without_delta(expr, A.exact_jacobian(expr, P, cots, bshift, h=exact.H), got)
    scale = np.max(np.abs(want), axis=1, keepdims=True)
    err = np.max(np.abs(got - want) / scale)
    print("jacobian err %.2e" % err)
    assert err <= tol, err
    return got, want


@pytest.mark.parametrize("x,y", A.PRODUCTS)
def test_reverse_product(x, y):
    rng = np.random.default_rng(2000 + 7 * len(x) + len(y))
    jacobian_check(*A.draw_operation("product", x, y, rng, 256), rng)


@pytest.mark.parametrize("op", ["diff", "convolve"])
@pytest.mark.parametrize("x", ["real", "complex", "under", "over", "matern32", "rotation"])
def test_reverse_diff_and_convolve(op, x):
    rng = np.random.default_rng(3000 + len(op) + 11 * len(x))
    jacobian_check(*A.draw_operation(op, x, None, rng, 256), rng)


def test_reverse_nested_expression():
    rng = np.random.default_rng(41)
    expr, P = A.nested_expr(rng, 256)
    jacobian_check(expr, P, rng)


def test_reverse_two_leaves_share_a_column_across_a_product():
    rng = np.random.default_rng(43)
    n = 256
    a, c, d = rng.uniform(0.5, 2.0, n), rng.uniform(0.05, 0.5, n), rng.uniform(0.2, 3.0, n)
    records = [R.rec("real", (0, 1)), R.rec("complex", (0, 2, 1, 3))]        # a and c read by BOTH sides
    expr = (records, A.resolve(records, [dict(op="product", a=(0, 1, 0, 0), b=(0, 0, 0, 1))]))
    jacobian_check(expr, np.stack([a, c, 0.3 * a, d], axis=1), rng)


@pytest.mark.parametrize("top", [None, "diff", "convolve"])
def test_reverse_mixed_regime_inside_a_product(top):
    """A mixed SHO (half the series on each side of Q = 1/2) times a real term: the inactive side's amplitudes are the
    constant 0, every product amplitude built from them is 0, and the rate cotangents that reach it stay proportional to
    those amplitudes (zero_inactive_rate_cotangents prepares what a likelihood would send)."""
    rng = np.random.default_rng(47 + len(top or ""))
    n = 256
    records, P = A.join(A.draw_leaf("mixed", rng, n), A.draw_leaf("real", rng, n), A.draw_leaf("matern32", rng, n))
    ops_ = [dict(op="sum", a=A.leaf_range(records, 1), b=A.leaf_range(records, 2)), dict(op="product", a=A.leaf_range(records, 0), b=0)]
    if top == "diff":
        ops_.append(dict(op="diff", a=1))
    if top == "convolve":
        P = np.concatenate([P, A.draw_delta(rng, n)], axis=1)
        ops_.append(dict(op="convolve", a=1, col=P.shape[1] - 1))
    expr = (records, A.resolve(records, ops_))
    co = A.coefficients(expr, P)
    over = P[:, 2] < 0.5
    # complex results: [over x matern32] x 2, real x under, [under x matern32] x 2; real results: over x real
    assert np.all(co[0][~over] == 0.0) and np.all(co[2][~over][:, :2] == 0.0) and np.all(co[2][over][:, 2:] == 0.0)
    assert np.all(co[0][over] != 0.0) and np.all(co[2][~over][:, 2] != 0.0)
    jacobian_check(expr, P, rng)


@pytest.mark.parametrize("x", ["real", "complex"])
def test_reverse_shift_alone_reaches_the_parameters(x):
    """bshift -> bP with zero coefficient cotangents: the gradient of delta_diag itself.  On a real and on a general complex
    term, where delta_diag = -delta (a c - b d) / 3 + O(delta^3) is a well-conditioned function of the parameters.  (For an
    SHO or Matern-3/2 term a c = b d -- the process is differentiable, k'(0) = 0 -- so delta_diag is the O(delta^3)
    remainder of a cancellation and ITS OWN derivative is conditioned like 1 / delta^2: no evaluation in float64 can meet
    1e-12 of it in isolation.  Those leaves are covered where the shift arrives together with the coefficients' cotangents,
    in the tests above and in the likelihood's gradient.)"""
    rng = np.random.default_rng(53 + len(x))
    expr, P = A.draw_operation("convolve", x, None, rng, 256)
    zeros = [np.zeros_like(c) for c in A.coefficients(expr, P)[:6]]
    bshift = rng.standard_normal(256)
    got = A.coefficients_rev(expr, P, zeros, bshift)
    want = without_delta(expr, A.exact_jacobian(expr, P, zeros, bshift, h=exact.H), got)
    err = np.max(np.abs(got - want) / np.max(np.abs(want), axis=1, keepdims=True))
    print("shift jacobian err %.2e" % err)
    assert err <= 1e-12
    assert np.all(np.abs(want).max(axis=1) > 0)


def test_series_and_closed_forms_agree_where_they_meet():
    """|z| = 1/2 is where the convolution's power series hand over to the closed forms: both sides of it agree to rounding."""
    for th in np.linspace(0.0, np.pi / 2, 7):
        lo = 0.5 * (1 - 1e-9) * np.exp(1j * th)
        hi = 0.5 * (1 + 1e-9) * np.exp(1j * th)
        for u, v in zip(A._conv_fg(lo), A._conv_fg(hi)):
            assert abs(u - v) <= 1e-8 * abs(v)
        (Fr, Fi), (Gr, Gi) = A.conv_FG_pairs(np.array(lo.real), np.array(lo.imag))
        F, G = A._conv_fg(lo)[:2]
        assert abs(Fr + 1j * Fi - F) <= 1e-15 * abs(F) and abs(Gr + 1j * Gi - G) <= 1e-15 * abs(G)
        from celerite2_amd import terms as T
        for u, v in zip(T._conv_FG(np.array([lo, hi])), (np.array([F, A._conv_fg(hi)[0]]), np.array([G, A._conv_fg(hi)[1]]))):
            assert np.max(np.abs(u - v)) <= 1e-15


# ---- 3. the expression builder -----------------------------------------------------------------------------------------------
def test_convolution_must_be_outermost_and_delta_is_data():
    import torch
    from celerite2_amd import terms as T

    conv = T.TermConvolution(T.RealTerm(a=1.0, c=0.4), 0.05)
    real = T.RealTerm(a=1.0, c=0.1)
    for bad in (lambda: conv + real, lambda: real + conv, lambda: conv * real, lambda: real * conv, lambda: T.TermDiff(conv),
                lambda: T.TermConvolution(conv, 0.01), lambda: T.TermSum(real, conv), lambda: T.TermProduct(conv, real)):
        with pytest.raises(TypeError, match="outer term"):
            bad()
    with pytest.raises(TypeError, match="delta"):
        T.TermConvolution(real, torch.tensor(0.05, dtype=torch.float64, requires_grad=True))
    k = T.TermConvolution(T.RealTerm(a=torch.tensor(1.0, dtype=torch.float64), c=0.4), torch.tensor(0.05, dtype=torch.float64))
    assert k._has_tensors() and k.program.has_shift and k.program.operations[-1]["col"] == 2
    with pytest.raises(TypeError, match="tensor parameters"):
        k.get_coefficients()


def test_expression_is_built_once_with_shared_columns_and_its_width_checked():
    import torch
    from celerite2_amd import ops, terms as T

    t = lambda v: torch.tensor(v, dtype=torch.float64)
    c = t(0.4)
    k = T.SHOTerm(sigma=t(1.0), rho=t(2.0), Q=t(3.0), regime="under") * T.RealTerm(a=1.0, c=c) + T.RealTerm(a=t(0.3), c=c)
    prog = k.program
    assert prog is k.program and isinstance(prog, ops.TermExpr)
    assert [r["kind"] for r in prog.records] == ["sho", "real", "real"]
    assert prog.records[1]["cols"][1] == prog.records[2]["cols"][1] and prog.NP == 6      # c: ONE column, two leaves
    assert [o["op"] for o in prog.operations] == ["product", "sum"]
    assert prog.operations[0] == dict(op="product", a=(0, 0, 0, 1), b=(0, 1, 1, 0), out=(2, 0, 1, 1), col=-1)
    assert prog.operations[1]["out"] == (2, 1, 2, 1) and (prog.Jr, prog.Jc, k.width) == (1, 1, 3)
    assert tuple(k.parameter_matrix().shape) == (6,)
    # a kernel without the new classes keeps its flat program
    assert isinstance((T.RealTerm(a=t(1.0), c=0.1) + T.Matern32Term(sigma=t(0.5), rho=2.0)).program, ops.TermProgram)
    # nested sums of plain terms become ONE leaf list (no copy operation)
    k2 = (T.RealTerm(a=t(1.0), c=0.1) + T.RealTerm(a=1.0, c=0.2)) * T.RealTerm(a=1.0, c=0.3)
    assert [o["op"] for o in k2.program.operations] == ["product"] and k2.program.operations[0]["a"] == (0, 2, 0, 0)
    # widths multiply: (3 complex) x (3 complex) = 18 complex terms = 36 > 32
    three = lambda: sum((T.ComplexTerm(a=t(1.0), b=0.1, c=0.2, d=1.0 + i) for i in range(1, 3)), T.ComplexTerm(a=t(1.0), b=0.1, c=0.2, d=1.0))
    with pytest.raises(ValueError, match="width"):
        (three() * three()).program
    assert ((three() + T.RealTerm(a=1.0, c=0.1)) * T.RealTerm(a=1.0, c=0.3)).width == 7
    with pytest.raises(ValueError, match="last operation"):
        ops.TermExpr([dict(kind="real", cols=(0, 1))], [dict(op="convolve", a=(0, 1, 0, 0), col=2), dict(op="diff", a=0)], 3)
    with pytest.raises(ValueError, match="outside the registers"):
        ops.TermExpr([dict(kind="real", cols=(0, 1))], [dict(op="diff", a=(0, 2, 0, 0))], 2)


# ---- 4. the C ABI refuses bad expressions before touching the device ---------------------------------------------------------
def test_entry_points_refuse_bad_expressions_before_touching_the_device():
    import ctypes

    from celerite2_amd import _lib, build, ops

    build.build_all()
    lib = _lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)      # never dereferenced: every call below is rejected first
    records = [dict(kind="sho", cols=(0, 1, 2), regime="mixed"), dict(kind="real", cols=(0, 1))]
    expr = ops.TermExpr(records, [dict(op="product", a=(0, 2, 0, 1), b=(2, 1, 0, 0)), dict(op="convolve", a=0, col=3)], 4)
    B = 4
    need = lib.c2_term_expr_workspace_bytes(ctypes.byref(expr._c), B)
    assert need == 2 * 8 * B * (2 * (3 + 2 + 2) + 4 * (1 + 1 + 1))        # values + cotangents, [slot][series]
    assert ctypes.sizeof(expr._c) < 2048                                   # far below the 4 KiB kernel-argument limit

    def fwd(c, B=i64(B), P=one, bs=i64(4), work=one, nbytes=need):
        return lib.c2_term_expr_coefficients(ctypes.byref(c), B, P, bs, one, one, one, one, one, one, one, one, work,
                                             ctypes.c_size_t(nbytes), null)

    def rev(c, nbytes=need):
        return lib.c2_term_expr_coefficients_rev(ctypes.byref(c), i64(B), one, i64(4), one, one, one, one, one, one, null, null,
                                                 null, null, one, one, ctypes.c_size_t(nbytes), null)

    INV, UNS = _lib.C2_ERR_INVALID, _lib.C2_ERR_UNSUPPORTED
    assert fwd(expr._c, P=null) == INV and fwd(expr._c, B=i64(0)) == INV and fwd(expr._c, bs=i64(3)) == INV
    assert fwd(expr._c, work=null) == INV
    assert fwd(expr._c, nbytes=need // 2 - 8) == INV and rev(expr._c, nbytes=need - 8) == INV       # too small work_bytes
    copy = lambda: ops._TermExpr.from_buffer_copy(expr._c)
    edits = {
        "operand range beyond what has been written": lambda c: setattr(c.op[0].a, "nr", 4),
        "negative operand range": lambda c: setattr(c.op[0].b, "r0", -1),
        "operand reaches into its own result": lambda c: setattr(c.op[1].a, "nr", 3),
        "result overlaps an operand it still needs": lambda c: setattr(c.op[0].out, "r0", 2),
        "result not where the registers end": lambda c: setattr(c.op[1].out, "c0", 3),
        "result size that is not the operation's": lambda c: setattr(c.op[0].out, "nc", 2),
        "convolve not last": lambda c: (setattr(c.op[0], "op", 3), setattr(c.op[0], "col", 3)),
        "delta column outside P": lambda c: setattr(c.op[1], "col", 4),
        "unknown operation": lambda c: setattr(c.op[0], "op", 7),
        "too many operations": lambda c: setattr(c, "nops", 17),
        "register count that is not the sum": lambda c: setattr(c, "NR", 8),
        "bad leaf program": lambda c: setattr(c.leaves, "nterms", 17),
        "bad leaf regime": lambda c: setattr(c.leaves.term[0], "regime", 3),
    }
    for what, edit in edits.items():
        bad = copy()
        edit(bad)
        assert fwd(bad) == INV, what
        assert rev(bad) == INV, what
        assert lib.c2_term_expr_workspace_bytes(ctypes.byref(bad), B) == 0, what
    # width 36 > 32: (6 reals) x (6 reals), built by hand because ops.TermExpr refuses it first
    six = [dict(kind="real", cols=(0, 1))] * 12
    ok = ops.TermExpr(six, [dict(op="product", a=(0, 4, 0, 0), b=(4, 8, 0, 0))], 2)
    wide = ops._TermExpr.from_buffer_copy(ok._c)
    wide.op[0].a.nr, wide.op[0].b.r0, wide.op[0].b.nr, wide.op[0].out.nr, wide.NR = 6, 6, 6, 36, 48
    big = 2 * 8 * B * 2 * 48
    assert fwd(wide, bs=i64(2), nbytes=big) == UNS
    assert lib.c2_term_expr_coefficients_rev(ctypes.byref(wide), i64(B), one, i64(2), one, one, one, one, one, one, null, null,
                                             null, null, one, one, ctypes.c_size_t(big), null) == UNS
    with pytest.raises(ValueError, match="width"):
        ops.TermExpr(six, [dict(op="product", a=(0, 6, 0, 0), b=(6, 6, 0, 0))], 2)
    # the shift variants of the noise / mean kernels
    assert lib.c2_noise_mean_shift_apply(i64(2), i64(0), one, 1, null, null, one, one, one, one, null) == INV
    assert lib.c2_noise_mean_shift_rev(i64(2), i64(3), null, one, one, null, null, null, null, null, null) == INV
