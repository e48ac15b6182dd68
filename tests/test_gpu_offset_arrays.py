# -*- coding: utf-8 -*-
"""Arrays that start 8 bytes off a 16-byte boundary.  The C ABI promises 8-byte alignment of every double*
(include/celerite2_amd.h); eleven dispatch sites pick a kernel that moves 16-byte pieces only when the pointers allow it,
and every tensor the rest of the suite passes is aligned to 256 bytes or more, so the other side of those conditions --
and a pointer missing from one -- would go unnoticed.  Each case runs the op once with EVERY array argument (inputs and
caller-supplied outputs) through offset_arrays.off16, then once per argument with only that one offset, and compares all
results with the float64 oracle under the rule of tests/test_gpu_ops.py::close.  Offset outputs must leave the two doubles
that flank them untouched (the only bounds check here).  The reverse sweeps of `ops` allocate their outputs themselves;
`sweep_rev_into` below makes the same C call on caller-owned ones, so that bU / bV of those conditions are offset too."""
import ctypes

import numpy as np
import pytest

import parity_cases as P
from offset_arrays import empty_off16, flanks_intact, off16
from parity_cases import close, dev, forced

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(autouse=True)
def no_option_left_set():
    yield
    from celerite2_amd import _lib
    left = [o["name"] for o in _lib.options() if o["is_set"]]
    for name in left:
        _lib.set_option(name, None)
    assert not left, "options still set after the test: %s" % left


class Args:
    """The array arguments of one call: inputs (name -> numpy array) and outputs (name -> (shape, fill)).  `pick(which)`
    gives device tensors with the argument `which` -- or all of them for "all" -- 8 bytes off a 16-byte boundary and the
    others straight from the allocator; outputs are fresh for every call."""

    def __init__(self, inputs, outputs=()):
        self.inputs = dict(inputs)
        self.outputs = dict(outputs)
        self.aligned = {k: dev(v)[0] for k, v in self.inputs.items()}
        self.offset = {k: off16(v) for k, v in self.inputs.items()}
        for v in self.aligned.values():
            assert v.data_ptr() % 16 == 0

    def variants(self):
        return ["all"] + list(self.inputs) + list(self.outputs)

    def pick(self, which, fresh=()):
        """`fresh`: inputs the call overwrites (in place), copied anew."""
        import torch
        out = {}
        for k in self.inputs:
            off = which in ("all", k)
            if k in fresh:
                out[k] = off16(self.inputs[k]) if off else dev(self.inputs[k])[0]
            else:
                out[k] = self.offset[k] if off else self.aligned[k]
        for k, (shape, fill) in self.outputs.items():
            if which in ("all", k):
                out[k] = empty_off16(shape, fill)
            else:
                out[k] = torch.full(tuple(shape), fill, dtype=torch.float64, device="cuda")
        return out

    @staticmethod
    def flanks(picked):
        for k, v in picked.items():
            if hasattr(v, "guard_buffer"):
                assert flanks_intact(v), "the doubles around %s were written" % k


NAN = float("nan")


def offset_forward(ops, case, name, modes):
    """One forward sweep of a case with offset arguments, in the given forms ("F": with the workspace, "noF", "inplace":
    Z is Y)."""
    matmul = name.startswith("matmul")
    w = case.want[name]
    B, N, J, nrhs = case.B, case.N, case.J, case.nrhs
    ins = dict(t=case.t, c=case.c, U=case.U, A=P.second(case, name), Y=case.Y)
    kw = dict(zero_z=True) if matmul else {}
    op = getattr(ops, name)
    if "F" in modes:
        A = Args(ins, dict(Z=((B, N, nrhs), NAN), F=((B, N, J, nrhs), NAN)))
        for which in A.variants():
            p = A.pick(which)
            Z, F = op(p["t"], p["c"], p["U"], p["A"], p["Y"], Z=p["Z"], F=p["F"], **kw)
            close(Z, w.Z); close(F, w.F); A.flanks(p)
    if "noF" in modes:
        A = Args(ins, dict(Z=((B, N, nrhs), NAN)))
        for which in A.variants():
            p = A.pick(which)
            close(op(p["t"], p["c"], p["U"], p["A"], p["Y"], Z=p["Z"], **kw), w.Z); A.flanks(p)
    if "inplace" in modes:
        A = Args(ins)
        for which in A.variants():
            p = A.pick(which, fresh=("Y",))
            Z = op(p["t"], p["c"], p["U"], p["A"], p["Y"], Z=p["Y"])
            assert Z.data_ptr() == p["Y"].data_ptr()
            close(Z, w.Z + case.Y if matmul else w.Z); A.flanks(p)


def sweep_rev_into(ops, name, t, c, U, A, Y, Z, F, bZ, bt, bc, bU, bA, bY):
    """ops.<name>_rev (celerite2_amd/ops.py, _sweep_rev) writing into caller-owned outputs: the same C call."""
    from celerite2_amd import _lib
    B, N, J = U.shape
    nrhs = Y.shape[-1]
    ops._chk(t, c, U, A, Y, Z, F, bZ, bt, bc, bU, bA, bY)
    i64, p = ctypes.c_int64, ops._p
    rc = getattr(_lib.load(), "c2_" + name + "_rev")(
        i64(B), i64(N), i64(J), i64(nrhs), p(t), i64(ops._bs(t, N)), p(c), i64(ops._bs(c, J)), p(U), p(A), p(Y), p(Z), p(F),
        p(bZ), p(bt), p(bc), p(bU), p(bA), p(bY), ops._stream())
    _lib.check(rc, name + "_rev")
    return bt, bc, bU, bA, bY


def offset_reverse(ops, case, name):
    w = case.want[name]
    B, N, J, nrhs = case.B, case.N, case.J, case.nrhs
    A = Args(dict(t=case.t, c=case.c, U=case.U, A=P.second(case, name), Y=case.Y, Z=w.Z, F=w.F, bZ=case.bZ),
             dict(bt=((B, N), NAN), bc=((B, J), NAN), bU=((B, N, J), NAN), bA=((B, N, J), NAN), bY=((B, N, nrhs), NAN)))
    for which in A.variants():
        p = A.pick(which)
        res = sweep_rev_into(ops, name, *[p[k] for k in ("t", "c", "U", "A", "Y", "Z", "F", "bZ", "bt", "bc", "bU", "bA", "bY")])
        P.check_reverse(case, name, res); A.flanks(p)
    # ... and through ops itself (its own outputs, every input offset)
    p = A.pick("all")
    P.check_reverse(case, name, getattr(ops, name + "_rev")(*[p[k] for k in ("t", "c", "U", "A", "Y", "Z", "F", "bZ")]))


@pytest.mark.parametrize("N", [3, 4, 9, 10])
def test_single_rhs_sweeps_at_width_8(ops, oracle, N):
    """c2_sweep.hip:778 and :821: an offset U or V (:821 also F, bU, bV) sends the single-rhs sweeps at J = 8 from the
    128-byte-line kernels k_sweep1<8, 8, ..., LN> / k_sweep1_rev<8, 8, ..., LN> to the row-by-row instances
    k_sweep1<8, 8, ..., false> / k_sweep1_rev<8, 8, ..., false>; an offset t, c, Y, Z (and F of the forward sweep) stays on
    the lines, which move those one double at a time.  B = 9: a full wavefront of eight series and a ragged one."""
    case = P.sweep_case(oracle, 700 + N, 9, N, 8, 1)
    for name in P.SWEEPS:
        offset_forward(ops, case, name, ("F", "noF", "inplace"))
        offset_reverse(ops, case, name)


@pytest.mark.parametrize("N", [8, 9, 33])
@pytest.mark.parametrize("B", [8, 13])
def test_eight_rhs_sweeps_at_width_8(ops, oracle, B, N):
    """c2_sweep.hip:875-879 and c2_sweep_rev.hip:490: nrhs = J = 8 from eight series and eight rows.  Any of U, V, Y, Z, F
    (reverse: also bZ, bU, bV, bY) off a 16-byte boundary sends the whole batch from k_sweep8_lines / k_sweep8_rev_lines to
    k_sweepK<8, 8, ...> / k_sweepK_rev<8, 8>; an offset F makes c2_internal_sweepK decline altogether (:875: the workspace
    goes through the LDS tile as whole rows) for k_sweep<8, 4>, and c2_internal_sweepK_rev too (c2_sweep_rev.hip:483) for
    k_sweep_rev<8, 4>.  B = 13: the lines take eight series, the row-by-row kernel the other five."""
    case = P.sweep_case(oracle, 800 + 10 * B + N, B, N, 8, 8)
    for name in P.SWEEPS:
        offset_forward(ops, case, name, ("F", "noF", "inplace"))
        offset_reverse(ops, case, name)


@pytest.mark.parametrize("N", [8, 11, 33])
@pytest.mark.parametrize("nrhs", [9, 12, 16, 17, 24])
def test_nine_to_24_rhs_sweeps_at_width_8(ops, oracle, nrhs, N):
    """c2_sweep_cols.hip:637-639 and :673-680: nine to 32 right-hand sides at J = 8 on whole wavefronts of eight series.  An
    offset U or V (reverse: or F, bU, bV) makes c2_internal_sweep_cols[_rev] decline for k_sweepK<16 / 32, 8, ...> and
    k_sweepK_rev<16, 8> (nrhs <= 16) or k_sweep_rev<8, 4>; an offset Y or Z (reverse: or bZ, bY) keeps k_sweepC<NC> /
    k_sweepC_rev<2 / 1> but on their one-double instances (v2 / al16 false), as an odd nrhs does.  17 and 24 right-hand sides
    run the reverse as two column slices, the second one column per lane.  B = 8 and 13 share a case: 13 = the eight
    series of these kernels + five on the kernels behind them."""
    for B in (8, 13):
        case = P.sweep_case(oracle, 900 + 100 * nrhs + 10 * B + N, B, N, 8, nrhs)
        for name in P.SWEEPS:
            offset_forward(ops, case, name, ("noF", "inplace"))
            offset_reverse(ops, case, name)


@pytest.mark.parametrize("J", [4, 8, 16])
@pytest.mark.parametrize("nrhs", [5, 8, 16])
def test_reverse_sweeps_with_lanes_over_the_right_hand_sides(ops, oracle, nrhs, J):
    """c2_sweep_rev.hip:483: k_sweepK_rev<KL, JM> loads the workspace columns 16 bytes at a time, so an offset F makes
    c2_internal_sweepK_rev decline for k_sweep_rev<G, 4>; every other argument offset stays on k_sweepK_rev."""
    for N in (2, 9):
        case = P.sweep_case(oracle, 1100 + 100 * nrhs + 10 * J + N, 5, N, J, nrhs)
        for name in P.SWEEPS:
            offset_reverse(ops, case, name)


@pytest.mark.parametrize("N", [2, 9, 33])
@pytest.mark.parametrize("J", [2, 4, 8, 16])
def test_factor_with_workspace(ops, oracle, J, N):
    """c2_ops.hip:1778-1784: an offset S sends factor(workspace=True) at J = 2, 4, 8, 16 from the fused forward kernel +
    k_s_replay<G, ...> (16-byte stores of the S rows) to the row-by-row k_factor<G>; an offset W at J = 8 keeps the replay
    but on k_s_replay<8, false> (:1784).  Every argument offset alone and all together, one series failing."""
    B = 9
    case = P.factor_case(oracle, B, N, J, fail=(4, N // 2))
    A = Args(dict(t=case.t, c=case.c, a=case.a, U=case.U, V=case.V),
             dict(d=((B, N), NAN), W=((B, N, J), NAN), S=((B, N, J, J), NAN)))
    for which in A.variants():
        p = A.pick(which)
        d, W, S, flag = ops.factor(p["t"], p["c"], p["a"], p["U"], p["V"], d=p["d"], W=p["W"], S=p["S"])
        P.check_factor(case, d, W, S, flag); A.flanks(p)


@pytest.mark.parametrize("nrhs", [4, 8])
def test_general_matmul_with_workspace(ops, oracle, nrhs):
    """c2_general.hip:136 (`dense_f`, decided inside k_generalK<8, 8, LOWER, true>): whole F rows leave through the LDS
    tile 16 bytes at a time only if F allows it, element by element otherwise.  Small batches are k_general_tile's
    (c2_general_tile.hip) by default, so each variant runs on the default dispatch and again with general_tile = 0, where
    k_generalK answers."""
    B, N, M, J = 4, 17, 33, 8
    case = P.general_case(oracle, 1200 + nrhs, B, N, M, J, nrhs)
    A = Args(dict(t1=case.t1, t2=case.t2, c=case.c, U=case.U, V=case.V, Y=case.Y, Z=case.Z0),
             dict(F=((B, M, J, nrhs), 3.0)))
    for opts in ({}, {"general_tile": 0}):
        for name in ("general_matmul_lower", "general_matmul_upper"):
            for which in A.variants():
                p = A.pick(which, fresh=("Z",))
                with forced(opts):
                    Z, F = getattr(ops, name)(p["t1"], p["t2"], p["c"], p["U"], p["V"], p["Y"], Z=p["Z"], F=p["F"])
                close(Z, case.want[name].Z); close(F, case.want[name].F); A.flanks(p)


@pytest.mark.parametrize("nrhs", [8, 32])
@pytest.mark.parametrize("J", [8, 16])
def test_chunked_products(ops, oracle, J, nrhs):
    """c2_scan.hip:205-206 (`fast`): k_mm_chunk<G, 4, 8, LOWER, FINAL, true> fetches the eight values of a column group of
    Y with one 16-byte request per lane pair -- taken at J = 8 / 16 when nrhs is a multiple of the slab of 32 and Y, Z are
    16-byte aligned; an offset Y or Z takes k_mm_chunk<..., false>.  Eight right-hand sides run k_mm_chunk<G, 1, 4, ...,
    false> whatever the alignment (no 16-byte pieces at all): kept as the plain case.  scan_min_rows = 256 lets 300 rows
    take the chunked path (c2_ops.hip:1377)."""
    case = P.sweep_case(oracle, 1300 + 10 * J + nrhs, 2, 300, J, nrhs)
    with forced({"scan_min_rows": 256}):
        for name in ("matmul_lower", "matmul_upper"):
            offset_forward(ops, case, name, ("F", "noF", "inplace"))


LOGLIK_SETTINGS = [
    # (id, options, B, J, floor of the gradients)
    ("auto", {}, 9, 8, 1e-12),
    ("lanes8", {"lanes": 8}, 9, 8, 1e-12),
    ("lanes4_rows", {"lanes": 4, "loglik_q4_lines": 0}, 17, 8, 1e-12),
    ("lanes4_lines", {"lanes": 4, "loglik_q4_lines": 1}, 17, 8, 1e-12),
    ("lanes2", {"lanes": 2}, 33, 8, 4e-12),   # (the floor tests/test_gpu_fuzz.py::test_fuzz_two_lane_kernels uses)
    ("lanes1_J8", {"lanes": 1}, 65, 8, 1e-12),
    ("lanes1_J6", {"lanes": 1}, 65, 6, 1e-12),
    ("lanes1_J4", {"lanes": 1}, 65, 4, 1e-12),
    ("lanes1_J2", {"lanes": 1}, 65, 2, 1e-12),
]
GRADS = ("bt", "bc", "ba", "bU", "bV", "by")


@pytest.mark.parametrize("N", [9, 33, 65])
@pytest.mark.parametrize("setting", LOGLIK_SETTINGS, ids=[s[0] for s in LOGLIK_SETTINGS])
def test_loglik_and_gradient(ops, oracle, setting, N):
    """c2_loglik.hip:1784 (`aligned16`): the four-lane gradient pair (k_q4_fwd / k_q4_rev, c2_loglik_q4.hip) moves U, V, bU,
    bV, bc and its records as double2, so any of U, V, bU, bV, bc or the workspace off a 16-byte boundary takes the
    eight-lane pair (loglik_grad_group) on the same workspace; t, a, y, bt, ba, by offset stay on four lanes.  The other
    lane mappings -- eight lanes, two (c2_loglik_k2.hip), one (c2_loglik_t.hip, widths 8, 6, 4, 2) -- have no such
    condition: they must simply be right on such arrays.  N is odd, as in t[1:], a[1:], y[1:] of a real batch.
    Log-likelihood, flags, all six gradients; `work=` and `out=` are the caller's."""
    _, opts, B, J, floor = setting
    case = P.loglik_case(oracle, B, N, J)
    shapes = dict(bt=(B, N), bc=(B, J), ba=(B, N), bU=(B, N, J), bV=(B, N, J), by=(B, N))
    with forced(opts):
        nwork = ops.loglik_grad_workspace(B, N, J, "cuda").numel()
        A = Args(dict(t=case.t, c=case.c, a=case.a, U=case.U, V=case.V, y=case.y),
                 dict([("work", ((nwork,), 0.0))] + [(k, (shapes[k], NAN)) for k in GRADS]))
        for which in A.variants():
            p = A.pick(which)
            args = [p[k] for k in ("t", "c", "a", "U", "V", "y")]
            ll, grads, flag = ops.loglik_grad(*args, work=p["work"], out=tuple(p[k] for k in GRADS))
            assert int(flag.abs().sum()) == 0, which
            close(ll, case.ll)
            for g, e in zip(grads, case.grads):
                close(g, e, floor=floor)
            A.flanks(p)
            if which in ("all", "t", "c", "a", "U", "V", "y"):
                ll0, flag0 = ops.loglik(*args)
                assert int(flag0.abs().sum()) == 0, which
                close(ll0, case.ll)


def test_slices_of_an_ordinary_batch(ops, oracle):
    """What a user does: a batch of B + 1 series of nine rows (J = 3, three right-hand sides) as ordinary tensors, and every
    op on the [1:] slices -- views that ops._chk accepts and that start 8 bytes off a 16-byte boundary because N, N J,
    N nrhs, J, N J nrhs and N J J are odd.  factor with and without S, the four sweeps with F and their reverses,
    loglik_grad into slices of the caller's arrays."""
    import torch
    B, N, J, nrhs = 6, 9, 3, 3
    sw = P.sweep_case(oracle, 1400, B + 1, N, J, nrhs)
    fc = P.factor_case(oracle, B + 1, N, J)
    full = dev(fc.t, fc.c, fc.a, fc.U, fc.V, fc.y)
    t, c, a, U, V, y = [x[1:] for x in full]
    for x in (t, c, a, U, V, y):
        assert x.is_contiguous() and x.data_ptr() % 16 == 8
    empty = lambda *shape: torch.full((B + 1,) + shape, NAN, dtype=torch.float64, device="cuda")[1:]
    d, W, S = empty(N), empty(N, J), empty(N, J, J)
    for x in (d, W, S):
        assert x.data_ptr() % 16 == 8
    d, W, S, flag = ops.factor(t, c, a, U, V, d=d, W=W, S=S)
    assert int(flag.abs().sum()) == 0
    close(d, fc.d[1:]); close(W, fc.W[1:]); close(S, fc.S[1:])
    d2, W2, flag2 = ops.factor(t, c, a, U, V, d=empty(N), W=empty(N, J))
    close(d2, fc.d[1:]); close(W2, fc.W[1:])
    st, sc, sU, sY, sbZ = [x[1:] for x in dev(sw.t, sw.c, sw.U, sw.Y, sw.bZ)]
    for name in P.SWEEPS:
        sA = dev(P.second(sw, name))[0][1:]
        kw = dict(zero_z=True) if name.startswith("matmul") else {}
        Z, F = getattr(ops, name)(st, sc, sU, sA, sY, Z=empty(N, nrhs), F=empty(N, J, nrhs), **kw)
        assert all(x.data_ptr() % 16 == 8 for x in (st, sc, sU, sA, sY, Z, F, sbZ))
        close(Z, sw.want[name].Z[1:]); close(F, sw.want[name].F[1:])
        res = getattr(ops, name + "_rev")(st, sc, sU, sA, sY, Z, F, sbZ)
        for b in range(B):
            for g, w in zip(res, sw.want[name].rev):
                close(g[b], w[b + 1])
    llo, go, flago = oracle.loglik_grad_batched(fc.t, fc.c, fc.a, fc.U, fc.V, fc.y, nthreads=2)
    assert not np.asarray(flago).any()
    out = (empty(N), empty(J), empty(N), empty(N, J), empty(N, J), empty(N))
    ll, grads, flag = ops.loglik_grad(t, c, a, U, V, y, out=out)
    assert int(flag.abs().sum()) == 0
    close(ll, llo[1:])
    for g, e in zip(grads, go):
        close(g, e[1:])
