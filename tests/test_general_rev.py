# -*- coding: utf-8 -*-
"""The reverse of general_matmul_lower / general_matmul_upper on the CPU: the numpy restatement of the recurrence
(tests/general_rev_ref.py, what csrc/c2_general_rev.hip implements) against the dense operator under torch autograd, the
local identities that give bt1 and bt2, and the C-ABI's argument checks, which need no device."""
import ctypes

import numpy as np
import pytest

import general_rev_ref as R

SHAPES = [(1, 1), (2, 7), (7, 2), (8, 9), (9, 8), (33, 17), (257, 300)]
WIDTHS = [1, 2, 3, 8, 16, 32]
NRHS = [1, 3, 8, 9]
NAMES = ("bt1", "bt2", "bc", "bU", "bV", "bY")


def cases():
    """Every width with every shape; the right-hand sides and grid kinds rotate so that each pairs with each width and shape."""
    out = []
    for iw, J in enumerate(WIDTHS):
        for ish, (N, M) in enumerate(SHAPES):
            out.append((J, N, M, NRHS[(iw + ish) % len(NRHS)]))
    return out


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
@pytest.mark.parametrize("kind", R.GRID_KINDS)
def test_recurrence_against_dense_autograd(kind, lower):
    """(i) against (ii): the forward value and all six cotangents within the project's criterion; the workspace rows the
    forward never wrote are NaN here, so the reverse reads none of them."""
    worst = 0.0
    for idx, (J, N, M, K) in enumerate(cases()):
        t1, t2, c, U, V, Y, bZ = (x[0] for x in R.inputs(kind, 1, N, M, J, K, 1000 + idx, lower))
        Z, F = R.forward(t1, t2, c, U, V, Y, lower)
        got = R.reverse(t1, t2, c, U, V, Y, F, bZ, lower)
        Zd, want = R.dense(t1, t2, c, U, V, Y, bZ, lower)
        worst = max(worst, R.close(Z, Zd, "Z %s" % ((J, N, M, K),)))
        for nm, g, w in zip(NAMES, got, want):
            worst = max(worst, R.close(g, w, "%s %s" % (nm, (J, N, M, K))))
        if kind == "t1_before":
            assert not np.any(Z) and all(not np.any(g) for g in got)
    print("%s %s: worst %.3g of the criterion" % (kind, "lower" if lower else "upper", worst))


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_time_cotangents_are_local(lower):
    """bt1 = -+ (U o bU) c and bt2 = +- (V o bV) c (upper sign: lower), checked on the DENSE gradients."""
    for kind in R.GRID_KINDS:
        t1, t2, c, U, V, Y, bZ = (x[0] for x in R.inputs(kind, 1, 33, 17, 3, 3, 7, lower))
        _, (bt1, bt2, bc, bU, bV, bY) = R.dense(t1, t2, c, U, V, Y, bZ, lower)
        sg = 1.0 if lower else -1.0
        R.close(bt1, -sg * (U * bU) @ c, "bt1 " + kind)
        R.close(bt2, sg * (V * bV) @ c, "bt2 " + kind)


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "upper"])
def test_event_loop_of_the_kernel(lower):
    """The kernel's event loop restated statement by statement (general_rev_ref.emulate_kernel: ring slots, requests eight
    indices ahead arriving four events later, clamping at the end of a grid, the accumulating launches of several right-hand
    sides) against the recurrence, on shapes around the ring and the unroll; a slot read before its row arrived holds NaN."""
    idx = 0
    for kind in R.GRID_KINDS:
        for N, M in SHAPES[:6] + [(60, 75), (17, 40)]:
            for J, K in ((1, 1), (3, 3), (8, 2)):
                idx += 1
                t1, t2, c, U, V, Y, bZ = (x[0] for x in R.inputs(kind, 1, N, M, J, K, idx, lower))
                _, F = R.forward(t1, t2, c, U, V, Y, lower)
                want = R.reverse(t1, t2, c, U, V, Y, F, bZ, lower)
                out = tuple(np.full(s, np.nan) for s in ((N,), (M,), (J,), (N, J), (M, J), (M, K)))
                for k in range(K):
                    R.emulate_kernel(t1, t2, c, U, V, Y, F, bZ, lower, out, k, k > 0)
                for nm, g, w in zip(NAMES, out, want):
                    R.close(g, w, "%s %s %s" % (nm, kind, (N, M, J, K)))


def test_abi_argument_errors():
    """c2_general_matmul_lower_rev / _upper_rev reject null pointers and non-positive sizes (C2_ERR_INVALID) and widths above
    C2_FAST_WIDTH (C2_ERR_UNSUPPORTED) before anything touches the device."""
    from celerite2_amd import _lib, build

    build.build_all()
    lib = _lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first
    for name in ("c2_general_matmul_lower_rev", "c2_general_matmul_upper_rev"):
        assert name in _lib.HEADERS["main"].symbols
        fn = getattr(lib, name)

        def call(B, N, M, J, K, ptrs):
            t1, t2, c = ptrs[:3]
            return fn(i64(B), i64(N), i64(M), i64(J), i64(K), t1, i64(0), t2, i64(0), c, i64(0), *ptrs[3:], null)

        ok = [one] * 14
        assert call(1, 4, 3, 2, 1, [null] * 14) == _lib.C2_ERR_INVALID
        for bad in ((0, 4, 3, 2, 1), (1, 0, 3, 2, 1), (1, 4, 0, 2, 1), (1, 4, 3, 0, 1), (1, 4, 3, 2, 0)):
            assert call(*bad, ok) == _lib.C2_ERR_INVALID, bad
        for i in range(14):   # each pointer in turn
            assert call(1, 4, 3, 2, 1, ok[:i] + [null] + ok[i + 1:]) == _lib.C2_ERR_INVALID, i
        assert call(1, 4, 3, 33, 1, ok) == _lib.C2_ERR_UNSUPPORTED
        assert call(1, 4, 3, 129, 1, [null] * 14) == _lib.C2_ERR_UNSUPPORTED
