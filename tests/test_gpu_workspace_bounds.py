# -*- coding: utf-8 -*-
"""Every mapping of the fused log-likelihood entry points stays inside the workspace size its query reports.

`work` is a view of EXACTLY the public size inside a larger buffer filled with a sentinel: an even number of doubles in
front (so `work` stays 16-byte aligned) and a tail at least as long as the largest need of any mapping for that shape
minus the public size, and never under 1024 doubles -- a dispatcher that took another mapping than the size query
reckoned with would write into memory this test owns, and be seen.  After the call flank and tail are intact and the
log-likelihood and every gradient are the float64 oracle's under the `close` rule of tests/parity_cases.py.  The mappings
are reached with the force options, so the shapes are the smallest that still exercise the layout: one series more than a
wavefront of the mapping carries, N = 2, a 32-row checkpoint segment plus one row, and two segments plus a bit."""
import ctypes
import functools

import numpy as np
import pytest

import parity_cases as P
from offset_arrays import SENTINEL, flanks_intact, off16
from parity_cases import close, dev, forced

from oracle import dense

pytestmark = pytest.mark.gpu
FLANK = 6
MAPPINGS = {1: "one", 2: "two", 4: "four", 8: "group", 9: "replay", 10: "timepar", 12: "wide", 13: "composed"}   # c2::Lanes
EVERY_FORCE = [{}, {"lanes": 1}, {"lanes": 2}, {"lanes": 4}, {"lanes": 8}, {"loglik_back": 0}, {"timepar_grad": 1}, {"timepar_grad": 0}]


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def raw():
    from celerite2_amd import _lib
    _lib.load()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    i64, out = ctypes.c_int64, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
    lib.c2_internal_loglik_grad_plan.restype, lib.c2_internal_loglik_grad_plan.argtypes = ctypes.c_int, [i64] * 3 + [ctypes.c_int] * 2 + out
    lib.c2_internal_loglik_terms_plan.restype, lib.c2_internal_loglik_terms_plan.argtypes = ctypes.c_int, [i64] * 4 + [ctypes.c_int] + out
    lib.c2_internal_loglik_grad_rows_workspace_bytes.restype = ctypes.c_size_t
    lib.c2_internal_loglik_grad_rows_workspace_bytes.argtypes = [i64] * 3
    lib.c2_internal_loglik_grad_rows.restype = ctypes.c_int
    lib.c2_internal_loglik_grad_rows.argtypes = [i64] * 3 + [ctypes.c_void_p, i64, ctypes.c_void_p, i64] + [ctypes.c_void_p] * 13 + [ctypes.c_size_t, ctypes.c_void_p]
    return lib


@pytest.fixture(autouse=True)
def no_option_left_set():
    yield
    from celerite2_amd import _lib
    left = [o["name"] for o in _lib.options() if o["is_set"]]
    for name in left:
        _lib.set_option(name, None)
    assert not left, "options still set after the test: %s" % left


def grad_plan(raw, B, N, J, allow_timepar=1, aligned16=1):
    m, need = ctypes.c_int(), ctypes.c_size_t()
    assert raw.c2_internal_loglik_grad_plan(B, N, J, allow_timepar, aligned16, ctypes.byref(m), ctypes.byref(need)) == 0
    return MAPPINGS[m.value], need.value


def largest_need(raw, B, N, J):
    """over every mapping this shape can be forced onto, either alignment, with and without the time-parallel form"""
    n = 0
    for opts in EVERY_FORCE:
        with forced(opts):
            n = max([n] + [grad_plan(raw, B, N, J, tp, al)[1] for tp in (0, 1) for al in (0, 1)])
    return n


class Guarded:
    """`work`: exactly n doubles, 16-byte aligned, between a flank and a tail of sentinels."""

    def __init__(self, n, tail):
        import torch
        self.n, self.tail = n, max(int(tail), 1024)
        self.buf = torch.full((FLANK + n + self.tail,), SENTINEL, dtype=torch.float64, device="cuda")
        self.work = self.buf[FLANK:FLANK + n]
        assert self.work.data_ptr() % 16 == 0 and self.work.numel() == n

    def intact(self):
        return bool((self.buf[:FLANK] == SENTINEL).all()) and bool((self.buf[FLANK + self.n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def case(cpu, B, N, J, gapped=False):
    """inputs and the oracle's ll and gradients, computed once per shape (`cpu`: the oracle fixture)"""
    t, c, a, U, V, y = P.problem(None, B, N, J)
    if gapped:
        # every series with a gap of its own row, c_max * gap = 30: beyond the backward guard, and more gap rows in a
        # wavefront than the one- and two-lane forward passes have extra checkpoints for (one gap row shared by the
        # wavefront would be re-anchored: tests/test_gpu_ops.py::test_one_lane_gaps_are_reanchored) -- so the groups are
        # closed and the gated fallback writes its overlay
        t = t.copy()
        for b in range(B):
            t[b, 1 + (7 * b) % (N - 1):] += 30.0 / c.max()
    ll, grads, flag = cpu.loglik_grad_batched(t, c, a, U, V, y, nthreads=2)
    assert not np.asarray(flag).any()
    return (t, c, a, U, V, y), ll, grads


def run_loglik_grad(ops, raw, oracle, B, N, J, opts, want_mapping, gapped=False, offset=()):
    inputs, llo, go = case(oracle, B, N, J, gapped)
    tail = largest_need(raw, B, N, J)
    with forced(opts):
        aligned = 0 if set(offset) & {"U", "V"} else 1
        mapping, need = grad_plan(raw, B, N, J, 1, aligned)
        assert mapping == want_mapping, (mapping, want_mapping)
        public = ops.loglik_grad_workspace(B, N, J, "cuda").numel()
        assert need <= public
        g = Guarded(public, tail - public)
        args = [off16(x) if k in offset else dev(x)[0] for k, x in zip("tcaUVy", inputs)]
        ll, grads, flag = ops.loglik_grad(*args, work=g.work)
        assert int(flag.abs().sum()) == 0
        assert g.intact(), "%s wrote outside a workspace of the public size" % mapping
        if gapped:   # head word 1 of the gate words: how many wavefronts / groups were left to the fallback
            import torch
            assert int(g.work[:2].view(torch.int64)[1]) >= 1, "the fallback did not run"
        for k, x in zip("tcaUVy", args):
            assert k not in offset or flanks_intact(x)
    close(ll, llo)
    for got, e in zip(grads, go):
        close(got, e)


@pytest.mark.parametrize("N", [2, 33, 70])
@pytest.mark.parametrize("J", [8, 6, 4, 2])
def test_one_lane(ops, raw, oracle, J, N):
    run_loglik_grad(ops, raw, oracle, 65, N, J, {"lanes": 1}, "one")


@pytest.mark.parametrize("N", [2, 33, 70])
def test_two_lanes(ops, raw, oracle, N):
    run_loglik_grad(ops, raw, oracle, 33, N, 8, {"lanes": 2}, "two")


@pytest.mark.parametrize("N", [2, 33, 70])
def test_four_lanes_and_what_unaligned_arrays_take_instead(ops, raw, oracle, N):
    run_loglik_grad(ops, raw, oracle, 17, N, 8, {"lanes": 4}, "four")
    run_loglik_grad(ops, raw, oracle, 17, N, 8, {"lanes": 4}, "group", offset=("U",))   # U 8 bytes off: the next mapping, same workspace


@pytest.mark.parametrize("N", [2, 33, 70])
@pytest.mark.parametrize("J", [3, 8, 12, 32])
def test_group_forms(ops, raw, oracle, J, N):
    run_loglik_grad(ops, raw, oracle, 9, N, J, {}, "group" if J <= 8 else "replay")
    if J <= 8:
        run_loglik_grad(ops, raw, oracle, 9, N, J, {"loglik_back": 0}, "replay")


@pytest.mark.parametrize("J", [2, 8])
def test_time_parallel_gradient(ops, raw, oracle, J):
    run_loglik_grad(ops, raw, oracle, 3, 130, J, {"timepar_grad": 1}, "timepar")


@pytest.mark.parametrize("opts,B,mapping", [({"lanes": 1}, 65, "one"), ({"lanes": 2}, 33, "two"), ({"lanes": 4}, 17, "four")])
def test_gated_fallback_writes_its_overlay(ops, raw, oracle, opts, B, mapping):
    run_loglik_grad(ops, raw, oracle, B, 70, 8, opts, mapping, gapped=True)


@pytest.mark.parametrize("opts,B,mapping", [({"lanes": 1}, 65, "one"), ({}, 9, "group"), ({"loglik_back": 0}, 9, "replay")])
def test_rows_forms(ops, raw, oracle, opts, B, mapping):
    """c2_internal_loglik_grad_rows (the 1-D pass of the interleaved 2-D gradient: never parallel along time) on a workspace
    of exactly c2_internal_loglik_grad_rows_workspace_bytes."""
    import torch
    N, J = 70, 8
    inputs, llo, go = case(oracle, B, N, J)
    tail = largest_need(raw, B, N, J)
    with forced(opts):
        assert grad_plan(raw, B, N, J, 0, 1)[0] == mapping
        n = raw.c2_internal_loglik_grad_rows_workspace_bytes(B, N, J) // 8
        g = Guarded(n, tail - n)
        t, c, a, U, V, y = dev(*inputs)
        ll = torch.empty(B, dtype=torch.float64, device="cuda")
        outs = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, N), (B, J), (B, N), (B, N, J), (B, N, J), (B, N))]
        flag = torch.zeros(B, dtype=torch.int32, device="cuda")
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        rc = raw.c2_internal_loglik_grad_rows(B, N, J, p(t), N, p(c), J, p(a), p(U), p(V), p(y), p(ll), *[p(o) for o in outs], p(flag),
                                              p(g.work), n * 8, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert int(flag.abs().sum()) == 0 and g.intact()
    close(ll, llo)
    for got, e in zip(outs, go):
        close(got, e)


@functools.lru_cache(maxsize=None)
def terms_case(cpu, B, N, Jr, Jc):
    rng = np.random.default_rng(100 * Jr + Jc)
    ar = rng.uniform(0.5, 1.5, (B, Jr)); cr = rng.uniform(0.05, 0.5, (B, Jr))
    ac = rng.uniform(0.5, 2.0, (B, Jc)); cc = rng.uniform(0.02, 0.3, (B, Jc)); dc = rng.uniform(0.2, 3.0, (B, Jc))
    bc = ac * cc / dc * rng.uniform(0.0, 0.9, (B, Jc))   # (positive semi-definite: ac cc >= bc dc)
    x = np.sort(rng.uniform(0, N / 10.0, (B, N)), axis=1)
    diag = rng.uniform(0.1, 0.3, (B, N))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    inputs = (ar, cr, ac, bc, cc, dc, x, diag, y)
    want = [dense.coefficient_chain(cpu, *[v[b] for v in inputs]) for b in range(B)]
    assert not any(w[2] for w in want)
    return inputs, np.array([w[0] for w in want]), [np.stack([w[1][k] for w in want]) for k in range(9)]


@pytest.mark.parametrize("Jr,Jc", [(2, 3), (0, 4)])
@pytest.mark.parametrize("option,B,mapping", [("terms_four_lanes", 17, "four"), ("terms_eight_lanes", 9, "group"), ("terms_two_lanes", 33, "two"),
                                              ("terms_fused", 65, "one")])
def test_coefficient_level_gradient(ops, raw, oracle, option, B, mapping, Jr, Jc):
    N = 33
    inputs, llo, go = terms_case(oracle, B, N, Jr, Jc)
    m, need = ctypes.c_int(), ctypes.c_size_t()
    with forced({option: 1}):
        assert raw.c2_internal_loglik_terms_plan(B, N, Jr, Jc, 1, ctypes.byref(m), ctypes.byref(need)) == 0
        assert MAPPINGS[m.value] == mapping
        public = ops.loglik_terms_workspace(B, N, Jr, Jc, "cuda").numel()
        assert need.value <= public
        g = Guarded(public, 0)   # (the public size is the largest need over the mappings already: the tail is the 1024)
        ll, grads, flag = ops.loglik_terms_grad(*dev(*inputs), work=g.work)
        assert int(flag.abs().sum()) == 0 and g.intact()
    close(ll, llo)
    for got, e in zip(grads, go):
        if e.size:
            close(got, e)


def test_interleaved_2d_gradient(ops, raw, oracle):
    B, N, M, J = 2, 12, 3, 4
    t, c, a, U, V, alpha, diag, y, _ = dense.kron_synthetic(B, N, M, J)
    lls, folded = [], []
    for b in range(B):   # the 1-D oracle on the interleaved series, gradients folded back (tests/test_gpu_kron.py)
        t2, c2, a2, U2, V2 = dense.kron_interleaved(c[b], a[b], U[b], V[b], t[b], alpha[b], diag[b])
        ll, g2, flag = oracle.loglik_grad(t2, c2, a2, U2, V2, np.ascontiguousarray(y[b].ravel()))
        assert flag == 0
        lls.append(ll); folded.append(dense.kron_fold_gradients(g2, a[b], U[b], V[b], alpha[b]))
    from celerite2_amd import _lib
    public = _lib.load().c2_kron_loglik_workspace_bytes(B, N, M, J, 1, 1) // 8
    g = Guarded(public, largest_need(raw, B, N * M, J))
    ll, grads, flag = ops.kron_loglik_grad(*dev(t, c, a, U, V, alpha, diag, y), method="interleaved", work=g.work)
    assert int(flag.abs().sum()) == 0 and g.intact()
    close(ll, np.array(lls))
    for k, got in enumerate(grads):
        close(got, np.stack([f[k] for f in folded]))
