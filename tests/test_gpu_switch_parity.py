# -*- coding: utf-8 -*-
"""Both sides of the dispatch switches no other test sets (csrc/c2_dispatch.hpp: "every alternative is parity-tested, so a
switch changes speed, never results beyond rounding").  Each case runs the default side and the forced side on the
smallest shapes that still reach the branch, and compares EACH with the float64 oracle under the rule of
tests/test_gpu_ops.py::close (1e-10 relative, floor 1e-12 of the largest entry).  Options are process-global: they are set
through parity_cases.forced (try / finally) and a module-local fixture asserts after every test that none is left set.
tests/test_switch_parity_table.py checks on the CPU that every switch of the table is in SWITCH_CASES, COVERED_ELSEWHERE or
EXEMPT."""
import numpy as np
import pytest

import parity_cases as P
from parity_cases import close, dev, forced

pytestmark = pytest.mark.gpu

# option -> (the forced side, the shapes, what runs there).  The test of an option is test_<option> below.
SWITCH_CASES = {
    "sweep1_lines": dict(force={"sweep1_lines": 0}, J=8, nrhs=1, B=(3, 9), N=(3, 4, 9, 10, 33),
                         runs="c2_sweep.hip:778 false -> k_sweep1<8, 8, LOWER, SOLVE, false> (rows one by one)"),
    "sweep1_rev_lines": dict(force={"sweep1_rev_lines": 0}, J=8, nrhs=1, B=(3, 9), N=(3, 4, 9, 10, 33),
                             runs="c2_sweep.hip:821 false -> k_sweep1_rev<8, 8, LOWER, SOLVE, false>"),
    "s_replay_lines": dict(force={"s_replay_lines": 0}, J=8, B=(3, 9), N=(1, 2, 9, 16, 17, 33),
                           runs="c2_ops.hip:1784 false -> k_s_replay<8, false>"),
    "sweept": dict(force={"sweept": 0}, nrhs=(2, 3, 4, 5), nrhs_F=(2, 3), J=(1, 3, 8, 12, 32), B=5, N=(2, 9, 40),
                   runs="c2_sweep_small.hip:179 declines -> k_sweep<G, 2> (nrhs = 2), k_sweepK<8, 8> (3 .. 5, J <= 8; "
                        "with F: J = 8), k_sweep<G, 4> (the rest)"),
    "sweept_rev": dict(force={"sweept_rev": 0}, nrhs=(2, 3, 4, 7), J=(1, 3, 8, 12, 32), B=5, N=(2, 9, 40),
                       runs="c2_sweep_small_rev.hip:232 declines -> k_sweep_rev<G, 4> (nrhs <= 4), k_sweepK_rev<8, 8> "
                            "(nrhs = 7, J = 8)"),
    "sweepk_rev": dict(force={"sweepk_rev": 0}, nrhs=(5, 8, 16), J=(4, 8, 16), B=(3, 9), N=(2, 9, 40),
                       runs="c2_ops.hip:1720 false -> k_sweep_rev<G, 4>; nrhs = 5 at J = 8 is taken by k_sweepT_rev first, "
                            "so that combination also sets sweept_rev = 0"),
    # test_gpu_general_rev.py produces its F with generalk = 0 but compares Z with a dense product and F only through the
    # reverse pass, not element by element with the oracle: the row is kept
    "generalk": dict(force={"generalk": 0, "general_tile": 0}, nrhs=(3, 5, 8), J=(3, 8), NM=((1, 1), (17, 33), (130, 100)),
                     B=4, runs="c2_ops.hip:1604 / :1623 false -> k_gm_state<G, 4> + k_gm_emit<G> (F given), "
                               "k_general<G, 4> (no F, nrhs > C2_GM_TWO_PHASE_MAX_NRHS)"),
    "scan_min_chunk": dict(force=({"scan_min_chunk": 64}, {"scan_min_chunk": 128}, {"scan_min_chunk": 256}),
                           with_={"scan_min_rows": 256}, B=2, N=(257, 511, 1030), J=(5, 8, 16), nrhs=(1, 5, 8),
                           runs="c2_ops.hip:1465 -> k_mm_chunk / k_mm_carry with Lc = 64, 128, 256 (automatic: 64 at "
                                "these lengths); powers of two only, as the automatic rule produces"),
    "timepar_cond_limit": dict(B=3, N=200, J=(8, 3),
                               runs="c2_timepar_grad.hip:370 true -> the gate opens: c2_internal_loglik_grad_replay "
                                    "(:1179, loglik_grad) and c2_internal_factor_rev_replay (:1787, factor_rev) recompute"),
}

# switches other test files set to both sides: option -> a file whose text names it (checked by the table test)
COVERED_ELSEWHERE = {
    "lanes": "test_gpu_ops.py", "loglik_back": "test_gpu_ops.py", "loglik_q4_lines": "test_gpu_ops.py",
    "timepar": "test_gpu_timepar.py", "timepar_grad": "test_gpu_timepar.py", "factor_iter": "test_gpu_timepar.py",
    "factor_scan8": "test_gpu_timepar.py", "tpg_rows": "test_gpu_timepar.py", "rev_long": "test_gpu_timepar.py",
    "sweep_cols": "test_gpu_ops.py", "solve_cols": "test_gpu_ops.py", "mfma": "test_gpu_ops.py",
    "kernel_values_tile": "test_gpu_ops.py", "general_tile": "test_gpu_ops.py", "general_chunks": "test_gpu_ops.py",
    "general_rhs_chunks": "test_gpu_ops.py", "sweepk_lines": "test_gpu_ops.py", "sweep_rev_lines": "test_gpu_ops.py",
    "terms_fused": "test_gpu_terms.py", "terms_two_lanes": "test_gpu_terms.py", "terms_eight_lanes": "test_gpu_terms.py",
    "terms_four_lanes": "test_gpu_terms.py", "kron_banded": "test_gpu_kron.py",
}

# switches that get no result test, and why
EXEMPT = {
    "verify_fallback": "a diagnostic: 0 keeps a result the device-side verification has rejected, so there is no "
                       "result to hold it to",
}


def _shapes(option, key):
    """A case's values for a parametrize mark; empty (the test then does not run, and tests/test_switch_parity_table.py
    fails on the CPU) if the option has left SWITCH_CASES."""
    return SWITCH_CASES.get(option, {}).get(key, ())


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
    for name in left:   # (put back before failing, so one leak does not fail every later test)
        _lib.set_option(name, None)
    assert not left, "options still set after the test: %s" % left


def sides(option, extra=None):
    """The option sets of a case: the default side (None) and every forced side, each with the case's `with_` options."""
    case = SWITCH_CASES[option]
    force = case["force"] if isinstance(case["force"], tuple) else (case["force"],)
    base = dict(case.get("with_", {}))
    return [dict(base)] + [dict(base, **f, **(extra or {})) for f in force]


@pytest.mark.parametrize("N", _shapes("sweep1_lines", "N"))
@pytest.mark.parametrize("B", _shapes("sweep1_lines", "B"))
def test_sweep1_lines(ops, oracle, B, N):
    """c2_sweep.hip:778 (`lines_ok`): with sweep1_lines = 0 the single-rhs forward sweeps at J = 8 leave
    k_sweep1<8, 8, ..., false, LN = 0 / 1> (rows by aligned 128-byte lines) for k_sweep1<8, 8, LOWER, SOLVE, false>, which
    requests its two rows per step one by one.  N = 3 is the shortest series the lines take; odd and even N enter the
    upper sweeps' lines at different positions; B = 9 leaves a ragged wavefront."""
    case = P.sweep_case(oracle, 100 * B + N, B, N, 8, 1)
    for opts in sides("sweep1_lines"):
        with forced(opts):
            for name in P.SWEEPS:
                P.check_forward_modes(ops, case, name)


@pytest.mark.parametrize("N", _shapes("sweep1_rev_lines", "N"))
@pytest.mark.parametrize("B", _shapes("sweep1_rev_lines", "B"))
def test_sweep1_rev_lines(ops, oracle, B, N):
    """c2_sweep.hip:821: with sweep1_rev_lines = 0 the single-rhs reverse sweeps at J = 8 leave
    k_sweep1_rev<8, 8, ..., false, LN> (five rows per step as 128-byte lines) for k_sweep1_rev<8, 8, LOWER, SOLVE, false>
    (c2_sweep.hip:836-858), row by row."""
    case = P.sweep_case(oracle, 200 * B + N, B, N, 8, 1)
    for opts in sides("sweep1_rev_lines"):
        with forced(opts):
            for name in P.SWEEPS:
                P.run_reverse(ops, case, name)


@pytest.mark.parametrize("N", _shapes("s_replay_lines", "N"))
@pytest.mark.parametrize("B", _shapes("s_replay_lines", "B"))
def test_s_replay_lines(ops, oracle, B, N):
    """c2_ops.hip:1784: with s_replay_lines = 0 the S rows of factor(workspace=True) at J = 8 come from
    k_s_replay<8, false> (one request per row for t, d and W) instead of k_s_replay<8, true> (transposed tiles, 128-byte
    lines).  d, W, S and the flags, one series failing in the middle (its S rows are not compared; the others' are)."""
    case = P.factor_case(oracle, B, N, 8, fail=(1, N // 2) if N >= 2 else None)
    if N >= 2:
        assert case.flag[1] != 0 and case.ok.sum() == B - 1
    args = dev(case.t, case.c, case.a, case.U, case.V)
    for opts in sides("s_replay_lines"):
        with forced(opts):
            d, W, S, flag = ops.factor(*args, workspace=True)
        P.check_factor(case, d, W, S, flag)


@pytest.mark.parametrize("N", _shapes("sweept", "N"))
@pytest.mark.parametrize("J", _shapes("sweept", "J"))
def test_sweept(ops, oracle, J, N):
    """c2_sweep_small.hip:179: with sweept = 0 c2_internal_sweepT declines the forward sweeps with two to five right-hand
    sides (two or three with F) and launch_sweep (c2_ops.hip:1527-1560) goes on: nrhs = 2 reaches k_sweep<G, 2> (the only
    shape besides N = 1 that does), 3 .. 5 reach k_sweepK<8, 8, ...> at J <= 8 (with F: only J = 8, whole workspace rows)
    and k_sweep<G, 4> at the other widths."""
    cfg = SWITCH_CASES["sweept"]
    for nrhs in cfg["nrhs"]:
        case = P.sweep_case(oracle, 1000 * J + 10 * N + nrhs, cfg["B"], N, J, nrhs, shared_t=(nrhs == 3))
        for opts in sides("sweept"):
            with forced(opts):
                for name in P.SWEEPS:
                    P.check_forward_modes(ops, case, name, with_F=nrhs in cfg["nrhs_F"])


@pytest.mark.parametrize("N", _shapes("sweept_rev", "N"))
@pytest.mark.parametrize("J", _shapes("sweept_rev", "J"))
def test_sweept_rev(ops, oracle, J, N):
    """c2_sweep_small_rev.hip:232: with sweept_rev = 0 c2_internal_sweepT_rev declines and launch_sweep_rev
    (c2_ops.hip:1699-1728) goes on: two to four right-hand sides reach k_sweep_rev<G, 4> (c2_internal_sweepK_rev wants
    five), seven at J = 8 reach k_sweepK_rev<8, 8>.  At the other widths k_sweepT_rev declines seven on either side (it
    takes more than four only on groups of eight lanes): k_sweepK_rev<16, 16> at J = 12, k_sweep_rev<G, 4> at J = 1, 3, 32."""
    cfg = SWITCH_CASES["sweept_rev"]
    for nrhs in cfg["nrhs"]:
        case = P.sweep_case(oracle, 2000 * J + 10 * N + nrhs, cfg["B"], N, J, nrhs, shared_t=(nrhs == 3))
        for opts in sides("sweept_rev"):
            with forced(opts):
                for name in P.SWEEPS:
                    P.run_reverse(ops, case, name)


@pytest.mark.parametrize("N", _shapes("sweepk_rev", "N"))
@pytest.mark.parametrize("J", _shapes("sweepk_rev", "J"))
@pytest.mark.parametrize("B", _shapes("sweepk_rev", "B"))
def test_sweepk_rev(ops, oracle, B, J, N):
    """c2_ops.hip:1720: with sweepk_rev = 0 the reverse sweeps with 5, 8, 16 right-hand sides leave k_sweepK_rev<KL, JM>
    (lanes over the right-hand sides; k_sweep8_rev_lines at nrhs = J = 8 from eight series) for k_sweep_rev<G, 4>
    (c2_ops.hip:1726), which loops over tiles of four columns.  Five right-hand sides at J = 8 are k_sweepT_rev's
    (c2_ops.hip:1699) before the switch is asked: that combination sets sweept_rev = 0 as well.  Sixteen at J = 8 belong to
    c2_sweep_cols.hip from eight series on (B = 9: its ninth series takes this branch, B = 3: all do)."""
    for nrhs in SWITCH_CASES["sweepk_rev"]["nrhs"]:
        case = P.sweep_case(oracle, 3000 * J + 100 * B + 10 * N + nrhs, B, N, J, nrhs)
        extra = {"sweept_rev": 0} if (nrhs == 5 and J == 8) else None
        for opts in sides("sweepk_rev", extra):
            with forced(opts):
                for name in P.SWEEPS:
                    P.run_reverse(ops, case, name)


@pytest.mark.parametrize("N,M", _shapes("generalk", "NM"))
@pytest.mark.parametrize("J", _shapes("generalk", "J"))
def test_generalk(ops, oracle, J, N, M):
    """c2_ops.hip:1604 and :1623: with general_tile = 0 and generalk = 0 neither k_general_tile nor k_generalk<KL, JM> takes
    general_matmul_lower/upper; with F the two data-parallel phases k_gm_state<G, 4> + k_gm_emit<G> run (c2_ops.hip:1647-1656),
    without F and more right-hand sides than the two phases take, the sequential merge k_general<G, 4> (:1641).  Z
    (accumulated into other numbers) and every element of F -- rows the merge never visits keep their 3 -- against the
    oracle."""
    cfg = SWITCH_CASES["generalk"]
    for nrhs in cfg["nrhs"]:
        case = P.general_case(oracle, 4000 * J + 10 * N + nrhs, cfg["B"], N, M, J, nrhs)
        t1d, t2d, cd, Ud, Vd, Yd = dev(case.t1, case.t2, case.c, case.U, case.V, case.Y)
        for opts in sides("generalk"):
            with forced(opts):
                for name in ("general_matmul_lower", "general_matmul_upper"):
                    (Zd,) = dev(case.Z0); (Fd,) = dev(np.full((case.B, M, J, nrhs), 3.0))
                    Zd, Fd = getattr(ops, name)(t1d, t2d, cd, Ud, Vd, Yd, Z=Zd, F=Fd)
                    close(Zd, case.want[name].Z); close(Fd, case.want[name].F)
                    (Zd,) = dev(case.Z0)
                    close(getattr(ops, name)(t1d, t2d, cd, Ud, Vd, Yd, Z=Zd), case.want[name].Z)


@pytest.mark.parametrize("N", _shapes("scan_min_chunk", "N"))
@pytest.mark.parametrize("J", _shapes("scan_min_chunk", "J"))
def test_scan_min_chunk(ops, oracle, J, N):
    """c2_ops.hip:1465: scan_min_chunk replaces the automatic chunk length of the chunked products (c2_scan.hip: k_mm_chunk,
    k_mm_carry, k_mm_chunk<FINAL>), 64 at these lengths, by 64, 128 and 256 -- one to seventeen chunks, the last one
    ragged or a single row (N = 257).  scan_min_rows = 256 lets series this short take the chunked path at all
    (c2_ops.hip:1377).  run_chunked computes ceil(N / Lc) chunks for any Lc, but the dispatcher itself only ever produces
    powers of two, so no other length is added.  Both products, with and without F, zero_z both ways."""
    cfg = SWITCH_CASES["scan_min_chunk"]
    for nrhs in cfg["nrhs"]:
        case = P.sweep_case(oracle, 5000 * J + 10 * N + nrhs, cfg["B"], N, J, nrhs)
        for opts in sides("scan_min_chunk"):
            with forced(opts):
                for name in ("matmul_lower", "matmul_upper"):
                    P.check_forward_modes(ops, case, name)


def _max_finite(x):
    x = x.cpu().numpy()
    return float(x[np.isfinite(x)].max())


def _bits_equal(xs, ys):
    import torch
    return all(torch.equal(x, y) or bool(((x == y) | (x.isnan() & y.isnan())).all()) for x, y in zip(xs, ys))


@pytest.mark.parametrize("J", _shapes("timepar_cond_limit", "J"))
def test_timepar_cond_limit(ops, oracle, J):
    """c2_timepar_grad.hip:370 (k_verify_combine): a conditioning kappa = max a_n / d_n beyond timepar_cond_limit opens the
    gate behind which the row-by-row kernels recompute the batch.  Its two call sites are :1179 (the time-parallel
    log-likelihood gradient, forced by timepar_grad = 1; the recomputation is c2_internal_loglik_grad_replay,
    c2_loglik.hip:1778: k_loglik_fwd + k_loglik_rev on checkpoints) and :1787 (run_factor_rev, which factor_rev takes from
    dropin_long_rows rows -- lowered to 128 here -- on d, W, S of factor(workspace=True) under factor_iter = 1; the
    recomputation is c2_internal_factor_rev_replay, c2_loglik.hip:1663).  The Newton factor itself has no such gate: its
    d, W, S are the same bits under every limit.  For both sites: the limit at 2 kappa leaves the bits of the run without a
    limit; at kappa / 2 the result meets the oracle, differs from the time-parallel one in at least one bit (the gate
    opened), and equals bit for bit what the same kernels give when the time-parallel form is switched off
    (timepar_grad = 0, with loglik_back = 0 for the log-likelihood: c2_loglik.hip:1826 then launches that replay pair
    without a gate)."""
    cfg = SWITCH_CASES["timepar_cond_limit"]
    B, N = cfg["B"], cfg["N"]
    rng = np.random.default_rng(6000 + J)
    t, c, a, U, V, y = P.problem(rng, B, N, J)
    llo, go, flago = oracle.loglik_grad_batched(t, c, a, U, V, y, nthreads=2)
    llx, gx, flagx = oracle.loglik_grad_batched_ld(t, c, a, U, V, y, nthreads=2)
    assert not np.asarray(flago).any() and not np.asarray(flagx).any()
    # (the draw is well-conditioned: the float64 oracle stands 1e-13 or closer to its extended-precision evaluation, so
    # the plain rule applies, as issue section 5 asks to check on the CPU)
    for e, x in zip(go, gx):
        assert np.abs(e - x).max() <= 1e-13 * np.abs(e).max()
    args = dev(t, c, a, U, V, y)
    kappa = _max_finite(ops.condition(*args[:5])[0])
    assert kappa > 1.0

    def grad(opts):
        with forced(opts):
            ll, grads, flag = ops.loglik_grad(*args)
        assert int(flag.abs().sum()) == 0
        close(ll, llo)
        for g, e in zip(grads, go):
            close(g, e)
        return (ll,) + tuple(grads)

    free = grad({"timepar_grad": 1})
    loose = grad({"timepar_grad": 1, "timepar_cond_limit": 2.0 * kappa})
    tight = grad({"timepar_grad": 1, "timepar_cond_limit": 0.5 * kappa})
    rows = grad({"timepar_grad": 0, "loglik_back": 0})
    assert _bits_equal(free, loose)
    assert not _bits_equal(free, tight)
    assert _bits_equal(tight, rows)

    # factor with S by the Newton iterations (no gate of this kind), then factor_rev through run_factor_rev
    case = P.factor_case(oracle, B, N, J)
    fargs = dev(case.t, case.c, case.a, case.U, case.V)
    kappa = _max_finite(ops.condition(*fargs)[0])
    bd = rng.standard_normal((B, N)); bW = rng.standard_normal((B, N, J))
    want = [np.empty((B, N)), np.empty((B, J)), np.empty((B, N)), np.empty((B, N, J)), np.empty((B, N, J))]
    for b in range(B):
        oracle.factor_rev(case.t[b], case.c[b], case.a[b], case.U[b], case.V[b], case.d[b], case.W[b], case.S[b], bd[b],
                          bW[b], *[w[b] for w in want])
    bdd, bWd = dev(bd, bW)

    def factor_and_rev(opts):
        with forced(dict(opts, dropin_long_rows=128)):
            d, W, S, flag = ops.factor(*fargs, workspace=True)
            P.check_factor(case, d, W, S, flag)
            res = ops.factor_rev(*fargs, d, W, S, bdd, bWd)
        for r, w in zip(res, want):
            for b in range(B):
                close(r[b], w[b])
        return (d, W, S), res

    f_free, r_free = factor_and_rev({"factor_iter": 1, "timepar_grad": 1})
    f_loose, r_loose = factor_and_rev({"factor_iter": 1, "timepar_grad": 1, "timepar_cond_limit": 2.0 * kappa})
    f_tight, r_tight = factor_and_rev({"factor_iter": 1, "timepar_grad": 1, "timepar_cond_limit": 0.5 * kappa})
    assert _bits_equal(f_free, f_loose) and _bits_equal(f_free, f_tight)
    assert _bits_equal(r_free, r_loose)
    assert not _bits_equal(r_free, r_tight)
    with forced({"timepar_grad": 0}):   # factor_rev row by row on the same d, W, S
        r_rows = ops.factor_rev(*fargs, *f_tight, bdd, bWd)
    assert _bits_equal(r_tight, r_rows)
