# -*- coding: utf-8 -*-
"""Non-finite inputs on the device: one series of a batch carries a NaN or an infinity in a value input (never in t, c or a
query grid).  Per series the behaviour is the reference's (include/celerite2_amd.h, "Non-finite values"); the reference is
the float64 oracle run on the same poisoned draw (tests/test_nonfinite_oracle.py pins what it does).  Criteria, for every
case (tests/nonfinite_cases.py spells them out):
  (a) the device flags equal the oracle's, for every series;
  (b) no silent numbers: where the oracle's element is non-finite, so is the device's;
  (c) causality -- factor (d, W, S) and the four sweeps (Z, F): rows before the poison (lower forms, factor), after it
      (upper forms) and every other right-hand side are finite and within 1e-10 |x_o| + 1e-12 max(1, max |x_o|);
  (d) neighbours: every other series meets that criterion and is bit-identical to ONE clean twin -- the same options, or
      the fallback nonfinite_cases names for the path, the entry point and the class of the poison;
  (e) a failed series (a_ninf) has ll = -inf and all six gradients NaN.
Every case poisons one series at a time at batch positions 0, mid-wavefront and B - 1, at the rows of its shape class.
The test ids name the forced path and the poison kind."""
from types import SimpleNamespace

import numpy as np
import pytest

import nonfinite_cases as NF
import parity_cases as P
from parity_cases import dev, forced

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


_cache = {}


def cached(key, make):
    """Clean draws and their twins' device results: computed once, shared by the cases of a path, never written to."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def positions(shape):
    return [(b, n) for b in shape["series"] for n in shape["rows"]]


def twin_options(opts, twin):
    """(sweeps, reverse passes) the same options, and the ONE named fallback where the table gives one."""
    return [dict(opts)] + ([] if twin == "same" else [dict(opts, **f) for f in twin])


def expected_twin_options(opts, spec):
    """The one option set whose clean-twin bits the healthy series must carry: `spec` is "same" or the forced fallback."""
    return dict(opts) if spec == "same" else dict(opts, **spec)


class Checks:
    """Runs every check of a case and fails at the end with all that failed (the first twenty in the message): one run
    then shows the whole picture of a path instead of its first miss.  Nothing is tolerated: any failure fails the test."""

    def __init__(self):
        self.failed = []

    def __call__(self, check, *args, **kw):
        try:
            check(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e).splitlines()[0][:400])

    def done(self):
        assert not self.failed, "%d check(s) failed:\n  %s" % (len(self.failed), "\n  ".join(self.failed[:20]))


def assert_flags(flag, want, what):
    assert flag.cpu().tolist() == want.tolist(), "%s: flags %s, the oracle's %s" % (
        what, np.flatnonzero(flag.cpu().numpy()).tolist(), np.flatnonzero(want).tolist())


def assert_failed_series(ll, grad, b, what):
    assert np.isneginf(float(ll[b])) and np.isneginf(float(grad[0][b])), what + ": ll of a failed series is not -inf"
    assert all(bool(g[b].isnan().all()) for g in grad[1:-1]), what + ": a gradient of a failed series is not all NaN"


def assert_twin(got, twins, keep, what):
    """(d), second half: the outputs `got` (device tensors) on the series `keep` carry the bits of ONE of the twins."""
    miss = [[i for i, (g, w) in enumerate(zip(got, tw)) if not NF.same_bits(g, w, keep)] for tw in twins]
    assert not all(miss), "%s: the healthy series differ in bits from the clean twin; outputs that differ, per candidate " \
                          "option set: %s" % (what, miss)


# ---- loglik, loglik_grad ---------------------------------------------------------------------------------------------------

def _loglik_run(ops, case):
    args = dev(case.t, case.c, case.a, case.U, case.V, case.y)
    ll, flag = ops.loglik(*args)
    ll2, grads, flag2 = ops.loglik_grad(*args)
    return (ll, flag), (ll2,) + tuple(grads) + (flag2,)


def _loglik_twin(ops, path, clean, o):
    def make():
        with forced(o):
            return _loglik_run(ops, clean)
    return cached(("loglik-twin", path, tuple(sorted(o.items()))), make)


def _loglik_case(ops, oracle, path, kind, grad_too):
    shape, J, opts, twin, _, _ = NF.LOGLIK_PATHS[path]
    B = shape["B"]
    op = "loglik_grad" if grad_too else "loglik"
    clean = cached(("loglik", path), lambda: NF.as_case(P.problem(None, shape["B"], shape["N"], J)))
    chk = Checks()
    for b, n in positions(shape):
        what = "%s %s series %d row %d" % (path, kind, b, n)
        bad = NF.poison(clean, kind, b, n, col=J // 2)
        want = NF.expect(oracle, bad, "loglik_grad")
        with forced(opts):
            fwd, grad = _loglik_run(ops, bad)
        keep = NF.others(B, b)
        assert not want.flag[keep].any() and not any(want.nonfinite[k][keep].any() for k in want.values)
        ll, flag = (grad[0], grad[-1]) if grad_too else fwd
        chk(assert_flags, flag, want.flag, what)                                                               # (a)
        chk(NF.no_silent_numbers, ll, want.values["ll"], what=what + " ll")                                    # (b)
        chk(NF.close_where, ll, want.values["ll"], keep, what=what + " ll")                                    # (d)
        if grad_too:
            for g, name in zip(grad[1:-1], NF.GRAD_NAMES):
                chk(NF.no_silent_numbers, g, want.values[name], what=what + " " + name)                        # (b)
                chk(NF.close_where, g, want.values[name], keep.reshape((B,) + (1,) * (g.dim() - 1)), what=what + " " + name)   # (d)
        if want.flag[b]:                                                                                       # (e)
            assert kind == "a_ninf"
            chk(assert_failed_series, fwd[0], grad, b, what)
        # (d): the class of the poison decides which ONE twin is owed (nonfinite_cases: "y", "matrix", "unseen")
        cls = "y" if kind.startswith("y_") else ("unseen" if (kind == "V_nan" and n == shape["N"] - 1) else "matrix")
        spec = "same" if (twin == "same" or cls == "unseen") else twin[op][cls]
        tw = _loglik_twin(ops, path, clean, expected_twin_options(opts, spec))
        if grad_too:
            chk(assert_twin, grad[:-1], [tw[1][:-1]], keep, what + " (" + cls + ")")
        else:
            chk(assert_twin, fwd[:1], [tw[0][:1]], keep, what + " (" + cls + ")")
    chk.done()


@pytest.mark.parametrize("kind", NF.LOGLIK_KINDS)
@pytest.mark.parametrize("path", list(NF.LOGLIK_PATHS))
def test_loglik(ops, oracle, path, kind):
    """The forward log-likelihood."""
    _loglik_case(ops, oracle, path, kind, False)


@pytest.mark.parametrize("kind", NF.LOGLIK_KINDS)
@pytest.mark.parametrize("path", list(NF.LOGLIK_PATHS))
def test_loglik_grad(ops, oracle, path, kind):
    """The log-likelihood with its six gradients (V_nan at the last row: the oracle's ll is finite and all its gradients NaN,
    0 x NaN in reverse.hpp:65 -- nonfinite_cases.ZERO_TIMES_NAN)."""
    _loglik_case(ops, oracle, path, kind, True)


# ---- factor ----------------------------------------------------------------------------------------------------------------

def _factor_run(ops, case, with_S):
    res = ops.factor(*dev(case.t, case.c, case.a, case.U, case.V), workspace=with_S)
    return tuple(res[:-1]), res[-1]


def _factor_twin(ops, path, clean, with_S, o):
    def make():
        with forced(o):
            return _factor_run(ops, clean, with_S)[0]
    return cached(("factor-twin", path, with_S, tuple(sorted(o.items()))), make)


@pytest.mark.parametrize("with_S", [False, True], ids=["dW", "dWS"])
@pytest.mark.parametrize("kind", NF.MATRIX_KINDS)
@pytest.mark.parametrize("path", list(NF.FACTOR_PATHS))
def test_factor(ops, oracle, path, kind, with_S):
    shape, J, opts, twin, _, _ = NF.FACTOR_PATHS[path]
    B, N = shape["B"], shape["N"]
    clean = cached(("factor", path), lambda: NF.as_case(P.problem(None, shape["B"], shape["N"], J)))
    chk = Checks()
    for b, n in positions(shape):
        what = "%s %s series %d row %d" % (path, kind, b, n)
        bad = NF.poison(clean, kind, b, n, col=J // 2)
        want = NF.expect(oracle, bad, "factor")
        with forced(opts):
            outs, flag = _factor_run(ops, bad, with_S)
        chk(assert_flags, flag, want.flag, what)                                                               # (a)
        keep = NF.others(B, b)
        before = NF.rows_mask(B, N, b, n if kind != "series_nan" else 0, "before")
        for x, name in zip(outs, ("d", "W", "S")):
            tail = (1,) * (x.dim() - 2)
            chk(NF.no_silent_numbers, x, want.values[name], where=want.written[name].reshape((B, N) + tail), what=what + " " + name)   # (b)
            chk(NF.close_where, x, want.values[name], before.reshape((B, N) + tail), what=what + " (c) " + name)    # (c)
            chk(NF.close_where, x, want.values[name], keep.reshape((B, 1) + tail), what=what + " (d) " + name)      # (d)
        seen = not (kind == "V_nan" and n == N - 1)      # (no formulation reads V of the last row for d: nonfinite_cases "unseen")
        spec = "same" if (twin == "same" or not seen) else twin["dWS" if with_S else "dW"]
        chk(assert_twin, outs, [_factor_twin(ops, path, clean, with_S, expected_twin_options(opts, spec))], keep, what)   # (d)
    chk.done()


# ---- factor_rev with a poisoned cotangent ----------------------------------------------------------------------------------

def _factor_rev_clean(ops, oracle, path):
    shape, J, opts, twin = NF.FACTOR_REV_PATHS[path]
    B, N = shape["B"], shape["N"]
    case = P.factor_case(oracle, B, N, J)
    rng = np.random.default_rng(7100 + J)
    case.bd = rng.standard_normal((B, N)); case.bW = rng.standard_normal((B, N, J))
    fixed = dev(case.t, case.c, case.a, case.U, case.V, case.d, case.W, case.S)
    twins = []
    for o in twin_options(opts, twin):
        with forced(o):
            twins.append(ops.factor_rev(*fixed, *dev(case.bd, case.bW)))
    return case, fixed, twins


@pytest.mark.parametrize("kind", ["bd_nan", "bW_nan"])
@pytest.mark.parametrize("path", list(NF.FACTOR_REV_PATHS))
def test_factor_rev(ops, oracle, path, kind):
    shape, J, opts, twin = NF.FACTOR_REV_PATHS[path]
    B = shape["B"]
    case, fixed, twins = cached(("factor_rev", path), lambda: _factor_rev_clean(ops, oracle, path))
    chk = Checks()
    for b, n in positions(shape):
        what = "%s %s series %d row %d" % (path, kind, b, n)
        bd, bW = case.bd.copy(), case.bW.copy()
        if kind == "bd_nan":
            bd[b, n] = NF.NAN
        else:
            bW[b, n, J // 2] = NF.NAN
        want = NF.expect(oracle, case, "factor_rev", extra=(case.d, case.W, case.S, bd, bW))
        with forced(opts):
            got = ops.factor_rev(*fixed, *dev(bd, bW))
        keep = NF.others(B, b)
        assert any(want.nonfinite[k][b].any() for k in NF.FACTOR_REV_NAMES)
        for g, name in zip(got, NF.FACTOR_REV_NAMES):
            chk(NF.no_silent_numbers, g, want.values[name], what=what + " " + name)                                 # (b)
            chk(NF.close_where, g, want.values[name], keep.reshape((B,) + (1,) * (g.dim() - 1)), what=what + " " + name)   # (d)
        chk(assert_twin, got, twins, keep, what)
    chk.done()


# ---- the four sweeps -------------------------------------------------------------------------------------------------------

def _sweep_names(which):
    return [s for s in P.SWEEPS if which == "all" or s.startswith(which)]


def _sweep_run(ops, case, name, with_F):
    td, cd, Ud, Sd, Yd = P.sweep_inputs(case, name)
    kw = dict(zero_z=True) if name.startswith("matmul") else {}
    res = getattr(ops, name)(td, cd, Ud, Sd, Yd, workspace=with_F, **kw)
    return tuple(res) if with_F else (res,)


def _sweep_clean(ops, oracle, path):
    shape, J, nrhs, opts, with_F, which, twin = NF.SWEEP_PATHS[path]
    case = P.sweep_case(oracle, 7200 + 10 * J + nrhs, shape["B"], shape["N"], J, nrhs)
    twins = {}
    for name in _sweep_names(which):
        twins[name] = []
        for o in twin_options(opts, twin):
            with forced(o):
                twins[name].append(_sweep_run(ops, case, name, with_F))
    return case, twins


@pytest.mark.parametrize("kind", NF.SWEEP_KINDS)
@pytest.mark.parametrize("path", list(NF.SWEEP_PATHS))
def test_sweeps(ops, oracle, path, kind):
    shape, J, nrhs, opts, with_F, which, twin = NF.SWEEP_PATHS[path]
    B, N = shape["B"], shape["N"]
    case, twins = cached(("sweep", path), lambda: _sweep_clean(ops, oracle, path))
    col = (nrhs // 2) if kind == "Y_nan_col" else J // 2
    keep = None
    chk = Checks()
    for b, n in positions(shape):
        bad = NF.poison(case, kind, b, n, col=col)
        keep = NF.others(B, b)
        for name in _sweep_names(which):
            what = "%s %s %s series %d row %d" % (path, name, kind, b, n)
            want = NF.expect(oracle, bad, "sweep", name)
            with forced(opts):
                got = _sweep_run(ops, bad, name, with_F)
            side = NF.rows_mask(B, N, b, n, "before" if name.endswith("lower") else "after")
            outs = [(got[0], want.values["Z"], "Z")]
            if with_F:
                outs.append((NF.F_by_rhs(NF.host(got[1])), NF.F_by_rhs(want.values["F"]), "F"))
            for x, w, tag in outs:
                tail = (1,) * (w.ndim - 2)
                chk(NF.no_silent_numbers, x, w, what=what + " " + tag)                                              # (b)
                chk(NF.close_where, x, w, side.reshape((B, N) + tail), what=what + " (c) rows " + tag)              # (c)
                if kind == "Y_nan_col":                                                                        # (c): other columns
                    cols = np.zeros(w.shape, bool); cols[b] = True; cols[b, :, col] = False
                    chk(NF.close_where, x, w, cols, what=what + " (c) columns " + tag)
                chk(NF.close_where, x, w, keep.reshape((B, 1) + tail), what=what + " (d) " + tag)                   # (d)
            chk(assert_twin, got, twins[name], keep, what)                                                          # (d)
    chk.done()


def _sweep_rev_clean(ops, oracle, path):
    shape, J, nrhs, opts, twin = NF.SWEEP_REV_PATHS[path]
    case = P.sweep_case(oracle, 7300 + 10 * J + nrhs, shape["B"], shape["N"], J, nrhs)
    twins = {}
    for name in P.SWEEPS:
        td, cd, Ud, Sd, Yd = P.sweep_inputs(case, name)
        Zd, Fd, bZd = dev(case.want[name].Z, case.want[name].F, case.bZ)
        twins[name] = []
        for o in twin_options(opts, twin):
            with forced(o):
                twins[name].append(getattr(ops, name + "_rev")(td, cd, Ud, Sd, Yd, Zd, Fd, bZd))
    return case, twins


@pytest.mark.parametrize("kind", NF.SWEEP_REV_KINDS)
@pytest.mark.parametrize("path", list(NF.SWEEP_REV_PATHS))
def test_sweeps_rev(ops, oracle, path, kind):
    """The reverse passes on Z and F of the oracle's forward sweep of the SAME poisoned input (they then carry the NaN the
    reference's forward pass would have handed its reverse pass)."""
    shape, J, nrhs, opts, twin = NF.SWEEP_REV_PATHS[path]
    B = shape["B"]
    case, twins = cached(("sweep_rev", path), lambda: _sweep_rev_clean(ops, oracle, path))
    col = J // 2 if kind == "U_nan" else nrhs // 2
    chk = Checks()
    for b, n in positions(shape):
        bad = NF.poison(case, kind, b, n, col=col)
        keep = NF.others(B, b)
        for name in P.SWEEPS:
            what = "%s %s_rev %s series %d row %d" % (path, name, kind, b, n)
            want = NF.expect(oracle, bad, "sweep_rev", name)
            td, cd, Ud, Sd, Yd = P.sweep_inputs(bad, name)
            Zd, Fd, bZd = dev(want.Z, want.F, bad.bZ)
            with forced(opts):
                got = getattr(ops, name + "_rev")(td, cd, Ud, Sd, Yd, Zd, Fd, bZd)
            for g, k in zip(got, NF.REV_NAMES):
                chk(NF.no_silent_numbers, g, want.values[k], what=what + " " + k)                                   # (b)
                chk(NF.close_where, g, want.values[k], keep.reshape((B,) + (1,) * (g.dim() - 1)), what=what + " " + k)   # (d)
            if kind == "bZ_nan" and nrhs > 1:                                                                  # (c): other columns of bY
                cols = np.zeros(want.values["bY"].shape, bool); cols[b] = True; cols[b, :, col] = False
                chk(NF.close_where, got[4], want.values["bY"], cols, what=what + " (c) columns bY")
            chk(assert_twin, got, twins[name], keep, what)                                                          # (d)
    chk.done()


# ---- dot_tril --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["Y_nan_col", "U_nan", "d_nan"])
@pytest.mark.parametrize("J,nrhs", [(8, 1), (5, 3), (8, 8)])
def test_dot_tril(ops, oracle, J, nrhs, kind):
    """Z = L sqrt(D) Y, a lower form: rows before the poison and the other right-hand sides under (c), neighbours under (d)
    as bit-identity with the clean run (no fallback: c2_ops.hip k_dot_tril / the product sweeps carry arithmetic only)."""
    shape = NF.ROWS
    B, N = shape["B"], shape["N"]
    case = cached(("dot_tril", J, nrhs), lambda: P.sweep_case(oracle, 7400 + 10 * J + nrhs, B, N, J, nrhs))
    base = SimpleNamespace(B=B, t=case.t, c=case.c, U=case.U, W=case.W, Y=case.Y, d=np.exp(0.1 * case.Z0[:, :, 0]))
    clean = cached(("dot_tril-clean", J, nrhs), lambda: ops.dot_tril(*dev(base.t, base.c, base.U, base.W, base.d, base.Y)))
    col = nrhs // 2
    chk = Checks()
    for b, n in positions(shape):
        what = "dot_tril J %d nrhs %d %s series %d row %d" % (J, nrhs, kind, b, n)
        bad = SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(base).items()})
        if kind == "Y_nan_col":
            bad.Y[b, n, col] = NF.NAN
        elif kind == "U_nan":
            bad.U[b, n, J // 2] = NF.NAN
        else:
            bad.d[b, n] = NF.NAN
        want = NF.dot_tril_reference(oracle, bad)
        got = ops.dot_tril(*dev(bad.t, bad.c, bad.U, bad.W, bad.d, bad.Y))
        keep = NF.others(B, b)
        chk(NF.no_silent_numbers, got, want, what=what)                                                        # (b)
        chk(NF.close_where, got, want, NF.rows_mask(B, N, b, n, "before").reshape(B, N, 1), what=what + " (c) rows")   # (c)
        if kind != "U_nan":
            cols = np.zeros(want.shape, bool); cols[b] = True; cols[b, :, col] = False
            if kind == "d_nan":
                cols[b, n:] = False          # (d_n scales every right-hand side of row n, which feeds the rows behind it)
            chk(NF.close_where, got, want, cols, what=what + " (c) columns")
        chk(NF.close_where, got, want, keep.reshape(B, 1, 1), what=what + " (d)")                              # (d)
        chk(assert_twin, [got], [[clean]], keep, what)
    chk.done()


# ---- the ops that consume a factor -----------------------------------------------------------------------------------------

def _consumer_params():
    return [(op, kind) for op, (kinds, _) in NF.CONSUMERS.items() for kind in kinds]


@pytest.mark.parametrize("J", [3, 8, 32])
@pytest.mark.parametrize("op,kind", _consumer_params())
def test_factor_consumers(ops, oracle, op, kind, J):
    """inverse_diag, explained_variance, whitened_gram / sinusoids / transits / keplerians, trial_projections on B = 9 series
    of 33 rows with one series' d row, W entry or Z0 / z / alpha entry NaN: (b) against the numpy restatement of the op on
    the same poisoned arrays, (d) as bit-identity with the clean run (these ops have no fallback), neighbours finite."""
    shape = NF.CONSUMER_SHAPE
    B = shape["B"]
    case = cached(("consumer", J), lambda: NF.consumer_case(oracle, J))
    clean = cached(("consumer-clean", J, op), lambda: NF.consumer_device(ops, op, case))
    chk = Checks()
    for b, n in positions(shape):
        what = "%s J %d %s series %d row %d" % (op, J, kind, b, n)
        bad = NF.consumer_poison(case, kind, b, n)
        want = NF.consumer_reference(op, bad)
        got = NF.consumer_device(ops, op, bad)
        keep = NF.others(B, b)
        if not (kind == "W_nan" and n == shape["N"] - 1):    # (a lower sweep never reads the last row of W: nothing to propagate)
            assert any((~np.isfinite(w[b])).any() for w in want), what + ": the poison does not reach the restatement"
        for i, (g, w) in enumerate(zip(got, want)):
            assert tuple(g.shape) == w.shape
            chk(NF.no_silent_numbers, g, w, what="%s output %d" % (what, i))                                   # (b)
            assert np.isfinite(w[keep]).all()
            chk(NF.close_where, g, w, keep.reshape((B,) + (1,) * (w.ndim - 1)), what="%s output %d (d)" % (what, i),
                tol=1e-9, floor=1e-11)       # (the restatements' own distance from the device: tests/test_gpu_periodogram.py)
        chk(assert_twin, got, [clean], keep, what)                                                             # (d)
    chk.done()


# ---- loglik_terms_grad on the fused mappings -------------------------------------------------------------------------------

TERMS_MAPPINGS = {   # the switches of tests/test_gpu_terms.py::test_fuzz_fused_terms_kernels (force)
    "fused":      {"terms_fused": 1, "terms_two_lanes": 0, "terms_eight_lanes": 0, "terms_four_lanes": 0},
    "two_lanes":  {"terms_fused": 0, "terms_two_lanes": 1, "terms_eight_lanes": 0, "terms_four_lanes": 0},
    "four_lanes": {"terms_fused": 0, "terms_two_lanes": 0, "terms_eight_lanes": 0, "terms_four_lanes": 1},
    "eight_lanes": {"terms_fused": 0, "terms_two_lanes": 0, "terms_eight_lanes": 1, "terms_four_lanes": 0},
}
TERMS_COMPOSED = {"terms_fused": 0, "terms_two_lanes": 0, "terms_eight_lanes": 0, "terms_four_lanes": 0}
TERMS_NAMES = ("bar", "bcr", "bac", "bbc", "bcc", "bdc", "bx", "bdiag", "by")


def _terms_case():
    rng = np.random.default_rng(7500)
    B, N, Jr, Jc = NF.ROWS["B"], NF.ROWS["N"], 2, 3
    ar = rng.uniform(0.5, 1.5, (B, Jr)); cr = rng.uniform(0.05, 0.5, (B, Jr))
    ac = rng.uniform(0.5, 2.0, (B, Jc)); cc = rng.uniform(0.02, 0.3, (B, Jc)); dc = rng.uniform(0.2, 3.0, (B, Jc))
    bc = ac * cc / dc * rng.uniform(0.0, 0.9, (B, Jc))
    x = np.sort(rng.uniform(0, N / 10.0, (B, N)), axis=1)
    diag = rng.uniform(0.1, 0.3, (B, N))
    y = np.sin(x) + 0.1 * rng.standard_normal((B, N))
    return dict(ar=ar, cr=cr, ac=ac, bc=bc, cc=cc, dc=dc, x=x, diag=diag, y=y)


def _terms_run(ops, opts, case):
    with forced(opts):
        ll, grads, flag = ops.loglik_terms_grad(*dev(*[case[k] for k in ("ar", "cr", "ac", "bc", "cc", "dc", "x", "diag", "y")]))
    return (ll,) + tuple(grads), flag


@pytest.mark.parametrize("kind", ["ar_nan", "y_nan", "y_inf", "diag_nan"])
@pytest.mark.parametrize("mapping", list(TERMS_MAPPINGS))
def test_loglik_terms_grad(ops, mapping, kind):
    """The coefficient-level pair on each fused mapping against the composed chain on the SAME poisoned input: flags equal,
    (b), and (d) -- the neighbours within the distance tests/test_gpu_terms.py holds the fused kernels to the composed chain
    (1e-9, floor 1e-11) and bit-identical to the clean twin of the mapping or, where a group of 64 series is handed to the
    composed chain (c2_loglik.hip:282, the per-group gate words), to the composed clean twin."""
    shape = NF.ROWS
    B = shape["B"]
    clean = cached("terms-case", _terms_case)
    opts = TERMS_MAPPINGS[mapping]
    twins = cached(("terms-twins", mapping), lambda: [_terms_run(ops, opts, clean)[0], _terms_run(ops, TERMS_COMPOSED, clean)[0]])
    chk = Checks()
    for b, n in positions(shape):
        what = "loglik_terms_grad %s %s series %d row %d" % (mapping, kind, b, n)
        bad = {k: v.copy() for k, v in clean.items()}
        if kind == "ar_nan":
            bad["ar"][b, 0] = NF.NAN
        elif kind == "diag_nan":
            bad["diag"][b, n] = NF.NAN
        else:
            bad["y"][b, n] = NF.NAN if kind == "y_nan" else NF.INF
        want, wflag = _terms_run(ops, TERMS_COMPOSED, bad)
        got, flag = _terms_run(ops, opts, bad)
        keep = NF.others(B, b)
        chk(assert_flags, flag, wflag.cpu().numpy(), what)                                                     # (a)
        for g, w, name in zip(got, want, ("ll",) + TERMS_NAMES):
            w = w.cpu().numpy()
            chk(NF.no_silent_numbers, g, w, what=what + " " + name)                                            # (b)
            chk(NF.close_where, g, w, keep.reshape((B,) + (1,) * (w.ndim - 1)), what=what + " " + name, tol=1e-9, floor=1e-11)
        chk(assert_twin, got, twins, keep, what)                                                               # (d)
    chk.done()


# ---- the front end ---------------------------------------------------------------------------------------------------------

def test_gaussian_process_with_a_nan_hyperparameter(ops):
    """GaussianProcess over B = 9 series with a per-series S0 that is NaN in one of them: compute(quiet=True), log_likelihood,
    log_likelihood_kernel(...).backward().  That series' value is NaN or -inf; every other series' value and per-series
    gradient are those of the clean twin; the gradient of a parameter SHARED by the batch is a sum over the series that
    contains a NaN, hence NaN -- as it would be in the reference."""
    import torch
    from celerite2_amd import gp as G, terms as T
    B, N, bad_b = 9, 33, 4
    rng = np.random.default_rng(7600)
    t = np.sort(rng.uniform(0, N / 10.0, (B, N)), axis=1)
    diag = rng.uniform(0.1, 0.3, (B, N))
    y = np.sin(t) + 0.1 * rng.standard_normal((B, N))
    S0 = rng.uniform(0.8, 1.6, B); w0 = rng.uniform(0.7, 1.2, B)
    td, dd, yd = dev(t, diag, y)

    def run(S0v):
        S0t, w0t = [x.requires_grad_() for x in dev(S0v, w0)]
        Qt = torch.tensor(2.5, dtype=torch.float64, device="cuda", requires_grad=True)      # shared by the batch
        gp = G.GaussianProcess(T.SHOTerm(S0=S0t, w0=w0t, Q=Qt, regime="under"), mean=0.0)
        with torch.no_grad():
            gp.compute(td, diag=dd, quiet=True)
            ll = gp.log_likelihood(yd)
        llk = gp.log_likelihood_kernel(yd)
        llk.sum().backward()
        return ll, llk.detach(), S0t.grad, w0t.grad, Qt.grad

    clean = run(S0)
    S0bad = S0.copy(); S0bad[bad_b] = NF.NAN
    got = run(S0bad)
    keep = NF.others(B, bad_b)
    for v in got[:4]:
        assert not bool(torch.isfinite(v[bad_b])), "the poisoned series returned a finite number"
    for g, w, name in zip(got[:4], clean[:4], ("log_likelihood", "log_likelihood_kernel", "dS0", "dw0")):
        NF.close_where(g, w.cpu().numpy(), keep, what=name)
    assert bool(torch.isfinite(clean[4])) and bool(torch.isnan(got[4])), "the gradient of the shared Q sums a NaN: it must be NaN"
