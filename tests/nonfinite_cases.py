# -*- coding: utf-8 -*-
"""Non-finite inputs (plain helpers, no tests): poisons of a parity_cases draw, the float64 oracle's answer to them, the
comparison rules of test_gpu_nonfinite.py and the table of what each forced path owes the healthy series of a batch.

The rule under test (include/celerite2_amd.h, "Non-finite values"): per series the behaviour is the reference's -- the pivot
test is `d <= 0`, which a NaN passes, so a NaN or an infinity in a, U, V, y, a right-hand side or a cotangent raises no
flag and propagates as IEEE arithmetic propagates it; nothing is sanitised; no other series is affected.  Poisons touch
VALUES only: never t, c, query times or trial grids, which steer merges, binary searches and gates.

Criteria (the letters are those of test_gpu_nonfinite.py):
  (a) the device flags equal the oracle's, for every series;
  (b) where the oracle's output element is non-finite, the device's is non-finite;
  (c) causality: rows strictly before the poison row (factor, lower sweeps), strictly after it (upper sweeps) and every
      other right-hand-side column are finite and meet `close_where` against the oracle;
  (d) every other series meets `close_where` against the oracle and is bit-identical to the clean twin (the same batch
      with the poisoned series healed) under the options PATHS names for the path;
  (e) a series that fails (flag != 0: a_ninf) has ll = -inf and all six gradients NaN.
A device NaN where the oracle is finite is tolerated only outside the regions of (c) and (d).
"""
import copy
from types import SimpleNamespace

import numpy as np

import parity_cases as P

NAN, INF = float("nan"), float("inf")

# poison kinds by what they touch
MATRIX_KINDS = ("a_nan", "a_pinf", "a_ninf", "U_nan", "V_nan", "series_nan")      # inputs of factor
LOGLIK_KINDS = ("y_nan", "y_inf") + MATRIX_KINDS                                  # inputs of loglik / loglik_grad
SWEEP_KINDS = ("Y_nan_col", "U_nan")                                              # inputs of the forward sweeps
SWEEP_REV_KINDS = ("Y_nan_col", "bZ_nan", "U_nan")                                # ... and of their reverse passes
ALL_KINDS = ("y_nan", "y_inf", "a_nan", "a_pinf", "a_ninf", "U_nan", "V_nan", "series_nan", "Y_nan_col", "bZ_nan")


def as_case(x):
    """A problem() tuple as a namespace with the fields of the other draws (B, N, J, t, c, a, U, V, y)."""
    if isinstance(x, SimpleNamespace):
        return x
    t, c, a, U, V, y = x
    return SimpleNamespace(B=y.shape[0], N=y.shape[1], J=c.shape[-1], t=t, c=c, a=a, U=U, V=V, y=y)


def poison(case, kind, series, row, col=0):
    """A copy of a parity_cases.problem tuple / factor_case / loglik_case / sweep_case draw with one poison in `series` at
    `row` (`col`: the column of U / V, the right-hand side of Y / bZ).  Every array is copied; oracle results the draw
    carried (`want`, d, W, S, ll, grads) are dropped -- expect() recomputes them.  t and c are never touched."""
    src = as_case(case)
    drop = ("want", "d", "S", "flag", "ok", "ll", "grads") + (("W",) if hasattr(src, "d") else ())   # (factor_case: W is a result)
    out = SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else copy.copy(v)) for k, v in vars(src).items()
                             if k not in drop})
    b, n = series, row
    if kind == "y_nan":
        out.y[b, n] = NAN
    elif kind == "y_inf":
        out.y[b, n] = INF
    elif kind == "a_nan":
        out.a[b, n] = NAN
    elif kind == "a_pinf":
        out.a[b, n] = INF
    elif kind == "a_ninf":
        out.a[b, n] = -INF
    elif kind == "U_nan":
        out.U[b, n, col] = NAN
    elif kind == "V_nan":
        out.V[b, n, col] = NAN
    elif kind == "series_nan":
        out.a[b] = NAN; out.U[b] = NAN; out.V[b] = NAN
    elif kind == "Y_nan_col":
        out.Y[b, n, col] = NAN
    elif kind == "bZ_nan":
        out.bZ[b, n, col] = NAN
    else:
        raise ValueError("unknown poison kind %r" % (kind,))
    out.poison = SimpleNamespace(kind=kind, series=b, row=n, col=col)
    assert np.array_equal(out.t, src.t) and np.array_equal(out.c, src.c)
    return out


def _result(flag, **values):
    return SimpleNamespace(flag=None if flag is None else np.asarray(flag, dtype=np.int64), values=values,
                           nonfinite={k: ~np.isfinite(v) for k, v in values.items()})


GRAD_NAMES = ("bt", "bc", "ba", "bU", "bV", "by")
REV_NAMES = ("bt", "bc", "bU", "bW", "bY")
FACTOR_REV_NAMES = ("bt", "bc", "ba", "bU", "bV")


def expect(oracle, case, op, name=None, extra=None):
    """The float64 oracle on a (poisoned) draw: a namespace of `flag` (per series; None for ops without one), `values`
    (output name -> array, non-finite elements as the oracle produced them: read the finite ones through ~nonfinite) and
    `nonfinite` (output name -> mask).  op:
      "loglik_grad"  ll and the six gradients (a failed series: ll = -inf, gradients NaN, as the header requires)
      "factor"       d, W, S; rows the reference's early return leaves unwritten are NaN here and listed as unwritten
                     in `written` (d: rows <= flag, W: rows < flag, S: rows <= flag)
      "factor_rev"   the five outputs for extra = (d, W, S, bd, bW)
      "sweep"        Z, F of `name` (one of parity_cases.SWEEPS) on case.U / W or V / Y
      "sweep_rev"    the five reverse outputs of `name` for the cotangent case.bZ (Z, F from the oracle's forward sweep)"""
    c = as_case(case)
    B, N, J = c.B, c.N, c.J
    if op == "loglik_grad":
        ll, grads, flag = oracle.loglik_grad_batched(c.t, c.c, c.a, c.U, c.V, c.y, nthreads=2)
        grads = [g.copy() for g in grads]
        for b in np.flatnonzero(flag):     # celerite2_amd.h: "ll[b] = -inf and ALL SIX gradients filled with NaN"
            for g in grads:
                g[b] = NAN
        return _result(flag, ll=ll, **dict(zip(GRAD_NAMES, grads)))
    if op == "factor":
        d = np.full((B, N), NAN); W = np.full((B, N, J), NAN); S = np.full((B, N, J, J), NAN)
        flag = np.zeros(B, dtype=np.int64)
        wd = np.ones((B, N), bool); wW = np.ones((B, N), bool)
        for b in range(B):
            flag[b] = oracle.factor_flag(c.t[b], c.c[b], c.a[b], c.U[b], c.V[b], d[b], W[b], S[b])
            if flag[b]:
                wd[b, flag[b] + 1:] = False; wW[b, flag[b]:] = False
        res = _result(flag, d=d, W=W, S=S)
        res.written = dict(d=wd, W=wW, S=wd)
        return res
    if op == "factor_rev":
        d, W, S, bd, bW = extra
        outs = [np.empty((B, N)), np.empty((B, J)), np.empty((B, N)), np.empty((B, N, J)), np.empty((B, N, J))]
        for b in range(B):
            oracle.factor_rev(c.t[b], c.c[b], c.a[b], c.U[b], c.V[b], d[b], W[b], S[b], bd[b], bW[b], *[o[b] for o in outs])
        return _result(None, **dict(zip(FACTOR_REV_NAMES, outs)))
    sec = P.second(c, name)
    nrhs = c.Y.shape[-1]
    Z = np.empty_like(c.Y); F = np.empty((B, N, J, nrhs))
    for b in range(B):
        getattr(oracle, name + "_fwd")(c.t[b], c.c[b], c.U[b], sec[b], c.Y[b], Z[b], F[b])
    if op == "sweep":
        return _result(None, Z=Z, F=F)
    if op == "sweep_rev":
        rev = [np.empty((B, N)), np.empty((B, J)), np.empty((B, N, J)), np.empty((B, N, J)), np.empty((B, N, nrhs))]
        for b in range(B):
            getattr(oracle, name + "_rev")(c.t[b], c.c[b], c.U[b], sec[b], c.Y[b], Z[b], F[b], c.bZ[b], *[r[b] for r in rev])
        res = _result(None, **dict(zip(REV_NAMES, rev)))
        res.Z, res.F = Z, F
        return res
    raise ValueError("unknown op %r" % (op,))


# ---- comparison rules ------------------------------------------------------------------------------------------------------

def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def no_silent_numbers(got, want, where=None, what=""):
    """(b): wherever the oracle's element is non-finite (inside `where`, default everywhere), so is the device's."""
    got, want = host(got), np.asarray(want)
    bad = ~np.isfinite(want) & np.isfinite(got)
    if where is not None:
        bad &= np.broadcast_to(where, bad.shape)
    assert not bad.any(), "%s: %d finite device element(s) where the oracle is non-finite, first at %s (device %r)" % (
        what, int(bad.sum()), tuple(np.argwhere(bad)[0]), float(got[tuple(np.argwhere(bad)[0])]))


def close_where(got, want, region, what="", tol=1e-10, floor=1e-12):
    """(c), (d): on `region` (a mask that broadcasts to the output) the oracle is finite, the device is finite, and
    |x - x_o| <= tol |x_o| + floor max(1, max |x_o|), the maximum over the oracle's finite elements of the region -- the
    rule of parity_cases.close."""
    got, want = host(got), np.asarray(want)
    region = np.broadcast_to(region, want.shape)
    if not region.any():
        return
    w, g = want[region], got[region]
    assert np.isfinite(w).all(), "%s: the oracle is not finite on the protected region" % what
    bad = ~np.isfinite(g)
    assert not bad.any(), "%s: %d non-finite device element(s) on the protected region, first at %s" % (
        what, int(bad.sum()), tuple(np.argwhere(region)[np.flatnonzero(bad)[0]]))
    lim = tol * np.abs(w) + floor * max(1.0, float(np.abs(w).max()))
    err = np.abs(g - w)
    worst = int(np.argmax(err - lim))
    assert (err <= lim).all(), "%s: |x - x_o| = %.3e > %.3e at %s" % (
        what, err[worst], lim[worst], tuple(np.argwhere(region)[worst]))


def F_by_rhs(F):
    """The workspace F, declared (B, N, J, nrhs), as the reference lays it out: row n is the J x nrhs state column-major,
    i.e. (B, N, nrhs, J) in memory -- [..., k, :] is the state of right-hand side k."""
    B, N, J, K = F.shape
    return F.reshape(B, N, K, J)


def others(B, series):
    keep = np.ones(B, bool); keep[series] = False
    return keep


def rows_mask(B, N, series, row, side):
    """(B, N) mask of the poisoned series' protected rows: side "before" (rows < row) or "after" (rows > row)."""
    m = np.zeros((B, N), bool)
    if side == "before":
        m[series, :row] = True
    else:
        m[series, row + 1:] = True
    return m


def same_bits(x, y, keep):
    """Bit-identity of two device tensors on the series `keep` (NaN payloads included: the words are compared)."""
    import torch
    idx = torch.from_numpy(np.flatnonzero(keep)).to(x.device)
    xi, yi = x.index_select(0, idx).contiguous(), y.index_select(0, idx).contiguous()
    if xi.dtype == torch.float64:
        xi, yi = xi.view(torch.int64), yi.view(torch.int64)
    return bool(torch.equal(xi, yi))


# ---- the per-path table ----------------------------------------------------------------------------------------------------
# shape classes (B, N): the row-by-row kernels -- two ragged wavefronts at one lane per series, nine at eight lanes, N
# straddling the 32-row checkpoint; the time-parallel forms -- chunk edges at 64, the 1024-row switch, the last row
ROWS = dict(B=70, N=33, rows=(0, 1, 16, 31, 32), series=(0, 37, 69))
LONG = dict(B=5, N=1030, rows=(0, 63, 64, 500, 1029), series=(0, 2, 4))

# What the healthy series of a batch are owed under (d), per forced path:
#   twin = "same"      bit-identical to the clean twin under the SAME options.  Nothing on the path makes a decision for more
#                      than one series from a value input: the gates of the lane mappings compare c_j x time spans and
#                      phases dc x with their guards (values of t, c, x only, which no poison touches).
#   twin = (options, ...)  the poison may send the batch to a fallback formulation by design (a poison the verification does
#                      not see -- a NaN in y of a factor-only check -- leaves it where it was): bit-identical to the clean
#                      twin under the same options or with ONE of these option sets, each of which forces the fallback
#                      kernels on the clean batch; the rule of
#                      test_gpu_timepar.py::test_timepar_falls_back_when_it_cannot_be_trusted.
# `decides`: the line that decides it.  `loops`: the finding of the safety reading (issue: "any address, trip count or loop
# exit computed from a value input") -- none on every path below: the loops are bounded by N, J, nrhs, chunk and launch
# counts (c2_timepar.hip:1042 `while (n > 1)` halves a record count, c2_timepar_grad.hip:230 walks a lane index,
# c2_timepar_grad.hip kNewtonMax bounds the Newton launches, each gated by the previous one's word on the device; the merge
# loops c2_wide.hip:400, c2_ops.hip:806/:819 and the binary searches compare TIMES only).
# The fallbacks a poisoned batch was measured to take (which option set reproduces the healthy series bit for bit):
#   forward log-likelihood       the row-by-row kernel behind the gate c2_loglik.hip:1528 = {timepar: 0} (with factor_iter: 0
#                                where the path forces the Newton form);
#   log-likelihood + gradient    a poison of a, U, V fails the FACTOR STAGE of the time-parallel gradient, whose d, W then come
#                                from the row-by-row factor (c2_loglik.hip:1631 / :1646) while the reverse pass stays parallel
#                                along time = {factor_iter: 0} (widths 8, 5), {timepar: 0, factor_iter: 0} (widths 4, 2: scanned
#                                chunk states); a poison of y alone is seen by no verification: the same-options twin; the
#                                segment-replay pair behind k_verify_combine (c2_loglik.hip:1826) = every form off, loglik_back: 0;
#   factor                       {timepar: 0, factor_iter: 0} without S, {factor_scan8: 0} / {timepar: 0} with S (the S rows are
#                                then replayed from the row-by-row d, W).
# Per path the expected twin is keyed by the entry point and the CLASS of the poison -- ONE option set each, no alternatives:
#   "y"       y_nan, y_inf: reaches the value, no pivot;
#   "matrix"  a, U, V poisons that reach a pivot (the oracle's ll / d of the series is not finite, or it is flagged);
#   "unseen"  V of the last row, which no pivot of any formulation reads (the oracle's ll and d stay finite): always the
#             same-options twin.  (U of row 0 is NOT unseen: the row-by-row kernels and the oracle never read it, but a chunk
#             element of the time-parallel forms multiplies it by its zero start state, 0 x NaN, and the verification word
#             sends the batch to the row-by-row kernels -- measured; it counts as a matrix poison.)
# twin(y, matrix) builds the two entries; "same" = the options of the path, a dict = those options with the fallback forced.
def twin(y, matrix):
    return {"y": y, "matrix": matrix}


_T0, _F0, _T0F0 = {"timepar": 0}, {"factor_iter": 0}, {"timepar": 0, "factor_iter": 0}
LONG_TWINS = {
    # forward: one-pass form (widths 8, 4, 2) -> row-by-row kernel behind c2_loglik.hip:1528; gradient: y is seen by no
    # verification; a matrix poison fails the factor stage alone (c2_loglik.hip:1631 / :1646), the reverse stays time-parallel
    "default-long-J8":  {"loglik": twin(_T0, _T0), "loglik_grad": twin("same", _F0)},
    "timepar1-J8":      {"loglik": twin(_T0, _T0), "loglik_grad": twin("same", _F0)},
    "timepar1-J4":      {"loglik": twin(_T0, _T0), "loglik_grad": twin("same", _T0)},
    "timepar1-J2":      {"loglik": twin(_T0, _T0), "loglik_grad": twin("same", _T0)},
    "timepar_grad1-J8": {"loglik": twin(_T0F0, _T0F0), "loglik_grad": twin("same", _F0)},
    # width 5: the forward form is Newton factor + chunk-map solve; k_ll_guard (c2_loglik.hip:1395) opens the row-by-row kernel
    "timepar_grad1-J5": {"loglik": twin(_F0, _F0), "loglik_grad": twin("same", _F0)},
    "timepar_grad1-J2": {"loglik": twin(_T0F0, _T0F0), "loglik_grad": twin("same", _T0F0)},
}
# 70 x 33 at width 8 by default dispatch: only the forward pass is time-parallel (cost model), the gradient is not
DEFAULT8_TWINS = {"loglik": twin(_T0, _T0), "loglik_grad": twin("same", "same")}
# factor: keyed by whether S is asked for ("dW" / "dWS"); only matrix poisons exist
FACTOR_TWINS = {
    "default-long-J8": {"dW": _F0, "dWS": {"factor_scan8": 0}},   # c2_loglik.hip:1620 scanned states; with S the drop-in form
    "timepar1-J4":     {"dW": _T0, "dWS": _T0},
    "timepar1-J2":     {"dW": _T0, "dWS": _T0},
}

# Where 0 x NaN arises in the reference and the device had a select (criterion (b) stays strict; the kernels now multiply):
ZERO_TIMES_NAN = {
    "bV of the last row":
        "reverse.hpp:55 divides bW_{N-1} = 0 by d_{N-1}: NaN behind a NaN pivot.  The seeds were a literal 0; they are "
        "0.0 * (1 / d_{N-1}) now: c2_loglik.hip:906, c2_loglik_t.hip (behind the seeds of ba, bz), c2_loglik_k2.hip (the same), "
        "c2_loglik_q4.hip:707",
    "ba of the last row":
        "reverse.hpp:65 subtracts W_{N-1} . bV_{N-1}: a NaN in V_{N-1} alone makes W_{N-1} NaN, and 0 x NaN turns ALL six "
        "gradients NaN although ll, which never reads W_{N-1}, is finite.  The seeds of ba_{N-1} carry that product now "
        "(the recorded W_{N-1}: c2_loglik_t.hip, c2_loglik_k2.hip, c2_loglik_q4.hip:709, c2_loglik.hip:908 in the "
        "backward-recursion form; the replay form of c2_loglik.hip has not formed W_{N-1} when it seeds and takes V_{N-1}, "
        "which is not finite for the same inputs once d_{N-1} is)",
}
# A fallback that was wrong (not a 0 x NaN matter): fixed in the dispatcher
FALLBACK_FIXES = {
    "forward loglik under factor_iter = 1 (widths other than 8, 4, 2)":
        "c2_timepar_grad.hip:1936 composes c2_factor -- which falls back to the row-by-row factor on its own -- with the "
        "chunk-map solve: the healthy series carried the bits of neither twin (2.3e-13 absolute from both).  k_ll_guard "
        "(c2_loglik.hip:1395) now opens the gate of the row-by-row kernel behind a failed or non-finite series "
        "(c2_loglik.hip:1511): the fallback twin is {factor_iter: 0}",
}
_AUTO8 = ("c2_loglik.hip:1309 use_timepar takes the forward pass at width 8 by its cost model (70 x 33 included), "
          "the gate c2_loglik.hip:1528; ")
_ROWGATE = "c2_loglik_helpers.hpp:29 gate_closed: the word is max c_j x span (k_anchor_spans), no value input"
_VERIFY = "c2_timepar.hip:1961 (a failed factorisation or a NaN raises the verification word); pivots c2_timepar.hip:643, :966"
LOGLIK_PATHS = {
    # id: (shape class, width J, forced options, twin, the line that decides, loops)
    "default-J8":          (ROWS, 8, {}, DEFAULT8_TWINS, _AUTO8 + _VERIFY, "none"),
    "lanes1-J8":           (ROWS, 8, {"lanes": 1}, "same", "c2_loglik_t.hip:591; " + _ROWGATE, "none"),
    "lanes1-J6":           (ROWS, 6, {"lanes": 1}, "same", "c2_loglik_t.hip:591; " + _ROWGATE, "none"),
    "lanes1-J4":           (ROWS, 4, {"lanes": 1}, "same", "c2_loglik_t.hip:591; " + _ROWGATE, "none"),
    "lanes1-J2":           (ROWS, 2, {"lanes": 1}, "same", "c2_loglik_t.hip:591; " + _ROWGATE, "none"),
    "lanes2-J8":           (ROWS, 8, {"lanes": 2}, "same", "c2_loglik_k2.hip:449; " + _ROWGATE, "none"),
    "lanes4-J8":           (ROWS, 8, {"lanes": 4}, "same", "c2_loglik_q4.hip:422, gates :98 / :183 (span words)", "none"),
    "lanes8-J8":           (ROWS, 8, {"lanes": 8}, "same", "c2_loglik.hip:462, gate :282 (span words)", "none"),
    "default-J16":         (ROWS, 16, {}, "same", "c2_loglik.hip:462 (groups of 16 lanes)", "none"),
    "wide-J40":            (ROWS, 40, {}, "same", "c2_wide.hip:90 `d <= 0.0`, a workgroup per series", "none"),
    "default-long-J8":     (LONG, 8, {}, LONG_TWINS["default-long-J8"], _VERIFY, "none"),
    "timepar1-J8":         (LONG, 8, {"timepar": 1}, LONG_TWINS["timepar1-J8"], _VERIFY + ", :1010 (width 8 records)", "none"),
    "timepar1-J4":         (LONG, 4, {"timepar": 1}, LONG_TWINS["timepar1-J4"], _VERIFY + ", :690-721 (fmin / prod words)", "none"),
    "timepar1-J2":         (LONG, 2, {"timepar": 1}, LONG_TWINS["timepar1-J2"], _VERIFY + ", :690-721", "none"),
    "timepar_grad1-J8":    (LONG, 8, {"timepar_grad": 1, "factor_iter": 1}, LONG_TWINS["timepar_grad1-J8"],
                            "c2_timepar_grad.hip:1292 `!(dn < huge)`, :370 k_verify_combine", "none"),
    "timepar_grad1-J5":    (LONG, 5, {"timepar_grad": 1, "factor_iter": 1}, LONG_TWINS["timepar_grad1-J5"],
                            "c2_timepar_grad.hip:1292, :370", "none"),
    "timepar_grad1-J2":    (LONG, 2, {"timepar_grad": 1, "factor_iter": 1}, LONG_TWINS["timepar_grad1-J2"],
                            "c2_timepar_grad.hip:1292, :370", "none"),
}
FACTOR_PATHS = {
    "default-J8":          (ROWS, 8, {}, "same", "c2_ops.hip:187 `d <= 0.0` (NaN passes, as in the reference)", "none"),
    "default-J3":          (ROWS, 3, {}, "same", "c2_ops.hip:187", "none"),
    "default-long-J8":     (LONG, 8, {}, FACTOR_TWINS["default-long-J8"], "c2_loglik.hip:1620 (scanned chunk states), gate :1631; " + _VERIFY, "none"),
    "timepar1-J4":         (LONG, 4, {"timepar": 1}, FACTOR_TWINS["timepar1-J4"], "c2_timepar.hip:1375, :1410; " + _VERIFY, "none"),
    "timepar1-J2":         (LONG, 2, {"timepar": 1}, FACTOR_TWINS["timepar1-J2"], "c2_timepar.hip:1553; " + _VERIFY, "none"),
}
# the sweeps have no pivot: the row-by-row and column-tiled kernels owe the same-options twin
SWEEP_PATHS = {
    # id: (shape class, J, nrhs, forced options, with the F workspace, which ops, twin)
    "nrhs1-J8":            (ROWS, 8, 1, {}, False, "all", "same"),
    "nrhs1-J8-F":          (ROWS, 8, 1, {}, True, "all", "same"),
    "nrhs3-J8":            (ROWS, 8, 3, {}, False, "all", "same"),
    "nrhs3-J5-F":          (ROWS, 5, 3, {}, True, "all", "same"),
    "nrhs8-J8":            (ROWS, 8, 8, {}, False, "all", "same"),
    "nrhs8-J8-F":          (ROWS, 8, 8, {}, True, "all", "same"),
    "nrhs20-J8":           (ROWS, 8, 20, {}, False, "all", "same"),
    "nrhs20-J16-F":        (ROWS, 16, 20, {}, True, "all", "same"),
    "nrhs70-J8-solve_cols1": (ROWS, 8, 70, {"solve_cols": 1}, False, "solve", "same"),
    "long-nrhs1-J8":       (LONG, 8, 1, {}, False, "all", ({"timepar": 0},)),
    "long-nrhs1-J8-timepar1": (LONG, 8, 1, {"timepar": 1}, False, "solve", ({"timepar": 0},)),
    "long-nrhs3-J8-F":     (LONG, 8, 3, {}, True, "all", "same"),
    "long-nrhs8-J8-scan_min_chunk64": (LONG, 8, 8, {"scan_min_chunk": 64, "scan_min_rows": 256}, False, "matmul", "same"),
    "long-nrhs1-J5-scan_min_chunk128": (LONG, 5, 1, {"scan_min_chunk": 128, "scan_min_rows": 256}, True, "matmul", "same"),
    "long-nrhs70-J8-solve_cols1": (LONG, 8, 70, {"solve_cols": 1}, False, "solve", "same"),
}
# per path: (the line that decides which kernel runs / whether a fallback exists, the loop finding).  None of these kernels
# compares a value: they carry IEEE arithmetic only, so a NaN stays in its series and its column; their loops run over rows,
# right-hand sides and chunks by count.
_SW = "c2_ops.hip:1527-1560 launch_sweep picks the kernel from B, N, J, nrhs and alignment only; "
SWEEP_DECIDES = {
    "nrhs1-J8":            (_SW + "c2_sweep.hip:778 k_sweep1 (rows as 128-byte lines)", "none"),
    "nrhs1-J8-F":          (_SW + "c2_sweep.hip:778 k_sweep1 with the workspace", "none"),
    "nrhs3-J8":            (_SW + "c2_sweep_small.hip:179 k_sweepT (two to five right-hand sides)", "none"),
    "nrhs3-J5-F":          (_SW + "c2_sweep_small.hip:179 k_sweepT with the workspace", "none"),
    "nrhs8-J8":            (_SW + "c2_sweep.hip:871-919 k_sweepK / the 8 x 8 lines", "none"),
    "nrhs8-J8-F":          (_SW + "c2_sweep.hip:871-919 with the workspace", "none"),
    "nrhs20-J8":           (_SW + "c2_sweep_cols.hip:646 (9 .. 32 right-hand sides at J = 8, columns per lane)", "none"),
    "nrhs20-J16-F":        (_SW + "c2_ops.hip:1404-1420 lanes over the right-hand sides", "none"),
    "nrhs70-J8-solve_cols1": ("c2_ops.hip:1433 / c2_solve_cols.hip:259 chunk maps, lanes over the right-hand sides; no verification", "none"),
    "long-nrhs1-J8":       ("c2_ops.hip:1508 c2_internal_use_timepar_solve (c2_loglik.hip:1326): the affine chunk maps of "
                            "c2_timepar.hip:1930 k_tps_apply have no verification word -- measured: the same-options twin; "
                            "{timepar: 0} is the row-by-row sweep the table would name if one were added", "none"),
    "long-nrhs1-J8-timepar1": ("c2_ops.hip:1508, forced", "none"),
    "long-nrhs3-J8-F":     ("c2_ops.hip:1508 declines (F / several right-hand sides): the chunk-map solves from long_min_rows, "
                            "c2_timepar_grad.hip:1073 solve_chunks; no verification", "none"),
    "long-nrhs8-J8-scan_min_chunk64": ("c2_ops.hip:1465 run_chunked (c2_scan.hip k_mm_chunk / k_mm_carry)", "none"),
    "long-nrhs1-J5-scan_min_chunk128": ("c2_ops.hip:1465", "none"),
    "long-nrhs70-J8-solve_cols1": ("c2_ops.hip:1433 / c2_solve_cols.hip:259", "none"),
}
_SWR = "c2_ops.hip:1699-1728 launch_sweep_rev picks the kernel from B, N, J, nrhs only; "
SWEEP_REV_DECIDES = {
    "nrhs1-J8":            (_SWR + "c2_sweep.hip:821 k_sweep1_rev", "none"),
    "nrhs3-J5":            (_SWR + "c2_sweep_small_rev.hip:232 k_sweepT_rev", "none"),
    "nrhs8-J8":            (_SWR + "c2_ops.hip:1720 k_sweepK_rev / the 8 x 8 lines", "none"),
    "nrhs20-J8":           (_SWR + "c2_sweep_cols.hip:692 column slices", "none"),
    "long-nrhs1-J8":       ("c2_ops.hip:1676-1691 c2_internal_sweep_rev_long (opposite sweep + per-row pass); rev_long = 0 is "
                            "the row-by-row kernel it replaces -- no verification word, so the same-options twin is expected "
                            "and {rev_long: 0} is accepted only as the form the switch names", "none"),
    "long-nrhs3-J8-rev_long1": ("c2_ops.hip:1676-1691, forced", "none"),
}
FACTOR_REV_DECIDES = {
    "default-J8":          ("c2_ops.hip:1862 c2_internal_factor_rev_replay without a gate: one kernel, no cross-series word", "none"),
    "default-J3":          ("c2_ops.hip:1862", "none"),
    "long-J8-timepar_grad1": ("c2_ops.hip:1858 c2_internal_factor_rev_long; k_verify_combine (c2_timepar_grad.hip:370) sends the "
                              "batch to the replay kernel behind its word (c2_loglik.hip:1695 verify_fallback_enabled) = "
                              "{timepar_grad: 0}", "none"),
}
# the reverse sweeps: (shape class, J, nrhs, forced options, twin)
SWEEP_REV_PATHS = {
    "nrhs1-J8":            (ROWS, 8, 1, {}, "same"),
    "nrhs3-J5":            (ROWS, 5, 3, {}, "same"),
    "nrhs8-J8":            (ROWS, 8, 8, {}, "same"),
    "nrhs20-J8":           (ROWS, 8, 20, {}, "same"),
    "long-nrhs1-J8":       (LONG, 8, 1, {}, ({"rev_long": 0},)),
    "long-nrhs3-J8-rev_long1": (LONG, 8, 3, {"rev_long": 1}, ({"rev_long": 0},)),
}
# factor_rev with a poisoned cotangent (bd / bW): (shape class, J, forced options, twin)
FACTOR_REV_PATHS = {
    "default-J8":          (ROWS, 8, {}, "same"),
    "default-J3":          (ROWS, 3, {}, "same"),
    "long-J8-timepar_grad1": (LONG, 8, {"timepar_grad": 1, "factor_iter": 1}, ({"timepar_grad": 0},)),
}

# Entry points NOT run poisoned here, and why (the issue's safety precondition asks for the kernels to be read first):
NOT_RUN = {
    "general_matmul_lower/upper": "c2_general_tile.hip:217 / :275 are event loops over the merged time grids; they were not "
                                  "read to the end for this file, so no poisoned input is sent to them",
    "predict_at / sample_at": "the event loops of c2_predvar.hip / c2_priordraw.hip: as above",
}


# ---- the ops that consume a factor (d, W) --------------------------------------------------------------------------------
# B = 9 series of 33 rows; one series' d row, W entry or Z0 / z / alpha entry set to NaN.  These ops have no pivot test, no
# verification word and no fallback: every healthy series owes the bits of the clean run (criterion (d) as bit-identity),
# and (b) is held against the numpy restatements under tests/*_ref.py run on the same poisoned arrays.
# Loop reading (none value-steered): c2_invdiag.hip, c2_gram.hip, c2_trial_project.hip and the one sweep of c2_periodogram.hip,
# c2_transit.hip and c2_kepler.hip (c2_trial_sweep.hpp:89) loop over rows, trials and columns by count; c2_trial_columns.hpp:98 is three
# fixed Newton steps on the TRIAL's eccentric anomaly and :41 / :73 round phases of t x trial (times and trials are never
# poisoned); the event loop of c2_predvar.hip:100 runs N + M times and picks data or query by `tn <= tq` (:110), times only.
CONSUMER_SHAPE = dict(B=9, N=33, rows=(0, 16, 32), series=(0, 4, 8))
CONSUMERS = {
    # op: (poison kinds, the line that keeps series apart)
    "inverse_diag":        (("d_nan", "W_nan", "Z0_nan"), "c2_invdiag.hip: a group of lanes per series, no cross-series word"),
    "explained_variance":  (("d_nan", "W_nan"), "c2_predvar.hip:110 the merge compares times only"),
    "whitened_gram":       (("d_nan", "W_nan", "Z0_nan"), "c2_gram.hip: S in the registers of the series' own lanes"),
    "whitened_sinusoids":  (("d_nan", "W_nan", "Z0_nan"), "c2_periodogram.hip via c2_trial_sweep.hpp:89: a lane per frequency of ONE series"),
    "whitened_transits":   (("d_nan", "W_nan", "Z0_nan"), "c2_transit.hip via c2_trial_sweep.hpp:89"),
    "whitened_keplerians": (("d_nan", "W_nan", "Z0_nan"), "c2_kepler.hip via c2_trial_sweep.hpp:89"),
    "trial_projections":   (("alpha_nan",), "c2_trial_project.hip: the contraction runs per series"),
}


def consumer_case(oracle, J, seed=0):
    """Factors of a problem() batch from the oracle and the side inputs of the seven ops."""
    import kepler_ref, periodogram_ref, predict_at_ref, transit_ref
    B, N = CONSUMER_SHAPE["B"], CONSUMER_SHAPE["N"]
    fc = P.factor_case(oracle, B, N, J)
    rng = np.random.default_rng(8100 + J + seed)
    K, M = 8, 7
    return SimpleNamespace(
        B=B, N=N, J=J, t=fc.t, c=fc.c, U=fc.U, W=fc.W, d=fc.d,
        Z0=rng.standard_normal((B, N, 2)), alpha=rng.standard_normal((B, N, 2)),
        freq=np.stack([periodogram_ref.grid(fc.t[b], 5) for b in range(B)]),
        transits=np.stack([transit_ref.trials_for(fc.t[b], K, seed=b) for b in range(B)]),
        keplers=np.stack([kepler_ref.trials_for(fc.t[b], K, seed=b) for b in range(B)]),
        ts=np.stack([predict_at_ref.queries(fc.t[b], rng, M) for b in range(B)]),
        Us=rng.standard_normal((B, M, J)), Vs=rng.standard_normal((B, M, J)))


def consumer_poison(case, kind, series, row):
    out = SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(case).items()})
    if kind == "d_nan":
        out.d[series, row] = NAN
    elif kind == "W_nan":
        out.W[series, row, case.J // 2] = NAN
    elif kind == "Z0_nan":
        out.Z0[series, row, 1] = NAN
    elif kind == "alpha_nan":
        out.alpha[series, row, 1] = NAN
    else:
        raise ValueError(kind)
    assert np.array_equal(out.t, case.t) and np.array_equal(out.c, case.c) and np.array_equal(out.ts, case.ts)
    return out


def consumer_inputs(op, x):
    """The arrays an op takes, in the order of both celerite2_amd.ops.<op> and its restatement."""
    fac = (x.t, x.c, x.U, x.W, x.d)
    return {"inverse_diag": fac + (x.Z0[:, :, 1].copy(),),
            "explained_variance": (x.t, x.ts, x.c, x.U, x.W, x.d, x.Us, x.Vs),
            "whitened_gram": fac + (x.Z0,),
            "whitened_sinusoids": fac + (x.Z0, x.freq),
            "whitened_transits": fac + (x.Z0, x.transits),
            "whitened_keplerians": fac + (x.Z0, x.keplers)}[op]


def consumer_reference(op, x):
    """The numpy restatement of `op` on the arrays of x: a tuple of (B, ...) outputs."""
    import inverse_diag_ref, kepler_ref, linear_model_ref, periodogram_ref, predict_at_ref, transit_ref, trial_projections_ref
    B = x.B
    with np.errstate(all="ignore"):
        if op == "inverse_diag":
            res = [inverse_diag_ref.inverse_diag(*[a[b] for a in consumer_inputs(op, x)]) for b in range(B)]
            return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        if op == "explained_variance":
            return (np.stack([predict_at_ref.explained_variance(*[a[b] for a in consumer_inputs(op, x)]) for b in range(B)]),)
        if op == "trial_projections":
            return tuple(trial_projections_ref.projections_batched(kind, x.t, x.alpha, tr)
                         for kind, tr in (("periodogram", x.freq), ("transit", x.transits), ("keplerian", x.keplers)))
        f = {"whitened_gram": linear_model_ref.whitened_gram_batched, "whitened_sinusoids": periodogram_ref.whitened_sinusoids_batched,
             "whitened_transits": transit_ref.whitened_transits_batched, "whitened_keplerians": kepler_ref.whitened_keplerians_batched}[op]
        return (f(*consumer_inputs(op, x)),)


def consumer_device(ops, op, x):
    if op == "trial_projections":
        t, alpha = P.dev(x.t, x.alpha)
        return tuple(ops.trial_projections(kind, t, alpha, P.dev(tr)[0])
                     for kind, tr in (("periodogram", x.freq), ("transit", x.transits), ("keplerian", x.keplers)))
    res = getattr(ops, op)(*P.dev(*consumer_inputs(op, x)))
    return tuple(res) if isinstance(res, tuple) else (res,)


def dot_tril_reference(oracle, x):
    """Z = L sqrt(D) Y (numpy.py:100-102): the oracle's matmul_lower accumulated onto sqrt(d) Y."""
    with np.errstate(all="ignore"):
        Ys = np.sqrt(x.d)[:, :, None] * x.Y
    Z = Ys.copy()
    for b in range(x.B):
        oracle.matmul_lower(x.t[b], x.c[b], x.U[b], x.W[b], np.ascontiguousarray(Ys[b]), Z[b])
    return Z
