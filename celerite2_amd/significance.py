# -*- coding: utf-8 -*-
"""False-alarm probabilities of the searches (periodogram, transit, keplerian, tabulated shape) under a correlated-noise
covariance, by Monte Carlo under the null: the torch part.  It runs on CPU tensors as well.

The white-noise formulae for the highest peak do not apply under a GP covariance.  What does: draw noise from the factored
covariance, run the same search on every draw, and compare the observed statistic with the distribution of the per-draw
maximum.  With K + D = L diag(d) L^T a draw is  y_r - mean = L D^1/2 n_r,  n_r ~ N(0, I)  (the statistics do not depend on
A0 beta0, so beta0 = 0 is the null), and of everything a search reads only three things depend on the draw:

    z_y = L^-1 (y_r - mean) = D^1/2 n_r                              (never formed)
    s_yy_r = |n_r|^2,      g0y_r = Z_A0^T D^-1/2 n_r                  (Z_A0 = L^-1 A0 from the observed call's Z0)
    gty_r[k] = col_k(t)^T alpha_r,   alpha_r = (K + D)^-1 (y_r - mean) = L^-T D^-1/2 n_r
                                                                     (one solve_upper with R columns, then ops.trial_projections)

Gtt and Gt0 are those of the one sweep the observed search runs anyway (its T).  `null_statistics` is the many-y form of
periodogram.finish / transit.finish / kepler.finish: the null fit's Cholesky and the per-trial Cholesky of M are done once,
then, per draw r,

    v_r = L0^-1 g0y_r,   chi2_0_r = s_yy_r - v_r^T v_r,   r_r = gty_r - X^T v_r,   dchi2_r = r_r^T M^-1 r_r

and the normalisation.  The NaN rules are the finish functions': a singular trial, one outside the domain, a `bad` series,
N too small.  Nothing here raises beyond the shape checks and nothing is read on the host.

The probability is CONDITIONAL ON THE HYPER-PARAMETERS: the kernel is not refitted per draw.
"""
import collections
import math

import torch

from . import kepler as _kp
from . import ops as _ops
from . import periodogram as _pg
from . import shapes as _sh
from . import transit as _tr
from ._trial_fit import null_fit
from .autograd import _RANK_TOL

__all__ = ["Significance", "KINDS", "null_statistics", "false_alarm_probability", "false_alarm_level"]

Significance = collections.namedtuple("Significance", "statistic fap null_maxima")
KINDS = ("periodogram", "transit", "keplerian")

# WHAT DIFFERS BETWEEN THE SEARCHES, beside ops._TRIAL_TABLE's words and columns under the same key:
#   sweep    (t, c, U, W, d, Z0, trials, t_ref, shapes) -> T, the op that whitens the trials' columns
#   project  (t, alpha, trials, t_ref, shapes) -> P (B, K, C, R), the op that contracts them with many vectors
#   finish   (S0, T, N, normalization, ok, trials, n_shapes) -> the fit of the observed series: a two-column kind's has .power,
#            a one-column kind's delta_chi2, chi2_null and, second, the fitted amplitude
#   domain   (trials, n_shapes) -> (..., K) bool, or None where every trial is in the domain
#   dips     whether `dips_only` applies
# KINDS are the ones `search_significance` and `null_statistics` take by name; "shape" has methods of its own (a bank goes
# with its trials).
_Search = collections.namedtuple("_Search", "sweep project finish domain dips")
SEARCHES = {
    "periodogram": _Search(lambda *a, t_ref, shapes: _ops.whitened_sinusoids(*a, t_ref=t_ref),
                           lambda *a, t_ref, shapes: _ops.trial_projections("periodogram", *a, t_ref=t_ref),
                           lambda S0, T, N, norm, ok, trials, n: _pg.finish(S0, T, N, norm, ok=ok), None, False),
    "transit": _Search(lambda *a, t_ref, shapes: _ops.whitened_transits(*a),
                       lambda *a, t_ref, shapes: _ops.trial_projections("transit", *a),
                       lambda S0, T, N, norm, ok, trials, n: _tr.finish(S0, T, N, ok=ok, trials=trials),
                       lambda trials, n: _tr.in_domain(trials), True),
    "keplerian": _Search(lambda *a, t_ref, shapes: _ops.whitened_keplerians(*a),
                         lambda *a, t_ref, shapes: _ops.trial_projections("keplerian", *a),
                         lambda S0, T, N, norm, ok, trials, n: _kp.finish(S0, T, N, norm, ok=ok, trials=trials),
                         lambda trials, n: _kp.in_domain(trials), False),
    "shape": _Search(lambda *a, t_ref, shapes: _ops.whitened_shapes(*a, shapes),
                     lambda *a, t_ref, shapes: _ops.shape_projections(*a, shapes),
                     lambda S0, T, N, norm, ok, trials, n: _sh.finish(S0, T, N, ok=ok, trials=trials, n_shapes=n), _sh.in_domain, True),
}


def check_trials(kind, trials, B, name="trials", count="K"):
    """`trials` contiguous, after the shape check every search makes on them: (K,) | (B, K) at one double per trial,
    (K, words) | (B, K, words) otherwise, K >= 1."""
    words = _ops._TRIAL_TABLE[kind].words
    lead = 1 if words == 1 else 2
    if not torch.is_tensor(trials) or trials.dim() not in (lead, lead + 1) or (trials.dim() == lead + 1 and trials.shape[0] != B) \
            or (lead == 2 and trials.shape[-1] != words) or trials.shape[-lead] < 1:
        raise ValueError("Invalid shape: %s (must be %s with B = %d, %s >= 1)"
                         % (name, "(F,) or (B, F)" if lead == 1 else "(K, %d) or (B, K, %d)" % (words, words), B, count))
    return trials.contiguous()


def _xtv(X, V):
    """X^T V (B, K, R) for X (B, P0, K), V (B, P0, R), one term of the sum after the other: the value at (k, r) does not
    depend on how many trials or draws the call holds (a library product may pick another order at another size)."""
    out = X[:, 0, :, None] * V[:, 0, None, :]
    for p in range(1, X.shape[1]):
        out = out + X[:, p, :, None] * V[:, p, None, :]
    return out


def _normalize(dchi2, chi2_0, normalization):
    if normalization == "standard":
        return dchi2 / chi2_0
    return dchi2 if normalization == "chi2" else 0.5 * dchi2


def null_statistics(kind, S0, T, G0Y, s_yy, P, N, *, normalization="standard", trials=None, dips_only=False, ok=None):
    """The search statistic of R series at once, (B, K, R): `kind` in KINDS; S0 (B, Q0, Q0) and T (B, K, width) of the
    observed call (only S0's A0 block G00 = S0[:P0, :P0] and T's entries without y are read); G0Y (B, P0, R) = g0y_r and
    s_yy (B, R) of the R series; P (B, K, C, R) = gty_r (ops.trial_projections; C = 1 for the transit, 2 otherwise); N the
    series length.  `normalization`: dchi2 / chi2_0 ("standard"), dchi2 ("chi2") or dchi2 / 2 ("log_likelihood"), for the
    transit as well (its delta_chi2 is "chi2").  `trials`: the trials T was made from, to hold NaN outside the domain
    (transit, keplerian).  `dips_only` (transit): a trial whose fitted depth is positive counts 0.  `ok` (B,) | None: series
    to take at all.  With R = 1 and the series' own products this is the `finish` of the kind."""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s" % (KINDS,))
    return _null_statistics(kind, S0, T, G0Y, s_yy, P, N, normalization, trials, None, dips_only, ok)


def _null_statistics(kind, S0, T, G0Y, s_yy, P, N, normalization, trials, n_shapes, dips_only, ok):
    """null_statistics for any kind of SEARCHES; `n_shapes`: the bank's, for the shape's domain."""
    if normalization not in _pg.NORMALIZATIONS:
        raise ValueError("normalization must be one of %s" % (_pg.NORMALIZATIONS,))
    Q0 = S0.shape[-1]
    words, C, domain = _ops._TRIAL_TABLE[kind].words, _ops._TRIAL_TABLE[kind].columns, SEARCHES[kind].domain
    two = C == 2
    layout = ("K", "3 + 2 Q0", 3 + 2 * Q0) if two else ("K", "1 + Q0", 1 + Q0)
    S0, T, bad, _, _, X, L0 = null_fit(S0, T, ok, layout, (3, 3 + Q0) if two else (1,))
    B, P0, K = S0.shape[0], Q0 - 1, T.shape[1]
    if P.dim() != 4 or tuple(P.shape[:3]) != (B, K, C):
        raise ValueError("Invalid shape: P (must be (B, K, C, R) = (%d, %d, %d, R))" % (B, K, C))
    R = P.shape[-1]
    if tuple(s_yy.shape) != (B, R) or tuple(G0Y.shape) != (B, P0, R):
        raise ValueError("Invalid shape: s_yy, G0Y (must be (B, R) and (B, P0, R) = (%d, %d) and (%d, %d, %d))" % (B, R, B, P0, R))
    if domain is None:
        trials = None
    if trials is not None:
        if trials.dim() not in (2, 3) or tuple(trials.shape[-2:]) != (K, words) or (trials.dim() == 3 and trials.shape[0] != B):
            raise ValueError("Invalid shape: trials (must be (K, %d) or (B, K, %d) = (%d, %d, %d))" % (words, words, B, K, words))
    nan = torch.full((), math.nan, dtype=S0.dtype, device=S0.device)
    one = torch.ones((), dtype=S0.dtype, device=S0.device)
    chi2_0 = s_yy
    if P0:
        G0Y = torch.where(bad[:, None, None], torch.zeros((), dtype=S0.dtype, device=S0.device), G0Y)
        V = torch.linalg.solve_triangular(L0, G0Y, upper=False)                                          # (B, P0, R)
        chi2_0 = s_yy - (V * V).sum(dim=1)
    chi2_0 = chi2_0[:, None, :]
    if two:
        a, b, c = T[..., 0], T[..., 1], T[..., 2]
        r1, r2 = P[:, :, 0], P[:, :, 1]
        if P0:
            Xc, Xs = X[..., :K], X[..., K:]
            a_, b_, c_ = a - (Xc * Xc).sum(dim=1), b - (Xc * Xs).sum(dim=1), c - (Xs * Xs).sum(dim=1)
            r1, r2 = r1 - _xtv(Xc, V), r2 - _xtv(Xs, V)
        else:
            a_, b_, c_ = a, b, c
        sing = ~(a_ > _RANK_TOL * a)
        l11 = torch.sqrt(torch.where(sing, one, a_))
        l21 = b_ / l11
        p22 = c_ - l21 * l21
        sing = sing | ~(p22 > _RANK_TOL * c)
        l22 = torch.sqrt(torch.where(sing, one, p22))
        w1 = r1 / l11[..., None]
        w2 = (r2 - l21[..., None] * w1) / l22[..., None]
        stat = _normalize(w1 * w1 + w2 * w2, chi2_0, normalization)
        if N < P0 + 3:
            sing = torch.ones_like(sing)
    else:
        M = zz = T[..., 0]
        r = P[:, :, 0]
        if P0:
            M = zz - (X * X).sum(dim=1)
            r = r - _xtv(X, V)
        sing = ~(M > _RANK_TOL * zz)
        if N < P0 + 2:
            sing = torch.ones_like(sing)
        snr = r / torch.sqrt(torch.where(sing | bad[:, None], one, M))[..., None]
        stat = _normalize(snr * snr, chi2_0, normalization)
        if dips_only and SEARCHES[kind].dips:
            stat = torch.where(r > 0, torch.zeros((), dtype=S0.dtype, device=S0.device), stat)
    if trials is not None:
        sing = sing | ~domain(trials, n_shapes).expand(B, K)
    return torch.where((sing | bad[:, None])[..., None], nan, stat)


def observed_statistic(kind, S0, T, N, normalization, trials, n_shapes, dips_only, ok):
    """(B, K): the statistic of the observed series from its own products -- the power of a two-column kind; of a
    one-column kind delta_chi2 in `normalization`, with `dips_only` 0 where the fitted amplitude is positive."""
    fit = SEARCHES[kind].finish(S0, T, N, normalization, ok, trials, n_shapes)
    if _ops._TRIAL_TABLE[kind].columns == 2:
        return fit.power
    statistic = _normalize(fit.delta_chi2, fit.chi2_null[:, None], normalization)
    return torch.where(fit[1] > 0, torch.zeros_like(statistic), statistic) if dips_only and SEARCHES[kind].dips else statistic


def false_alarm_probability(statistic, maxima, *, rtol=0.0):
    """(1 + #{r : maxima[b, r] >= statistic[b, ...]}) / (R + 1) for statistic (B, ...) and the per-draw maxima (B, R): the
    Monte-Carlo false-alarm probability with the observed series counted among the draws, so it lies in [1 / (R + 1), 1]
    and is never 0.  NaN where the statistic is NaN; a NaN maximum (a draw with no valid trial) is never at or above.
    `rtol`: a maximum within rtol |statistic| below the statistic counts as at it (the larger, conservative probability) --
    for maxima and statistics that reach the same value by different routes and agree only to rounding."""
    B, R = maxima.shape
    if statistic.shape[0] != B:
        raise ValueError("Invalid shape: statistic (must be (B, ...) with B = %d)" % B)
    void = torch.isnan(maxima)
    srt = torch.sort(torch.where(void, torch.full_like(maxima, -math.inf), maxima), dim=1)[0]   # (the NaN ones first)
    flat = statistic.reshape(B, -1)
    gone = torch.isnan(flat)
    if rtol:
        flat = flat - rtol * flat.abs()
    below = torch.searchsorted(srt, torch.where(gone, torch.zeros_like(flat), flat).contiguous(), right=False)   # maxima < statistic
    below = torch.maximum(below, void.sum(dim=1, keepdim=True))
    # (a tensor divisor: the device divides by a Python number as a product with its reciprocal, one bit off the quotient)
    fap = (1.0 + (R - below).to(maxima.dtype)) / torch.full((), R + 1.0, dtype=maxima.dtype, device=maxima.device)
    return torch.where(gone, torch.full_like(fap, math.nan), fap).reshape(statistic.shape)


def false_alarm_level(maxima, fap):
    """(B,): the quantile of the per-draw maxima (B, R) that a statistic has to reach for a false-alarm probability of at
    most `fap` -- the m-th largest maximum, m = floor(fap (R + 1)) - 1, so that false_alarm_probability(level) <= fap.
    +inf where R draws cannot resolve `fap` (m < 1: fap < 2 / (R + 1)); NaN maxima are ignored (taken as -inf)."""
    fap = float(fap)
    if not 0.0 < fap <= 1.0:
        raise ValueError("fap must be in (0, 1]")
    B, R = maxima.shape
    m = min(int(math.floor(fap * (R + 1.0) + 1e-9)) - 1, R)
    if m < 1:
        return torch.full((B,), math.inf, dtype=maxima.dtype, device=maxima.device)
    srt = torch.sort(torch.where(torch.isnan(maxima), torch.full_like(maxima, -math.inf), maxima), dim=1, descending=True)[0]
    return srt[:, m - 1]
