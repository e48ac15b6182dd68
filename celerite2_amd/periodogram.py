# -*- coding: utf-8 -*-
"""The generalized Lomb-Scargle periodogram under a correlated-noise covariance: the torch part.

For each trial frequency w the model  y = mean + A0 beta0 + alpha cos w(t - t_ref) + beta sin w(t - t_ref) + GP  is fitted by
generalized least squares and compared with the fit without the sinusoid.  Everything that costs O(N) per frequency is in
one kernel (ops.whitened_sinusoids, csrc/c2_periodogram.hip); what is left is algebra on (B, F, .) arrays, here, in plain
torch.  With K + D = L diag(d) L^T, Z0 = L^-1 [A0 | y - mean] (B, N, Q0 = P0 + 1) and <a, b> = sum_n a_n b_n / d_n:

    S0 = Z0^T diag(1/d) Z0       ->  G00 = S0[:P0, :P0],  g0y = S0[:P0, P0],  s_yy = S0[P0, P0]
    T[b, f] (whitened_sinusoids) ->  Gtt = [[T0, T1], [T1, T2]],  Gt0 (2, P0) = [T[3:3+P0]; T[3+Q0:3+Q0+P0]],
                                     gty = [T[3+P0], T[3+Q0+P0]]
    chi2_0 = s_yy - g0y^T G00^-1 g0y                 (the fit without the sinusoid; one per series)
    M      = Gtt - Gt0 G00^-1 G0t,   r = gty - Gt0 G00^-1 g0y
    dchi2  = r^T M^-1 r,             (alpha, beta) = M^-1 r

With P0 = 0 the G00 terms vanish.  Nothing here raises: a frequency whose M is not positive definite (to _RANK_TOL of
Gtt's own diagonal: w = 0 with a constant column; N <= P0 + 1) holds NaN, so does every frequency when N < P0 + 3 (no degree of
freedom is left beside the fit), and a series with a rank-deficient G00 or a failed factorisation is NaN throughout.
"""
import collections
import math

import torch

from ._trial_fit import null_fit, null_products
from .autograd import _RANK_TOL

__all__ = ["Periodogram", "NORMALIZATIONS", "null_products", "finish"]

Periodogram = collections.namedtuple("Periodogram", "power amplitude chi2_null")
NORMALIZATIONS = ("standard", "chi2", "log_likelihood")


def finish(S0, T, N, normalization="standard", ok=None):
    """Periodogram(power (B, F), amplitude (B, F, 2), chi2_null (B,)) from S0 (B, Q0, Q0), T (B, F, 3 + 2 Q0) and the series
    length N (the module docstring has the formulas).  power: dchi2 / chi2_0 ("standard", in [0, 1]), dchi2 ("chi2") or
    dchi2 / 2 ("log_likelihood": the log-likelihood ratio at fixed hyper-parameters); amplitude = (alpha, beta).
    `ok` (B,) | None: series to take at all (the others hold NaN; their S0, T are not read)."""
    if normalization not in NORMALIZATIONS:
        raise ValueError("normalization must be one of %s" % (NORMALIZATIONS,))
    Q0 = S0.shape[-1]
    S0, T, bad, chi2_0, v, X, _ = null_fit(S0, T, ok, ("F", "3 + 2 Q0", 3 + 2 * Q0), (3, 3 + Q0))   # X (B, P0, 2 F)
    P0, F = Q0 - 1, T.shape[1]
    nan = torch.full((), math.nan, dtype=S0.dtype, device=S0.device)
    a, b, c = T[..., 0], T[..., 1], T[..., 2]                         # Gtt
    r1, r2 = T[..., 3 + P0], T[..., 3 + Q0 + P0]                      # gty
    if P0:
        Xc, Xs = X[..., :F], X[..., F:]                                                                # (B, P0, F) each
        a_, b_, c_ = a - (Xc * Xc).sum(dim=1), b - (Xc * Xs).sum(dim=1), c - (Xs * Xs).sum(dim=1)     # M
        r1, r2 = r1 - (Xc * v[:, :, None]).sum(dim=1), r2 - (Xs * v[:, :, None]).sum(dim=1)           # r
    else:
        a_, b_, c_ = a, b, c
    # the 2 x 2 Cholesky of M per frequency; a pivot below _RANK_TOL of Gtt's own diagonal entry: not positive definite
    one = torch.ones((), dtype=S0.dtype, device=S0.device)
    sing = ~(a_ > _RANK_TOL * a)
    l11 = torch.sqrt(torch.where(sing, one, a_))
    l21 = b_ / l11
    p22 = c_ - l21 * l21
    sing = sing | ~(p22 > _RANK_TOL * c)
    l22 = torch.sqrt(torch.where(sing, one, p22))
    w1 = r1 / l11
    w2 = (r2 - l21 * w1) / l22
    dchi2 = w1 * w1 + w2 * w2
    beta = w2 / l22
    alpha = (w1 - l21 * beta) / l11
    if N < P0 + 3:
        sing = torch.ones_like(sing)
    sing = sing | bad[:, None]
    if normalization == "standard":
        power = dchi2 / chi2_0[:, None]
    elif normalization == "chi2":
        power = dchi2
    else:
        power = 0.5 * dchi2
    power = torch.where(sing, nan, power)
    amplitude = torch.where(sing[..., None], nan, torch.stack([alpha, beta], dim=-1))
    return Periodogram(power, amplitude, torch.where(bad, nan, chi2_0))
