# -*- coding: utf-8 -*-
"""The multi-harmonic (truncated Fourier series) periodogram under a correlated-noise covariance: the torch part.

For each trial frequency w and H = nterms harmonics the model

    y = mean + A0 beta0 + sum_{h=1..H} [alpha_h cos x_h(t) + beta_h sin x_h(t)] + GP,   x_h = fl(fl(h w) * fl(t - t_ref))

is fitted by generalized least squares and compared with the fit without the 2 H columns.  Everything that costs O(N) per
frequency is in one kernel (ops.whitened_harmonics, csrc/c2_harmonics.hip); what is left is algebra on (B, F, .) arrays,
here, in plain torch.  With NC = 2 H columns ordered (c_1, s_1, ..., c_H, s_H), HEAD = H (2 H + 1), Z0 = L^-1 [A0 | y - mean]
(B, N, Q0 = P0 + 1) and <a, b> = sum_n a_n b_n / d_n:

    S0 = Z0^T diag(1/d) Z0       ->  G00 = S0[:P0, :P0],  g0y = S0[:P0, P0],  s_yy = S0[P0, P0]
    T[b, f] (whitened_harmonics) ->  Gtt (NC, NC) from the upper triangle T[:HEAD] (row-major),
                                     Gt0[i] = T[HEAD + i Q0 : HEAD + i Q0 + P0],   gty[i] = T[HEAD + i Q0 + P0]
    chi2_0 = s_yy - g0y^T G00^-1 g0y                 (the fit without the columns; one per series: _trial_fit.null_fit)
    M      = Gtt - Gt0 G00^-1 G0t = Gtt - X^T X,   r = gty - X^T v
    dchi2  = r^T M^-1 r,             (alpha_1, beta_1, ..., alpha_H, beta_H) = M^-1 r

by an NC x NC Cholesky of M per frequency, written out column by column over (B, F) as periodogram.finish writes its 2 x 2
(at H = 1 these are its statements).  Nothing here raises beyond shape checks: a frequency whose M is not positive definite
(a pivot below _RANK_TOL of Gtt's own diagonal entry: w = 0 beside a constant column; a harmonic that aliases onto the
constant or onto another harmonic on an even grid) holds NaN, so does every frequency when N < P0 + 2 H + 1 (no degree of
freedom is left beside the fit), and a series with a rank-deficient G00 or a failed factorisation is NaN throughout.
"""
import collections
import math

import torch

from ._trial_fit import null_fit, null_products
from .autograd import _RANK_TOL
from .periodogram import NORMALIZATIONS

__all__ = ["Harmonics", "NORMALIZATIONS", "null_products", "finish", "waveform"]

Harmonics = collections.namedtuple("Harmonics", "power amplitude chi2_null")


def finish(S0, T, N, nterms, normalization="standard", ok=None):
    """Harmonics(power (B, F), amplitude (B, F, 2 H), chi2_null (B,)) from S0 (B, Q0, Q0), T (B, F, H (2 H + 1) + 2 H Q0),
    the series length N and H = nterms (the module docstring has the formulas).  power: dchi2 / chi2_0 ("standard", in
    [0, 1]), dchi2 ("chi2") or dchi2 / 2 ("log_likelihood"); amplitude = (alpha_1, beta_1, ..., alpha_H, beta_H).
    `ok` (B,) | None: series to take at all (the others hold NaN; their S0, T are not read)."""
    if normalization not in NORMALIZATIONS:
        raise ValueError("normalization must be one of %s" % (NORMALIZATIONS,))
    if isinstance(nterms, bool) or not isinstance(nterms, int) or nterms < 1:
        raise ValueError("nterms must be a positive integer (got %r)" % (nterms,))
    H, Q0 = nterms, S0.shape[-1]
    NC, HEAD = 2 * H, H * (2 * H + 1)
    S0, T, bad, chi2_0, v, X, _ = null_fit(S0, T, ok, ("F", "H (2 H + 1) + 2 H Q0", HEAD + NC * Q0),
                                           tuple(HEAD + i * Q0 for i in range(NC)))     # X (B, P0, NC F), column-major
    P0, F = Q0 - 1, T.shape[1]
    nan = torch.full((), math.nan, dtype=S0.dtype, device=S0.device)
    one = torch.ones((), dtype=S0.dtype, device=S0.device)
    tri = lambda i, j: i * NC - (i * (i - 1)) // 2 + (j - i)             # (i <= j) of the row-major upper triangle
    Xi = [X[..., i * F:(i + 1) * F] for i in range(NC)] if P0 else None   # (B, P0, F) each
    # M's lower triangle and r, (B, F) each
    M = [[None] * NC for _ in range(NC)]
    r = [None] * NC
    for i in range(NC):
        r[i] = T[..., HEAD + i * Q0 + P0]
        if P0:
            r[i] = r[i] - (Xi[i] * v[:, :, None]).sum(dim=1)
        for j in range(i + 1):
            M[i][j] = T[..., tri(j, i)]
            if P0:
                M[i][j] = M[i][j] - (Xi[i] * Xi[j]).sum(dim=1)
    # the Cholesky of M per frequency; a pivot below _RANK_TOL of Gtt's own diagonal entry: not positive definite
    L = [[None] * NC for _ in range(NC)]
    sing = torch.zeros(T.shape[:2], dtype=torch.bool, device=T.device)
    for j in range(NC):
        p = M[j][j]
        for k in range(j):
            p = p - L[j][k] * L[j][k]
        sing = sing | ~(p > _RANK_TOL * T[..., tri(j, j)])
        L[j][j] = torch.sqrt(torch.where(sing, one, p))
        for i in range(j + 1, NC):
            x = M[i][j]
            for k in range(j):
                x = x - L[i][k] * L[j][k]
            L[i][j] = x / L[j][j]
    w = [None] * NC                                                    # L w = r
    dchi2 = torch.zeros_like(r[0])
    for i in range(NC):
        x = r[i]
        for k in range(i):
            x = x - L[i][k] * w[k]
        w[i] = x / L[i][i]
        dchi2 = dchi2 + w[i] * w[i]
    amp = [None] * NC                                                  # L^T amplitude = w
    for i in reversed(range(NC)):
        x = w[i]
        for k in range(i + 1, NC):
            x = x - L[k][i] * amp[k]
        amp[i] = x / L[i][i]
    if N < P0 + NC + 1:
        sing = torch.ones_like(sing)
    sing = sing | bad[:, None]
    if normalization == "standard":
        power = dchi2 / chi2_0[:, None]
    elif normalization == "chi2":
        power = dchi2
    else:
        power = 0.5 * dchi2
    power = torch.where(sing, nan, power)
    amplitude = torch.where(sing[..., None], nan, torch.stack(amp, dim=-1))
    return Harmonics(power, amplitude, torch.where(bad, nan, chi2_0))


def waveform(amplitude, freq, t, *, t_ref=0.0):
    """The fitted periodic part sum_h alpha_h cos x_h + beta_h sin x_h at the times `t`, by the phase rule of the sweep
    (x_h = (h * freq) * (t - t_ref), each product rounded once): amplitude (..., 2 H) as `finish` orders it, freq broadcast
    to amplitude's leading axes ((F,) or (B, F) beside (B, F, 2 H)), t (M,) shared or (B, M) -> (..., M)."""
    if amplitude.dim() < 1 or amplitude.shape[-1] < 2 or amplitude.shape[-1] % 2:
        raise ValueError("Invalid shape: amplitude (must be (..., 2 H))")
    lead = amplitude.shape[:-1]
    try:
        freq = torch.broadcast_to(freq, lead)
    except RuntimeError:
        raise ValueError("Invalid shape: freq (must broadcast to amplitude's leading axes %s)" % (tuple(lead),))
    if t.dim() not in (1, 2) or (t.dim() == 2 and (not lead or t.shape[0] != lead[0])):
        raise ValueError("Invalid shape: t (must be (M,) or (B, M))")
    dt = t - t_ref
    if t.dim() == 2:
        dt = dt.reshape((lead[0],) + (1,) * (len(lead) - 1) + (t.shape[1],))
    out = torch.zeros(tuple(lead) + (t.shape[-1],), dtype=amplitude.dtype, device=amplitude.device)
    for h in range(1, amplitude.shape[-1] // 2 + 1):
        x = (h * freq)[..., None] * dt
        out = out + amplitude[..., 2 * h - 2, None] * torch.cos(x) + amplitude[..., 2 * h - 1, None] * torch.sin(x)
    return out
