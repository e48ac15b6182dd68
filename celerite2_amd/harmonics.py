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

__all__ = ["Harmonics", "NullFactors", "NORMALIZATIONS", "null_products", "finish", "null_factors", "null_statistics", "waveform"]

Harmonics = collections.namedtuple("Harmonics", "power amplitude chi2_null")
NullFactors = collections.namedtuple("NullFactors", "Lm Xt L0 singular bad")


def _check_nterms(nterms):
    if isinstance(nterms, bool) or not isinstance(nterms, int) or nterms < 1:
        raise ValueError("nterms must be a positive integer (got %r)" % (nterms,))


def _factors(S0, T, ok, H):
    """What `finish` and `null_statistics` share, from S0 (B, Q0, Q0) and T (B, F, H (2 H + 1) + 2 H Q0) alone: (S0, T, bad,
    chi2_0, v, Xi, L0, L, sing) -- null_fit's S0, T, bad (B,), chi2_0 (B,), v (B, P0) and L0 (B, P0, P0); Xi[i] (B, P0, F) =
    column i's L0^-1 Gt0^T (None when P0 = 0); L[i][j] (B, F), j <= i, the Cholesky factor of M = Gtt - X^T X, and sing (B, F):
    a pivot below _RANK_TOL of Gtt's own diagonal entry (that pivot is taken as 1: L stays finite)."""
    Q0 = S0.shape[-1]
    NC, HEAD = 2 * H, H * (2 * H + 1)
    S0, T, bad, chi2_0, v, X, L0 = null_fit(S0, T, ok, ("F", "H (2 H + 1) + 2 H Q0", HEAD + NC * Q0),
                                            tuple(HEAD + i * Q0 for i in range(NC)))    # X (B, P0, NC F), column-major
    P0, F = Q0 - 1, T.shape[1]
    one = torch.ones((), dtype=S0.dtype, device=S0.device)
    tri = lambda i, j: i * NC - (i * (i - 1)) // 2 + (j - i)             # (i <= j) of the row-major upper triangle
    Xi = [X[..., i * F:(i + 1) * F] for i in range(NC)] if P0 else None   # (B, P0, F) each
    M = [[None] * NC for _ in range(NC)]                                 # M's lower triangle, (B, F) each
    for i in range(NC):
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
    return S0, T, bad, chi2_0, v, Xi, L0, L, sing


def finish(S0, T, N, nterms, normalization="standard", ok=None):
    """Harmonics(power (B, F), amplitude (B, F, 2 H), chi2_null (B,)) from S0 (B, Q0, Q0), T (B, F, H (2 H + 1) + 2 H Q0),
    the series length N and H = nterms (the module docstring has the formulas).  power: dchi2 / chi2_0 ("standard", in
    [0, 1]), dchi2 ("chi2") or dchi2 / 2 ("log_likelihood"); amplitude = (alpha_1, beta_1, ..., alpha_H, beta_H).
    `ok` (B,) | None: series to take at all (the others hold NaN; their S0, T are not read)."""
    if normalization not in NORMALIZATIONS:
        raise ValueError("normalization must be one of %s" % (NORMALIZATIONS,))
    _check_nterms(nterms)
    H, Q0 = nterms, S0.shape[-1]
    NC, HEAD = 2 * H, H * (2 * H + 1)
    S0, T, bad, chi2_0, v, Xi, _, L, sing = _factors(S0, T, ok, H)
    P0 = Q0 - 1
    nan = torch.full((), math.nan, dtype=S0.dtype, device=S0.device)
    r = [None] * NC                                                    # (B, F) each
    for i in range(NC):
        r[i] = T[..., HEAD + i * Q0 + P0]
        if P0:
            r[i] = r[i] - (Xi[i] * v[:, :, None]).sum(dim=1)
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


def null_factors(S0, T, N, nterms, ok=None):
    """NullFactors(Lm, Xt, L0, singular, bad): what does not depend on the draw of the statistic of many series y_r, from the
    observed call's S0 (B, Q0, Q0) and T (B, F, H (2 H + 1) + 2 H Q0) (only the entries without y are read), in the layout
    ops.harmonic_null_chi2 takes.  Lm (B, F, H (2 H + 1)): the factor of M = Gtt - X^T X, its lower triangle row-major, NaN
    throughout at a frequency or in a series that holds NaN (`singular`).  Xt (B, F, 2 H, P0): X = L0^-1 Gt0^T by column, None
    when P0 = 0.  L0 (B, P0, P0) the factor of G00 (the identity in a bad series; None when P0 = 0).  singular (B, F): M not
    positive definite, N < P0 + 2 H + 1, or a bad series.  bad (B,): as null_fit has it."""
    _check_nterms(nterms)
    H, P0 = nterms, S0.shape[-1] - 1
    NC = 2 * H
    S0, T, bad, _, _, Xi, L0, L, sing = _factors(S0, T, ok, H)
    if N < P0 + NC + 1:
        sing = torch.ones_like(sing)
    sing = sing | bad[:, None]
    nan = torch.full((), math.nan, dtype=S0.dtype, device=S0.device)
    Lm = torch.stack([L[i][j] for i in range(NC) for j in range(i + 1)], dim=-1)
    Lm = torch.where(sing[..., None], nan, Lm).contiguous()
    Xt = torch.stack([x.transpose(1, 2) for x in Xi], dim=2).contiguous() if P0 else None     # (B, F, NC, P0)
    return NullFactors(Lm, Xt, L0, sing, bad)


def null_draws(factors, G0Y, s_yy):
    """(V (B, P0, R) = L0^-1 g0y_r -- None when P0 = 0 --, chi2_0 (B, R) = s_yy_r - |v_r|^2) of R series from their
    G0Y (B, P0, R) and s_yy (B, R): the fit without the harmonics, per draw (significance.null_statistics' statements)."""
    if factors.L0 is None:
        return None, s_yy
    G0Y = torch.where(factors.bad[:, None, None], torch.zeros((), dtype=G0Y.dtype, device=G0Y.device), G0Y)
    V = torch.linalg.solve_triangular(factors.L0, G0Y, upper=False).contiguous()   # (the solver may hand back another layout)
    return V, s_yy - (V * V).sum(dim=1)


def normalize(dchi2, chi2_0, normalization):
    """dchi2 (B, F, R) of R series in `normalization`, chi2_0 (B, R) their fits without the harmonics."""
    if normalization == "standard":
        return dchi2 / chi2_0[:, None, :]
    return dchi2 if normalization == "chi2" else 0.5 * dchi2


def null_statistics(S0, T, G0Y, s_yy, P, N, nterms, *, normalization="standard", ok=None):
    """The multi-harmonic statistic of R series at once, (B, F, R), in plain torch: the many-y form of `finish`, with its
    statements.  S0 (B, Q0, Q0) and T (B, F, H (2 H + 1) + 2 H Q0) of the observed call (only S0's A0 block and T's entries
    without y are read); G0Y (B, P0, R) = g0y_r and s_yy (B, R) of the R series; P (B, F, 2 H, R) = gty_r
    (ops.harmonic_projections); N the series length; H = nterms.  Per draw r and frequency, for i = 0 .. 2 H - 1 ascending,

        v_r = L0^-1 g0y_r,   chi2_0_r = s_yy_r - |v_r|^2,   r_i = gty_i - sum_p X[p, i] v_r[p]  (p ascending),
        w_i = (r_i - sum_{k < i} L_ik w_k) / L_ii,           dchi2 = sum_i w_i^2

    then the normalisation: what ops.harmonic_null_chi2 finishes in registers without P in memory.  NaN as `finish` has it:
    a frequency whose M is not positive definite, every frequency when N < P0 + 2 H + 1, a bad series.  With R = 1 and the
    series' own products this is `finish`'s power; nterms = 1 is significance.null_statistics("periodogram", ...)."""
    if normalization not in NORMALIZATIONS:
        raise ValueError("normalization must be one of %s" % (NORMALIZATIONS,))
    fac = null_factors(S0, T, N, nterms, ok)
    NC, (B, F), P0 = 2 * nterms, fac.Lm.shape[:2], S0.shape[-1] - 1
    if P.dim() != 4 or tuple(P.shape[:3]) != (B, F, NC):
        raise ValueError("Invalid shape: P (must be (B, F, 2 H, R) = (%d, %d, %d, R))" % (B, F, NC))
    R = P.shape[-1]
    if tuple(s_yy.shape) != (B, R) or tuple(G0Y.shape) != (B, P0, R):
        raise ValueError("Invalid shape: s_yy, G0Y (must be (B, R) and (B, P0, R) = (%d, %d) and (%d, %d, %d))" % (B, R, B, P0, R))
    V, chi2_0 = null_draws(fac, G0Y, s_yy)
    w = [None] * NC
    dchi2 = torch.zeros_like(P[:, :, 0])
    for i in range(NC):
        x = P[:, :, i]
        if P0:                                                         # (one term after the other: significance._xtv)
            xv = fac.Xt[:, :, i, 0, None] * V[:, 0, None, :]
            for p in range(1, P0):
                xv = xv + fac.Xt[:, :, i, p, None] * V[:, p, None, :]
            x = x - xv
        for k in range(i):
            x = x - fac.Lm[..., i * (i + 1) // 2 + k, None] * w[k]
        w[i] = x / fac.Lm[..., i * (i + 1) // 2 + i, None]
        dchi2 = dchi2 + w[i] * w[i]
    return normalize(dchi2, chi2_0, normalization)


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
