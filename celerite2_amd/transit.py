# -*- coding: utf-8 -*-
"""The transit search (box least squares) under a correlated-noise covariance: the torch part.

For each trial (period P, epoch t0, duration w, ingress tau) the model  y = mean + A0 beta0 + delta b_k(t) + GP, b_k a box
or trapezoid template folded at P (P = 0: a single event), is fitted by generalized least squares and compared with the fit
without the template.  Everything that costs O(N) per trial is in one kernel (ops.whitened_transits, csrc/c2_transit.hip;
include/celerite2_amd_transit.h has the rule for b_k); what is left is algebra on (B, K, .) arrays, here, in plain torch.
With K + D = L diag(d) L^T, Z0 = L^-1 [A0 | y - mean] (B, N, Q0 = P0 + 1), z = L^-1 b_k and <a, b> = sum_n a_n b_n / d_n:

    S0 = Z0^T diag(1/d) Z0     ->  G00 = S0[:P0, :P0],  g0y = S0[:P0, P0],  s_yy = S0[P0, P0]   (_trial_fit.null_products)
    T[b, k] (whitened_transits) ->  <z, z> = T[0],  Gt0 (P0) = T[1:1+P0],  gty = T[1+P0]
    chi2_0 = s_yy - g0y^T G00^-1 g0y               (the fit without the template; one per series)
    M      = <z, z> - Gt0 G00^-1 G0t,   r = gty - Gt0 G00^-1 g0y
    depth  = r / M,   depth_err = M^-1/2,   dchi2 = r^2 / M,   snr = r / sqrt(M)

With P0 = 0 the G00 terms vanish.  A dip has a NEGATIVE depth and snr (b_k is +1 in transit).  Nothing here raises and
nothing is read on the host: a trial whose M is not above _RANK_TOL <z, z> (no sample in transit; a template inside the span
of A0) holds NaN, so does a trial outside the domain w > 0, 0 <= tau <= w / 2, P >= 0, w <= P when P > 0 (when `trials` is
given), so does every trial when N < P0 + 2, and a series with a rank-deficient G00 or a failed factorisation is NaN
throughout.
"""
import collections
import math

import torch

from ._trial_fit import null_fit
from .autograd import _RANK_TOL

__all__ = ["TransitSearch", "finish", "trial_grid", "in_domain"]

TransitSearch = collections.namedtuple("TransitSearch", "delta_chi2 depth depth_err snr chi2_null")


def in_domain(trials):
    """(..., K) bool: the trials (..., K, 4) = (P, t0, w, tau) with w > 0, 0 <= tau <= w / 2, P >= 0 and w <= P when P > 0."""
    P, w, tau = trials[..., 0], trials[..., 2], trials[..., 3]
    return (w > 0) & (tau >= 0) & (tau <= 0.5 * w) & (P >= 0) & ((P == 0) | (w <= P))


def finish(S0, T, N, ok=None, trials=None):
    """TransitSearch(delta_chi2, depth, depth_err, snr (each (B, K)), chi2_null (B,)) from S0 (B, Q0, Q0), T (B, K, 1 + Q0)
    and the series length N (the module docstring has the formulas).  `ok` (B,) | None: series to take at all (the others
    hold NaN; their S0, T are not read).  `trials` (K, 4) | (B, K, 4) | None: the trials T was made from, to hold NaN where one
    is outside the domain."""
    Q0 = S0.shape[-1]
    S0, T, bad, chi2_0, v, X, _ = null_fit(S0, T, ok, ("K", "1 + Q0", 1 + Q0), (1,))                 # X (B, P0, K)
    B, P0, K = S0.shape[0], Q0 - 1, T.shape[1]
    if trials is not None and (trials.dim() not in (2, 3) or tuple(trials.shape[-2:]) != (K, 4)
                               or (trials.dim() == 3 and trials.shape[0] != B)):
        raise ValueError("Invalid shape: trials (must be (K, 4) or (B, K, 4) = (%d, %d, 4))" % (B, K))
    nan = torch.full((), math.nan, dtype=S0.dtype, device=S0.device)
    M = zz = T[..., 0]
    r = T[..., 1 + P0]
    if P0:
        M = zz - (X * X).sum(dim=1)
        r = r - (X * v[:, :, None]).sum(dim=1)
    sing = ~(M > _RANK_TOL * zz)
    if trials is not None:
        sing = sing | ~in_domain(trials)
    if N < P0 + 2:
        sing = torch.ones_like(sing)
    sing = sing | bad[:, None]
    M = torch.where(sing, torch.ones((), dtype=S0.dtype, device=S0.device), M)
    rootM = torch.sqrt(M)
    snr = r / rootM
    out = [snr * snr, r / M, 1.0 / rootM, snr]
    return TransitSearch(*[torch.where(sing, nan, x) for x in out], torch.where(bad, nan, chi2_0))


def trial_grid(periods, durations, *, phase_step=0.25, t0=0.0, ingress=0.0):
    """(K, 4) trials (P, t0, w, tau) for a folded search: for each period and each duration w <= P, epochs
    t0 + m phase_step w for m = 0 .. ceil(P / (phase_step w)) - 1 (one period in steps of `phase_step` durations), with
    tau = ingress w (`ingress` in [0, 1/2]: 0 the box, 1/2 the triangle).  Period-major, then duration, then epoch.
    `periods`, `durations`: sequences or 1-d tensors (their values are read on the host to count the epochs); the result is
    float64 on the device of `periods` when that is a tensor."""
    if not 0.0 < phase_step:
        raise ValueError("phase_step must be positive")
    if not 0.0 <= ingress <= 0.5:
        raise ValueError("ingress must be in [0, 1/2] (a fraction of the duration)")
    dev = periods.device if torch.is_tensor(periods) else None
    periods = torch.as_tensor(periods, dtype=torch.float64).reshape(-1).tolist()
    durations = torch.as_tensor(durations, dtype=torch.float64).reshape(-1).tolist()
    if not all(p > 0 for p in periods) or not all(w > 0 for w in durations):
        raise ValueError("periods and durations must be positive")
    blocks = []
    for p in periods:
        for w in durations:
            if w > p:
                continue
            m = torch.arange(int(math.ceil(p / (phase_step * w))), dtype=torch.float64)
            one = torch.ones_like(m)
            blocks.append(torch.stack([p * one, t0 + m * (phase_step * w), w * one, ingress * w * one], dim=1))
    out = torch.cat(blocks) if blocks else torch.zeros((0, 4), dtype=torch.float64)
    return out if dev is None else out.to(dev)
