# -*- coding: utf-8 -*-
"""The Keplerian search (the radial-velocity periodogram of an eccentric orbit) under a correlated-noise covariance: the
torch part.

For each trial (angular frequency w = 2 pi / P, eccentricity e, time of periastron tp) the model

    y = mean + A0 beta0 + K [cos(nu(t) + omega) + e cos omega] + GP,      nu(t): the true anomaly of the orbit (w, e, tp),

is linear in (alpha, beta) = (K cos omega, -K sin omega) on the two columns cos nu(t), sin nu(t); its constant K e cos omega
is absorbed by a constant column of A0 (A="mean", or a design matrix with one).  It is fitted by generalized least squares
and compared with the fit without the orbit.  Everything that costs O(N) per trial is in one kernel (ops.whitened_keplerians,
csrc/c2_kepler.hip; include/celerite2_amd_kepler.h has the rule for the columns and the solver of Kepler's equation), which
writes the layout of ops.whitened_sinusoids: what is left is periodogram.finish, unchanged, and

    semi_amplitude K = hypot(alpha, beta),   omega = atan2(-beta, alpha)          (the argument of periastron, in (-pi, pi])

Nothing here raises beyond the shape checks and nothing is read on the host: a trial outside the domain w > 0,
0 <= e <= MAX_ECC, tp finite holds NaN (when `trials` is given), beside the NaN rules of periodogram.finish.
"""
import collections
import math

import torch

from . import periodogram as _pg

__all__ = ["KeplerianSearch", "MAX_ECC", "in_domain", "finish", "trial_grid", "profile"]

KeplerianSearch = collections.namedtuple("KeplerianSearch", "power amplitude semi_amplitude omega chi2_null")
MAX_ECC = 0.99   # C2_KEPLER_MAX_ECC of the header: the solver's fixed sequence reaches rounding level up to it


def in_domain(trials):
    """(..., K) bool: the trials (..., K, 3) = (w, e, tp) with w > 0, 0 <= e <= MAX_ECC and tp finite."""
    w, e, tp = trials[..., 0], trials[..., 1], trials[..., 2]
    return (w > 0) & (e >= 0) & (e <= MAX_ECC) & torch.isfinite(tp)


def finish(S0, T, N, normalization="standard", ok=None, trials=None):
    """KeplerianSearch(power (B, K), amplitude (B, K, 2) = (alpha, beta), semi_amplitude (B, K), omega (B, K),
    chi2_null (B,)) from S0 (B, Q0, Q0), T (B, K, 3 + 2 Q0) and the series length N: periodogram.finish on the trials'
    products, then the orbit's semi-amplitude and argument of periastron (the module docstring has the formulas).  `ok`
    (B,) | None: series to take at all (the others hold NaN; their S0, T are not read).  `trials` (K, 3) | (B, K, 3) | None:
    the trials T was made from, to hold NaN where one is outside the domain."""
    fit = _pg.finish(S0, T, N, normalization, ok=ok)
    B, K = fit.power.shape
    power, amplitude = fit.power, fit.amplitude
    if trials is not None:
        if trials.dim() not in (2, 3) or tuple(trials.shape[-2:]) != (K, 3) or (trials.dim() == 3 and trials.shape[0] != B):
            raise ValueError("Invalid shape: trials (must be (K, 3) or (B, K, 3) = (%d, %d, 3))" % (B, K))
        nan = torch.full((), math.nan, dtype=power.dtype, device=power.device)
        out = (~in_domain(trials)).expand(B, K)
        power = torch.where(out, nan, power)
        amplitude = torch.where(out[..., None], nan, amplitude)
    alpha, beta = amplitude[..., 0], amplitude[..., 1]
    return KeplerianSearch(power, amplitude, torch.hypot(alpha, beta), torch.atan2(-beta, alpha), fit.chi2_null)


def trial_grid(freq, ecc, n_phase, *, t0=0.0):
    """(F E n_phase, 3) trials (w, e, tp): the regular grid of the ANGULAR frequencies `freq` (F), the eccentricities `ecc`
    (E) and n_phase times of periastron over one period, tp = t0 + m (2 pi / w) / n_phase for m = 0 .. n_phase - 1.
    Frequency-major, then eccentricity, then tp.  `freq`, `ecc`: sequences or 1-d tensors; the result is float64 on the
    device of `freq` when that is a tensor, and nothing is read on the host."""
    n_phase = int(n_phase)
    if n_phase < 1:
        raise ValueError("n_phase must be at least 1")
    dev = freq.device if torch.is_tensor(freq) else None
    w = torch.as_tensor(freq, dtype=torch.float64, device=dev).reshape(-1)
    e = torch.as_tensor(ecc, dtype=torch.float64).reshape(-1).to(w.device)
    m = torch.arange(n_phase, dtype=torch.float64, device=w.device)
    step = (2.0 * math.pi / w) / n_phase
    shape = (w.numel(), e.numel(), n_phase)
    tp = t0 + m[None, None, :] * step[:, None, None]
    return torch.stack([w[:, None, None].expand(shape), e[None, :, None].expand(shape), tp.expand(shape)], dim=-1).reshape(-1, 3)


def profile(search, F):
    """(power (B, F), index (B, F)): the maximum of `search.power` (B, K) -- a KeplerianSearch, or the power itself -- over the
    K / F trials of each frequency of a regular, frequency-major grid (trial_grid), and the index in 0 .. K - 1 of the
    maximising trial.  NaN trials are ignored; a frequency whose trials are all NaN holds NaN (and the index of its first
    trial)."""
    power = search.power if isinstance(search, KeplerianSearch) else search
    B, K = power.shape
    F = int(F)
    if F < 1 or K % F:
        raise ValueError("Invalid shape: power (B, K) = %s is no regular grid of F = %d frequencies" % ((B, K), F))
    per = K // F
    p = power.reshape(B, F, per)
    gone = torch.isnan(p)
    best, arg = torch.where(gone, torch.full((), -math.inf, dtype=p.dtype, device=p.device), p).max(dim=-1)
    best = torch.where(gone.all(dim=-1), torch.full((), math.nan, dtype=p.dtype, device=p.device), best)
    return best, arg + per * torch.arange(F, device=p.device)[None, :]
