# -*- coding: utf-8 -*-
"""The search for events of a TABULATED SHAPE under a correlated-noise covariance: the torch part.  It runs on CPU tensors
as well.

For each trial (period P, epoch t0, width w, shape index s) the model  y = mean + A0 beta0 + delta b_k(t) + GP, b_k the s-th
profile of a bank of shapes placed at t0 with full width w and folded at P (P = 0: a single event), is fitted by generalized
least squares and compared with the fit without it: transit.py's search with the box or trapezoid replaced by any profile
the host can tabulate -- a limb-darkened transit, a flare, a measured template; with w = P a full phase-folded periodic
template.  A shape is S >= 2 values on a uniform grid from the leading edge (node 0, at -w/2 from the centre) to the
trailing edge (node S - 1, at +w/2), linearly interpolated between nodes and zero outside; a bank is (NS, S) with
NS * S <= 1024.  Everything that costs O(N) per trial is in one kernel (ops.whitened_shapes, csrc/c2_shapes.hip;
include/celerite2_amd_shapes.h has the rule for b_k); what is left is transit.finish's algebra on (B, K, .) arrays under
this module's own domain mask: a trial outside w > 0, P >= 0, w <= P when P > 0, (P, t0, w) finite, s an integer in [0, NS)
holds NaN.  The kernel clamps the index, so such a trial reads shape 0, never outside the bank.

The builders return (S,) float64 tensors with peak value exactly 1, so that the fitted amplitude is the event's extreme
(a transit of depth delta has amplitude -delta); `stack` makes a bank of them.
"""
import collections
import math

import torch

from . import transit as _tr

__all__ = ["ShapeSearch", "finish", "trial_grid", "in_domain", "box", "trapezoid", "limb_darkened", "flare", "stack"]

ShapeSearch = collections.namedtuple("ShapeSearch", "delta_chi2 amplitude amplitude_err snr chi2_null")


def in_domain(trials, n_shapes):
    """(..., K) bool: the trials (..., K, 4) = (P, t0, w, s) with w > 0, P >= 0, w <= P when P > 0, all three finite, and s an
    integer in [0, n_shapes)."""
    P, t0, w, s = trials[..., 0], trials[..., 1], trials[..., 2], trials[..., 3]
    finite = torch.isfinite(P) & torch.isfinite(t0) & torch.isfinite(w)
    return finite & (w > 0) & (P >= 0) & ((P == 0) | (w <= P)) & (s >= 0) & (s < n_shapes) & (s == torch.floor(s))


def finish(S0, T, N, ok=None, trials=None, n_shapes=None):
    """ShapeSearch(delta_chi2, amplitude, amplitude_err, snr (each (B, K)), chi2_null (B,)) from S0 (B, Q0, Q0), T
    (B, K, 1 + Q0) of ops.whitened_shapes and the series length N: transit.finish's formulas (amplitude = its depth).  `ok`
    (B,) | None: series to take at all.  `trials` (K, 4) | (B, K, 4) | None with `n_shapes`: the trials T was made from, to
    hold NaN where one is outside `in_domain`."""
    fit = _tr.finish(S0, T, N, ok=ok, trials=None)
    out = list(fit[:4])
    if trials is not None:
        if n_shapes is None:
            raise ValueError("n_shapes (the number of shapes in the bank) is needed with trials")
        B, K = out[0].shape
        if trials.dim() not in (2, 3) or tuple(trials.shape[-2:]) != (K, 4) or (trials.dim() == 3 and trials.shape[0] != B):
            raise ValueError("Invalid shape: trials (must be (K, 4) or (B, K, 4) = (%d, %d, 4))" % (B, K))
        keep = in_domain(trials, int(n_shapes)).expand(B, K)
        nan = torch.full((), math.nan, dtype=out[0].dtype, device=out[0].device)
        out = [torch.where(keep, x, nan) for x in out]
    return ShapeSearch(*out, fit.chi2_null)


def trial_grid(periods, widths, *, phase_step=0.25, t0=0.0, shape=0):
    """(K, 4) trials (P, t0, w, s) for a folded search: for each period and each width w <= P, epochs t0 + m phase_step w for
    m = 0 .. ceil(P / (phase_step w)) - 1 (one period in steps of `phase_step` widths), all with the shape index `shape`.
    Period-major, then width, then epoch.  `periods`, `widths`: sequences or 1-d tensors (their values are read on the host
    to count the epochs); the result is float64 on the device of `periods` when that is a tensor."""
    if not 0.0 < phase_step:
        raise ValueError("phase_step must be positive")
    if int(shape) != shape or shape < 0:
        raise ValueError("shape must be a non-negative integer (an index into the bank)")
    dev = periods.device if torch.is_tensor(periods) else None
    periods = torch.as_tensor(periods, dtype=torch.float64).reshape(-1).tolist()
    widths = torch.as_tensor(widths, dtype=torch.float64).reshape(-1).tolist()
    if not all(p > 0 for p in periods) or not all(w > 0 for w in widths):
        raise ValueError("periods and widths must be positive")
    blocks = []
    for p in periods:
        for w in widths:
            if w > p:
                continue
            m = torch.arange(int(math.ceil(p / (phase_step * w))), dtype=torch.float64)
            one = torch.ones_like(m)
            blocks.append(torch.stack([p * one, t0 + m * (phase_step * w), w * one, float(shape) * one], dim=1))
    out = torch.cat(blocks) if blocks else torch.zeros((0, 4), dtype=torch.float64)
    return out if dev is None else out.to(dev)


# ---- builders -----------------------------------------------------------------------------------------------------------
def _nodes(S):
    S = int(S)
    if S < 2:
        raise ValueError("a shape has S >= 2 nodes")
    return S


def box(S=2):
    """The box: all ones (closed at both edges).  S = 2 says it all; more nodes give the same column."""
    return torch.ones(_nodes(S), dtype=torch.float64)


def trapezoid(ingress, S):
    """The trapezoid with ramps of `ingress` (0, 1/2] of the width at either end: 0 at the edges, 1 between the corners.  The
    corners must fall on nodes: ingress (S - 1) an integer (ValueError otherwise; S = 1 + m / ingress for any integer m)."""
    S = _nodes(S)
    if not 0.0 < ingress <= 0.5:
        raise ValueError("ingress must be in (0, 1/2] (a fraction of the width)")
    m = int(round(ingress * (S - 1)))
    if m < 1 or abs(ingress * (S - 1) - m) > 1e-9 * (S - 1):
        raise ValueError("ingress * (S - 1) = %r is not an integer: the corners do not fall on nodes" % (ingress * (S - 1),))
    i = torch.arange(S, dtype=torch.float64)
    edge = torch.minimum(i, (S - 1) - i)                    # nodes from the nearer edge
    return torch.clamp(edge / float(m), max=1.0)


def limb_darkened(k, b, u1, u2, S=65, *, quad=64):
    """A transit under the quadratic limb-darkening law I(mu) = 1 - u1 (1 - mu) - u2 (1 - mu)^2 from first to fourth contact:
    radius ratio k, impact parameter b < 1 + k (both in stellar radii).  Node i is the planet's centre at
    x = s sqrt((1 + k)^2 - b^2), s = -1 + 2 i / (S - 1), i.e. a constant speed along the chord; the value is the occulted flux
    there over the largest occulted flux among the nodes (peak 1; 0 at both contacts).  The occulted flux is a midpoint
    rule on a polar grid over the planet's disk, `quad` rings of 2 `quad` sectors, the points outside the star left out."""
    S, quad = _nodes(S), int(quad)
    if not (k > 0 and 0 <= b < 1 + k) or quad < 1:
        raise ValueError("limb_darkened needs k > 0, 0 <= b < 1 + k and quad >= 1")
    s = -1.0 + 2.0 * torch.arange(S, dtype=torch.float64) / (S - 1)
    x = s * math.sqrt((1.0 + k) ** 2 - b * b)
    rho = (torch.arange(quad, dtype=torch.float64) + 0.5) * (k / quad)
    th = (torch.arange(2 * quad, dtype=torch.float64) + 0.5) * (math.pi / quad)
    px = x[:, None, None] + rho[None, :, None] * torch.cos(th)[None, None, :]
    py = b + rho[None, :, None] * torch.sin(th)[None, None, :]
    r2 = px * px + py * py
    mu = torch.sqrt(torch.clamp(1.0 - r2, min=0.0))
    inten = 1.0 - u1 * (1.0 - mu) - u2 * (1.0 - mu) ** 2
    w = rho * (k / quad) * (math.pi / quad)                  # rho drho dtheta
    flux = (torch.where(r2 < 1.0, inten, torch.zeros_like(inten)) * w[None, :, None]).sum(dim=(1, 2))
    flux[0] = flux[-1] = 0.0                                 # (the contacts: the disks touch)
    if not float(flux.max()) > 0.0:
        raise ValueError("limb_darkened: nothing is occulted at any node")
    return flux / flux.max()


def flare(rise, decay, S=65):
    """A flare: a linear rise to 1 at the fraction `rise` [0, 1) of the width, then exp(-(tau - rise) / decay) to the
    trailing edge (tau in [0, 1] across the width; `decay` > 0 in the same unit).  Divided by the largest node, which
    changes nothing when `rise` falls on a node."""
    S = _nodes(S)
    if not (0.0 <= rise < 1.0 and decay > 0.0):
        raise ValueError("flare needs 0 <= rise < 1 and decay > 0")
    tau = torch.arange(S, dtype=torch.float64) / (S - 1)
    up = tau / rise if rise > 0 else torch.ones_like(tau)
    v = torch.where(tau < rise, up, torch.exp(-(tau - rise) / decay))
    return v / v.max()


def stack(*shapes):
    """(NS, S) bank of (S,) shapes with one node count."""
    if not shapes or any(s.dim() != 1 or s.shape != shapes[0].shape for s in shapes):
        raise ValueError("stack takes one or more (S,) shapes of the same S")
    return torch.stack([s.to(torch.float64) for s in shapes])
