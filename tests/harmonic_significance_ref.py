# -*- coding: utf-8 -*-
"""numpy restatement of the projections on the 2 H columns of a multi-harmonic grid and of the statistic finished from them
(celerite2_amd/csrc/c2_harmonic_trials.hip), and what they and harmonics.null_statistics are checked against: dense algebra
on the matrix the celerite matrices stand for and two dense generalized-least-squares fits per frequency and draw.  Test
infrastructure only -- nothing here is imported by the package.

The columns are harmonics_ref.columns (the kernel's rule, statement by statement), imported and not edited; the draws and
their products are trial_projections_ref.null_draws.  The contraction with alpha is in np.longdouble, so the reference's own
rounding stays far below the criterion.

    P[f, i, r] = sum_n col_i(f; t_n) alpha[n, r]                               (i over c_1, s_1, ..., c_H, s_H)
    r_i = P_i - sum_p X[p, i] v[p],   w_i = (r_i - sum_{k<i} L_ik w_k) / L_ii,   dchi2 = sum_i w_i^2
"""
import numpy as np

import harmonics_ref as HR
from trial_projections_ref import dense, err, lower, null_draws, normalized  # noqa: F401  (re-exported for the tests)


def projections(t, alpha, freq, H, t_ref=0.0):
    """P (F, 2 H, R) for one series: t (N,), alpha (N, R).  The sum in np.longdouble."""
    col = HR.columns(t, freq, H, t_ref).astype(np.longdouble)               # (NC, N, F)
    with np.errstate(all="ignore"):
        return np.einsum("cnk,nr->kcr", col, alpha.astype(np.longdouble)).astype(float)


def projections_batched(t, alpha, freq, H, t_ref=0.0):
    """(B, F, 2 H, R) for alpha (B, N, R); t (N,) | (B, N) and freq (F,) | (B, F)."""
    B = alpha.shape[0]
    return np.stack([projections(t[b] if t.ndim == 2 else t, alpha[b], freq[b] if freq.ndim == 2 else freq, H, t_ref)
                     for b in range(B)])


def null_chi2(P, Lm, Xt, V):
    """D (F, R): the kernel's lines for one series from P (F, 2 H, R), the packed factor Lm (F, H (2 H + 1)) (row-major lower
    triangle), Xt (F, 2 H, P0) and V (P0, R); Xt, V None when P0 = 0."""
    F, NC, R = P.shape
    w = np.zeros((NC, F, R))
    D = np.zeros((F, R))
    with np.errstate(all="ignore"):
        for i in range(NC):
            r = P[:, i].copy()
            if Xt is not None and Xt.shape[-1]:
                r = r - np.einsum("fp,pr->fr", Xt[:, i], V)
            for k in range(i):
                r = r - Lm[:, i * (i + 1) // 2 + k, None] * w[k]
            w[i] = r / Lm[:, i * (i + 1) // 2 + i, None]
            D += w[i] * w[i]
    return D


def dense_statistics(D, y, H, t_ref=0.0):
    """(dchi2 (F, R), chi2_0 (R,)) by two dense generalized-least-squares fits per frequency and draw of y (N, R), sharing no
    formula with the package (harmonics_ref.dense_harmonics)."""
    Kd = dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    out, nul = [], []
    for r in range(y.shape[1]):
        dchi2, _, chi2_0 = HR.dense_harmonics(Kd, D["t"], D["A0"], y[:, r], D["freq"], H, t_ref)
        out.append(dchi2)
        nul.append(chi2_0)
    return np.stack(out, axis=1), np.array(nul)


def safe_grid(t, F, H, lo=1.1):
    """F angular frequencies from `lo` cycles over the baseline up to where the H-th harmonic has 0.45 N cycles over it (at
    most 5.7), irrational in the baseline: away from 0 and, the highest harmonic staying below half the mean sampling rate,
    away from the aliases of an even grid, so that M is well conditioned."""
    span = float(np.max(t) - np.min(t))
    hi = max(min(5.7, 0.45 * len(t) / H), lo + 0.4)
    return 2.0 * np.pi / span * (np.linspace(lo, hi, F) + 0.1 * np.sqrt(2.0) * np.arange(F) / F)


def case(seed, N, J, P0, F, H):
    """harmonics_ref.case (a seeded series with its factors, A0, Z0) on the grid `safe_grid`."""
    D = HR.case(seed, N, J, P0, F=F)
    D["freq"] = safe_grid(D["t"], F, H)
    return D
