# -*- coding: utf-8 -*-
"""numpy restatement of the projections on trial columns (celerite2_amd/csrc/c2_trial_project.hip) and of what they and the
many-series finish (celerite2_amd/significance.py) are checked against: dense algebra on the matrix the celerite matrices
stand for and two dense generalized-least-squares fits per trial and draw.  Test infrastructure only -- nothing here is
imported by the package.

The columns are the existing restatements', imported and not edited: periodogram_ref.columns, transit_ref.template,
kepler_ref.columns (each the kernel's rule, statement by statement).  The contraction with alpha is in np.longdouble, so the
reference's own rounding stays far below the criterion.

Notation as linear_model_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay), <a, b> = sum_n a_n b_n / d_n.  A draw from
the null is y_r = L D^1/2 n_r (mean 0 here), and

    s_yy_r = |n_r|^2,   g0y_r = Z_A0^T D^-1/2 n_r,   alpha_r = (K + D)^-1 y_r = L^-T D^-1/2 n_r,   gty_r[k] = col_k^T alpha_r.
"""
import numpy as np

import kepler_ref as KR
import periodogram_ref as PR
import transit_ref as TR
from linear_model_ref import dense, err  # noqa: F401  (re-exported for the tests)

KINDS = ("periodogram", "transit", "keplerian")
WORDS = {"periodogram": 1, "transit": 4, "keplerian": 3}
NCOL = {"periodogram": 2, "transit": 1, "keplerian": 2}
REF = {"periodogram": PR, "transit": TR, "keplerian": KR}
TRIALS_KEY = {"periodogram": "freq", "transit": "trials", "keplerian": "trials"}


def columns(kind, t, trials, t_ref=0.0):
    """(C, N, K): the trial columns as the kernel forms them, for one series t (N,)."""
    with np.errstate(all="ignore"):
        if kind == "periodogram":
            return np.stack(PR.columns(t, trials, t_ref))
        if kind == "transit":
            return TR.template(t, trials)[None]
        return np.stack(KR.columns(t, trials))


def projections(kind, t, alpha, trials, t_ref=0.0):
    """P (K, C, R) = sum_n col_c(trial k; t_n) alpha[n, r] for one series: t (N,), alpha (N, R).  The sum in np.longdouble."""
    col = columns(kind, t, trials, t_ref).astype(np.longdouble)              # (C, N, K)
    with np.errstate(all="ignore"):
        return np.einsum("cnk,nr->kcr", col, alpha.astype(np.longdouble)).astype(float)


def projections_batched(kind, t, alpha, trials, t_ref=0.0):
    """(B, K, C, R) for alpha (B, N, R); t (N,) | (B, N) and trials shared or per series."""
    B = alpha.shape[0]
    per = trials.ndim == (2 if kind == "periodogram" else 3)
    return np.stack([projections(kind, t[b] if t.ndim == 2 else t, alpha[b], trials[b] if per else trials, t_ref) for b in range(B)])


def lower(t, c, U, W):
    """L (N, N) = I + tril(U W^T o decay, -1), dense."""
    dt = t[:, None] - t[None, :]
    L = np.einsum("nj,mj,nmj->nm", U, W, np.exp(-c[None, None, :] * np.abs(dt)[:, :, None]))
    return np.tril(L, -1) + np.eye(len(t))


def null_draws(D, normals):
    """For the case D (a dict of a *_ref.case) and normals (N, R): the draws y (N, R) = L D^1/2 n formed densely, and what
    the fused route feeds null_statistics -- s_yy (R,), G0Y (P0, R), alpha (N, R) = L^-T D^-1/2 n by a dense solve."""
    L = lower(D["t"], D["c"], D["U"], D["W"])
    y = L @ (np.sqrt(D["d"])[:, None] * normals)
    scaled = normals / np.sqrt(D["d"])[:, None]
    P0 = D["A0"].shape[1]
    return y, (normals * normals).sum(0), D["Z0"][:, :P0].T @ scaled, np.linalg.solve(L.T, scaled)


def sweep_products(kind, D, t_ref=0.0):
    """T of the observed series by the kind's restated sweep."""
    args = [D[x] for x in ("t", "c", "U", "W", "d", "Z0")]
    with np.errstate(all="ignore"):
        if kind == "periodogram":
            return PR.whitened_sinusoids(*args, D["freq"], t_ref)
        return REF[kind].whitened_transits(*args, D["trials"]) if kind == "transit" else KR.whitened_keplerians(*args, D["trials"])


def dense_statistics(kind, D, y, t_ref=0.0):
    """(dchi2 (K, R), chi2_0 (R,), sign (K, R)) by two dense generalized-least-squares fits per trial and draw of y (N, R),
    sharing no formula with the package; sign: of the fitted depth (transit), else zeros."""
    Kd = dense(D["t"], D["c"], D["a"], D["U"], D["V"])
    out, nul, sgn = [], [], []
    for r in range(y.shape[1]):
        if kind == "periodogram":
            dchi2, _, chi2_0 = PR.dense_periodogram(Kd, D["t"], D["A0"], y[:, r], D["freq"], t_ref)
            s = np.zeros_like(dchi2)
        elif kind == "transit":
            dchi2, depth, _, chi2_0 = TR.dense_search(Kd, D["t"], D["A0"], y[:, r], D["trials"])
            s = np.sign(depth)
        else:
            dchi2, _, chi2_0 = KR.dense_keplerian(Kd, D["t"], D["A0"], y[:, r], D["trials"])
            s = np.zeros_like(dchi2)
        out.append(dchi2); nul.append(chi2_0); sgn.append(s)
    return np.stack(out, axis=1), np.array(nul), np.stack(sgn, axis=1)


def normalized(dchi2, chi2_0, normalization):
    return {"standard": dchi2 / chi2_0, "chi2": dchi2, "log_likelihood": 0.5 * dchi2}[normalization]


def case(kind, seed, N, J, P0=1, K=12):
    """The kind's own seeded case (periodogram_ref.case, transit_ref.case, kepler_ref.case) with K trials."""
    if kind == "periodogram":
        return PR.case(seed, N, J, P0, F=K)
    return TR.case(seed, N, J, P0, K=K) if kind == "transit" else KR.case(seed, N, J, P0, K=K, e_max=0.9)
