# -*- coding: utf-8 -*-
"""numpy restatement of the explained-variance recurrence (celerite2_amd/csrc/c2_predvar.hip) and of what it is checked
against: k(0) - diag(K*^T (K + D)^-1 K*) from dense algebra.  Test infrastructure only -- nothing here is imported by
the package.

Notation as inverse_diag_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay).  A query s has rows u*, v*; n is the
last data row with t_n <= s (ties="data_first") or t_n < s (ties="query_first"), -1 in front of the data.

    forward state   S'_n = (p p^T) o S'_{n-1} + d_n w_n w_n^T,  p = exp(-c (t_n - t_{n-1})),  S'_{-1} = 0
    backward state  R_{n+1}: the M of inverse_diag_ref.inverse_diag after row n + 1,  R_N = 0

    uL = u* o exp(-c (s - t_n)) ;  h = S'_n uL ;  r = uL^T h                                     (0 if n = -1)
    x  = exp(-c (t_{n+1} - s)) o (v* - exp(-c (s - t_n)) o h) ;  r += x^T R_{n+1} x               (0 if n = N - 1)
"""
import numpy as np

from inverse_diag_ref import dense, draw, err, factor  # noqa: F401  (re-exported for the tests)


def _last_row(t, s, ties):
    return int(np.searchsorted(t, s, side="right" if ties == "data_first" else "left")) - 1


def explained_variance(t, ts, c, U, W, d, Us, Vs, ties="data_first"):
    """r (M,) = diag(K*^T (K + D)^-1 K*): two sweeps, nothing stored per data row but the states at the row each query
    follows (the device keeps neither: it merges the grids)."""
    N, J = U.shape
    M = len(ts)
    nq = np.array([_last_row(t, s, ties) for s in ts])
    r = np.zeros(M)
    X = np.array(Vs, dtype=float)
    S = np.zeros((J, J))
    for n in range(N):
        if n > 0:
            p = np.exp(-c * (t[n] - t[n - 1]))
            S = np.outer(p, p) * S
        S = S + d[n] * np.outer(W[n], W[n])
        for m in np.nonzero(nq == n)[0]:
            e = np.exp(-c * (ts[m] - t[n]))
            uL = Us[m] * e
            h = S @ uL
            r[m] = uL @ h
            X[m] = Vs[m] - e * h
    R = np.zeros((J, J))
    for n in range(N - 1, -1, -1):
        if n < N - 1:
            p = np.exp(-c * (t[n + 1] - t[n]))
            G = np.outer(p, p) * R
        else:
            G = R
        g = G @ W[n]
        q = 1.0 / d[n] + W[n] @ g
        R = G - np.outer(U[n], g) - np.outer(g, U[n]) + q * np.outer(U[n], U[n])
        for m in np.nonzero(nq == n - 1)[0]:
            x = np.exp(-c * (t[n] - ts[m])) * X[m]
            r[m] += x @ R @ x
    return r


def cross(t, ts, c, U, V, Us, Vs):
    """K* (N, M): k(t_n - s_m) from the rows of both grids."""
    dt = ts[None, :] - t[:, None]
    e = np.exp(-c[None, None, :] * np.abs(dt)[:, :, None])
    lo = np.einsum("mj,nj,nmj->nm", Us, V, e)    # t_n <= s_m
    hi = np.einsum("nj,mj,nmj->nm", U, Vs, e)    # t_n > s_m
    return np.where(dt >= 0, lo, hi)


def dense_explained(t, ts, c, a, U, V, Us, Vs):
    Ks = cross(t, ts, c, U, V, Us, Vs)
    return np.einsum("nm,nm->m", Ks, np.linalg.solve(dense(t, c, a, U, V), Ks))


def queries(t, rng, M):
    """M sorted query times for the data grid t: t_0, t_{N-1} and t_{N/2} exactly, points before the first and after the
    last data time, several in the widest gap, the rest uniform over the span."""
    N = len(t)
    fixed = [t[0], t[-1], t[N // 2], t[0] - 0.7, t[0] - 0.01, t[-1] + 0.02, t[-1] + 1.3]
    if N > 1:
        k = int(np.argmax(np.diff(t)))
        fixed += list(t[k] + (t[k + 1] - t[k]) * np.array([0.1, 0.5, 0.9]))
    fixed = fixed[:M]
    rest = rng.uniform(t[0] - 0.5, t[-1] + 0.5, M - len(fixed))
    return np.sort(np.concatenate([fixed, rest]))


def draw_with_queries(seed, N, J, M=None, *, gap=False, t=None, ts=None):
    """A seeded draw on the data grid `t` (default: inverse_diag_ref.draw's own for this seed) and consistent U*, V* on the
    query grid `ts` (default: queries(t, ., M)): ONE draw on the concatenated grid [t, ts], rows split.  Returns draw's dict
    for the data rows, with ts, Us, Vs added."""
    if t is None:
        t = draw(seed, N, J, gap=gap)["t"]
    if ts is None:
        ts = queries(t, np.random.default_rng(seed + 7919), M)
    full = draw(seed, N + len(ts), J, t=np.concatenate([t, ts]))
    out = {k: (v[:N] if k in ("a", "U", "V", "diag", "y") else v) for k, v in full.items()}
    out["t"], out["ts"], out["Us"], out["Vs"] = t, ts, full["U"][N:], full["V"][N:]
    return out
