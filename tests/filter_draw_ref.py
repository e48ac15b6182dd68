# -*- coding: utf-8 -*-
"""numpy restatement of the forecast sample paths (celerite2_amd/csrc/c2_filter_draw.hip,
include/celerite2_amd_filter_draw.h) on filter_ref's helpers: the append run backwards in y.  Test infrastructure only --
nothing here is imported by the package.

Per row, after the decay (p := 0 when n == 0),

    g = S u ;  d = a - u^T g ;  w = (v - g) / d                       (as filter_ref.append: no y in them)
    z_k = sqrt(d) eps_k ;  y_k = u^T F_k + z_k ;  F_k = F_k + w z_k   (per draw k)
    S = S + d w w^T

so S, d and w are shared by the K draws and only F is per draw: paths = mu_c + L_c D_c^(1/2) eps = mu_c + chol(Sigma_c) eps for
the dense conditional mean and covariance of the M rows given every absorbed row."""
import numpy as np

from filter_ref import _decay, unpack


def draw_paths(state, c, t, a, U, V, eps):
    """state (SW,), c (J,), t, a (M,), U, V (M, J), eps (M, K) -> (paths (M, K), d (M,), flag).  flag: the 1-based row with
    d <= 0 (the rows of paths and d before it are filled in, the failing row's d, NaN behind), else 0."""
    M, J = U.shape
    K = eps.shape[1]
    tl, n, _, _, F, S = unpack(state, J)
    Fk = np.repeat(F[:, None], K, axis=1)   # (J, K)
    paths, d = np.full((M, K), np.nan), np.full(M, np.nan)
    for m in range(M):
        p = _decay(c, t[m], tl, n)
        S = np.outer(p, p) * S
        Fk = p[:, None] * Fk
        g = U[m] @ S
        d[m] = a[m] - g @ U[m]
        if d[m] <= 0:
            return paths, d, m + 1
        w = (V[m] - g) / d[m]
        z = np.sqrt(d[m]) * eps[m]
        paths[m] = U[m] @ Fk + z
        Fk = Fk + np.outer(w, z)
        S = S + d[m] * np.outer(w, w)
        tl, n = t[m], n + 1
    return paths, d, 0


def dense_conditional(K, y, n0):
    """Mean (M,) and covariance (M, M) of rows n0 .. N-1 of y ~ N(0, K) given rows 0 .. n0-1 (the prior for n0 == 0)."""
    if n0 == 0:
        return np.zeros(K.shape[0]), K.copy()
    sol = np.linalg.solve(K[:n0, :n0], np.column_stack([y[:n0], K[:n0, n0:]]))
    Sig = K[n0:, n0:] - K[n0:, :n0] @ sol[:, 1:]
    return K[n0:, :n0] @ sol[:, 0], 0.5 * (Sig + Sig.T)


def joint_log_density(d, z):
    """-(1/2) sum (z^2 / d + log d + log 2 pi) over the rows of an append: the joint log density of those rows."""
    return -0.5 * np.sum(z ** 2 / d + np.log(d) + np.log(2 * np.pi))
