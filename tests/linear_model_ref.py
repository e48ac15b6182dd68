# -*- coding: utf-8 -*-
"""numpy restatement of the whitened Gram sweep (celerite2_amd/csrc/c2_gram.hip), of the composed reverse rule that
autograd.whitened_gram uses, and of what both are checked against: dense generalized least squares.  Test infrastructure
only -- nothing here is imported by the package.  Every function takes real or complex arrays (complex-step derivatives).

Notation as inverse_diag_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay).  With Y = [A | y] (N, Q):

    F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x Q, zero at row 0; p_n = exp(-c (t_n - t_{n-1})))
    z_n = y_n - F^T u_n
    S  += z_n z_n^T / d_n                   ->   S = Y^T (K + D)^-1 Y
"""
import math

import numpy as np

from inverse_diag_ref import dense, draw, err, factor  # noqa: F401  (re-exported for the tests)


def design(t, P):
    """(N, P): the powers 0 .. P-1 of the centred, range-scaled times (|x| <= 1/2 + the offset of the mean)."""
    span = float(np.max(t) - np.min(t))
    x = (t - np.mean(t)) / (span if span > 0 else 1.0)
    return x[:, None] ** np.arange(P)[None, :]


def sweep(t, c, U, W, Y):
    """internal::forward with Q columns: Z = L^-1 Y (N, Q) and G (N, J, Q), the state of row n BEFORE its decay,
    G_n = F_{n-1} + w_{n-1} z_{n-1}^T (zeros at row 0) -- what the reverse below reads."""
    N, J = U.shape
    dt = np.result_type(t, c, U, W, Y)
    Z, G = np.array(Y, dtype=dt), np.zeros((N, J, Y.shape[1]), dtype=dt)
    F = np.zeros((J, Y.shape[1]), dtype=dt)
    for n in range(1, N):
        p = np.exp(-c * (t[n] - t[n - 1]))
        G[n] = F + np.outer(W[n - 1], Z[n - 1])
        F = p[:, None] * G[n]
        Z[n] = Y[n] - U[n] @ F
    return Z, G


def whitened_gram_rows(t, c, U, W, d, Y):
    """The plain recurrence, row by row: S (Q, Q)."""
    Z, _ = sweep(t, c, U, W, Y)
    S = np.zeros((Y.shape[1],) * 2, dtype=Z.dtype)
    for n in range(len(d)):
        S = S + np.outer(Z[n], Z[n]) / d[n]
    return S


def whitened_gram(t, c, U, W, d, Y):
    """The sweep in the kernel's order (k_gram): one state, nothing stored per row; row 0 takes the general step with p = 1
    and w_{-1} z_{-1} = 0; F^T u_n in four interleaved partial sums; (z_i z_k) rounded before it is scaled by a reciprocal
    of d_n.  The 16-row blocks of t, d, y and the look-ahead ring of U, W, A rows move data only, so rows are visited
    0 .. N-1 whatever the block length."""
    N, J = U.shape
    Q = Y.shape[1]
    F, S = np.zeros((J, Q)), np.zeros((Q, Q))
    wprev, zprev, tprev = np.zeros(J), np.zeros(Q), t[0]
    for n in range(N):
        p = np.exp(c * (tprev - t[n]))
        tprev = t[n]
        F = p[:, None] * (F + np.outer(wprev, zprev))
        acc = np.zeros((4, Q))
        for j in range(J):
            acc[j & 3] += F[j] * U[n, j]
        z = Y[n] - ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        S += np.outer(z, z) * (1.0 / d[n])
        wprev, zprev = W[n], z
    return S


def whitened_gram_batched(t, c, U, W, d, Y):
    """`whitened_gram` for a whole batch at once: t (B, N), c (B, J), U, W (B, N, J), d (B, N), Y (B, N, Q) -> (B, Q, Q).
    The same statements with a leading axis (F^T u_n in one sum: the order inside a row is below the criterion)."""
    B, N, J = U.shape
    Q = Y.shape[2]
    F, S = np.zeros((B, J, Q)), np.zeros((B, Q, Q))
    wprev, zprev, tprev = np.zeros((B, J)), np.zeros((B, Q)), t[:, 0]
    for n in range(N):
        p = np.exp(c * (tprev - t[:, n])[:, None])
        tprev = t[:, n]
        F = p[:, :, None] * (F + wprev[:, :, None] * zprev[:, None, :])
        z = Y[:, n] - np.einsum("bjq,bj->bq", F, U[:, n])
        S += (z[:, :, None] * z[:, None, :]) * (1.0 / d[:, n])[:, None, None]
        wprev, zprev = W[:, n], z
    return S


def sweep_rev(t, c, U, W, Y, Z, G, bZ):
    """Reverse of `sweep`: (bt (N,), bc (J,), bU (N, J), bW (N, J), bY (N, Q)) from the cotangent bZ (N, Q)."""
    N, J = U.shape
    dt = np.result_type(Z, bZ)
    bt, bc, bU, bW = np.zeros(N, dtype=dt), np.zeros(J, dtype=dt), np.zeros((N, J), dtype=dt), np.zeros((N, J), dtype=dt)
    bz = np.array(bZ, dtype=dt)
    bF = np.zeros((J, Y.shape[1]), dtype=dt)
    for n in range(N - 1, 0, -1):
        p = np.exp(-c * (t[n] - t[n - 1]))
        F = p[:, None] * G[n]
        bU[n] = -F @ bz[n]
        bF = bF - np.outer(U[n], bz[n])
        bp = (bF * G[n]).sum(axis=1) * p          # d/d(log p)
        bc -= bp * (t[n] - t[n - 1])
        bt[n] -= bp @ c
        bt[n - 1] += bp @ c
        bF = p[:, None] * bF                      # cotangent of G_n = F_{n-1} + w_{n-1} z_{n-1}^T
        bW[n - 1] = bF @ Z[n - 1]
        bz[n - 1] = bz[n - 1] + W[n - 1] @ bF
    return bt, bc, bU, bW, bz


def whitened_gram_rev(t, c, U, W, d, Y, bS):
    """The composed backward rule of autograd.whitened_gram: Z recomputed, bZ = Z (bS + bS^T) / d,
    bd_n = -(z_n^T bS z_n) / d_n^2, then the reverse of the sweep.  Returns (bt, bc, bU, bW, bd, bY)."""
    Z, G = sweep(t, c, U, W, Y)
    bZ = Z @ (bS + bS.T) / d[:, None]
    bd = -np.einsum("nq,qr,nr->n", Z, bS, Z) / d ** 2
    bt, bc, bU, bW, bY = sweep_rev(t, c, U, W, Y, Z, G, bZ)
    return bt, bc, bU, bW, bd, bY


def case(seed, N, J, Q, with_y=True):
    """One series: draw's dict with d, W (its factors), A (N, P) = design, Y = [A | y] (N, Q); P = Q - 1 with y, Q without."""
    D = draw(seed, N, J)
    D["d"], D["W"] = factor(D["t"], D["c"], D["a"], D["U"], D["V"])
    P = Q - 1 if with_y else Q
    D["A"] = design(D["t"], P)
    D["Y"] = np.concatenate([D["A"], D["y"][:, None]], axis=1) if with_y else D["A"]
    return D


# ---- dense generalized least squares ------------------------------------------------------------------------------------
def log_normal(r, C):
    """log N(r | 0, C)."""
    sign, logdet = np.linalg.slogdet(C)
    assert sign > 0
    return -0.5 * (r @ np.linalg.solve(C, r)) - 0.5 * logdet - 0.5 * len(r) * math.log(2.0 * math.pi)


def dense_gls(K, A, y, mu0=None, Lam=None, eps=1e-7):
    """beta, cov, the log-likelihood at beta and the marginal one, from dense algebra that shares no formula with the
    package: beta and cov from the normal equations in K^-1, the likelihood at beta as log N(y - A beta | 0, K) (plus the
    prior's quadratic term at beta), the Gaussian-prior marginal as log N(y | A mu0, K + A Lam^-1 A^T).  The flat-prior
    marginal is returned twice, as (sharp, (limit, bound)):
      sharp: the density of the data projected on the null space of A^T, which does not depend on beta, with the Jacobian
             of the projection: log N(N^T y | 0, N^T K N) - logdet(A^T A) / 2, N an orthonormal basis of null(A^T);
      limit: Lam = eps I in the Gaussian-prior form with the divergence logdet(Lam) / 2 - P log(2 pi) / 2 removed,
             log N(y | 0, K + A A^T / eps) - (P / 2) log eps + (P / 2) log(2 pi).  It lies eps (tr(cov) + |beta|^2) / 2
             below the flat value to first order, and its matrix C has condition ~ |A|^2 / (eps lambda_min(K)), so
             bound = eps (tr(cov) + |beta|^2) + N 2.2e-16 cond(C) max(1, |value|): twice the bias plus the solve's rounding."""
    N, P = A.shape
    Ki = np.linalg.inv(K)
    mu0 = np.zeros(P) if mu0 is None else mu0
    H = A.T @ Ki @ A + (0.0 if Lam is None else Lam)
    cov = np.linalg.inv(H)
    beta = mu0 + cov @ (A.T @ Ki @ (y - A @ mu0))
    ll = log_normal(y - A @ beta, K)
    if Lam is None:
        Qf, _ = np.linalg.qr(A, mode="complete")
        Nn = Qf[:, P:]
        sharp = (log_normal(Nn.T @ y, Nn.T @ K @ Nn) if N > P else 0.0) - 0.5 * np.linalg.slogdet(A.T @ A)[1]
        C = K + A @ A.T / eps
        limit = log_normal(y, C) - 0.5 * P * math.log(eps) + 0.5 * P * math.log(2.0 * math.pi)
        bound = eps * (np.trace(cov) + beta @ beta) + N * 2.2e-16 * np.linalg.cond(C) * max(1.0, abs(limit))
        mll = (sharp, (limit, bound))
    else:
        ll = ll - 0.5 * (beta - mu0) @ Lam @ (beta - mu0)
        mll = log_normal(y - A @ mu0, K + A @ np.linalg.solve(Lam, A.T))
    return beta, cov, ll, mll


# ---- the same in torch (float64, CPU), differentiable --------------------------------------------------------------------
def torch_factor(t, c, a, U, V):
    """inverse_diag_ref.factor in torch: the link between the closed form's (a, V) and the sweep's (d, W)."""
    import torch
    S = torch.zeros((U.shape[1],) * 2, dtype=torch.float64)
    d, W = [a[0]], [V[0] / a[0]]
    for n in range(1, U.shape[0]):
        p = torch.exp(-c * (t[n] - t[n - 1]))
        S = torch.outer(p, p) * (S + d[-1] * torch.outer(W[-1], W[-1]))
        tmp = U[n] @ S
        d.append(a[n] - tmp @ U[n])
        W.append((V[n] - tmp) / d[-1])
    return torch.stack(d), torch.stack(W)


def torch_dense(t, c, a, U, V):
    """inverse_diag_ref.dense in torch; the lag is taken signed under the mask (abs has derivative 0 on the diagonal)."""
    import torch
    N = t.shape[0]
    low = torch.tril(torch.ones(N, N, dtype=torch.bool), -1)
    dt = torch.where(low, t[:, None] - t[None, :], torch.zeros(N, N, dtype=torch.float64))
    K = torch.einsum("nj,mj,nmj->nm", U, V, torch.exp(-c[None, None, :] * dt[:, :, None]))
    K = torch.where(low, K, torch.zeros_like(K))
    return K + K.T + torch.diag(a)


def torch_log_normal(r, C):
    import torch
    return -0.5 * (r @ torch.linalg.solve(C, r)) - 0.5 * torch.linalg.slogdet(C)[1] - 0.5 * r.shape[0] * math.log(2.0 * math.pi)


def torch_objective(K, A, y, mu0=None, Lam=None, profiled=False):
    """The dense objective of one series: the Gaussian-prior marginal as log N(y | A mu0, K + A Lam^-1 A^T); the flat-prior
    one as the likelihood at the dense GLS beta - logdet(A^T K^-1 A) / 2 + P log(2 pi) / 2 (pinned to the limit of the
    former by tests/test_linear_model.py); profiled: the likelihood at beta (with the prior's quadratic term)."""
    import torch
    P = A.shape[1]
    r = y if mu0 is None else y - A @ mu0
    KiA = torch.linalg.solve(K, A)
    H = A.T @ KiA + (0.0 if Lam is None else Lam)
    delta = torch.linalg.solve(H, KiA.T @ r)
    ll = torch_log_normal(r - A @ delta, K)
    if Lam is not None:
        ll = ll - 0.5 * delta @ Lam @ delta
    if profiled:
        return ll
    if Lam is None:
        return ll - 0.5 * torch.linalg.slogdet(H)[1] + 0.5 * P * math.log(2.0 * math.pi)
    return torch_log_normal(r, K + A @ torch.linalg.solve(Lam, A.T))
