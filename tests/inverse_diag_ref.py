# -*- coding: utf-8 -*-
"""numpy restatement of the inverse-diagonal recurrence (celerite2_amd/csrc/c2_invdiag.hip) and of what it is checked
against: the dense matrix of a set of celerite matrices, its inverse, and delete-one conditioning.  Test infrastructure
only -- nothing here is imported by the package.

Conventions (the reference's forward.hpp factor and solve): L = I + tril(U W^T o decay), K + D = L diag(d) L^T,
p_n = exp(-c (t_{n+1} - t_n)).  Starting from M = 0 behind the last row, for n = N-1 .. 0:

    G = (p_n p_n^T) o M ;  g = G w_n ;  s = w_n^T g ;  q_n = 1/d_n + s
    M = G - u_n g^T - g u_n^T + (s + 1/d_n) u_n u_n^T
"""
import numpy as np


def factor(t, c, a, U, V):
    """forward.hpp:69-135: d (N,), W (N, J)."""
    N, J = U.shape
    d, W = np.empty(N), np.empty((N, J))
    S = np.zeros((J, J))
    d[0] = a[0]
    W[0] = V[0] / d[0]
    for n in range(1, N):
        p = np.exp(-c * (t[n] - t[n - 1]))
        S = np.outer(p, p) * (S + d[n - 1] * np.outer(W[n - 1], W[n - 1]))
        tmp = U[n] @ S
        d[n] = a[n] - tmp @ U[n]
        W[n] = (V[n] - tmp) / d[n]
    return d, W


def solve_lower(t, c, U, W, y):
    """forward.hpp:156-170: z = L^-1 y for one right-hand side."""
    N, J = U.shape
    z = np.array(y, dtype=float)
    F = np.zeros(J)
    for n in range(1, N):
        p = np.exp(-c * (t[n] - t[n - 1]))
        F = p * (F + W[n - 1] * z[n - 1])
        z[n] = y[n] - U[n] @ F
    return z


def inverse_diag(t, c, U, W, d, z=None):
    """q (N,) = diag((K + D)^-1), and with z = L^-1 r also alpha = L^-T (z / d) = (K + D)^-1 r."""
    N, J = U.shape
    q = np.empty(N)
    alpha = None if z is None else np.empty(N)
    M = np.zeros((J, J))
    F = np.zeros(J)
    for n in range(N - 1, -1, -1):
        if n == N - 1:
            G = M
            p = np.ones(J)
        else:
            p = np.exp(-c * (t[n + 1] - t[n]))
            G = np.outer(p, p) * M
        g = G @ W[n]
        s = W[n] @ g
        q[n] = 1.0 / d[n] + s
        M = G - np.outer(U[n], g) - np.outer(g, U[n]) + q[n] * np.outer(U[n], U[n])
        if z is not None:
            if n < N - 1:
                F = p * (F + U[n + 1] * alpha[n + 1])   # forward.hpp:193-207 (internal::backward)
            alpha[n] = z[n] / d[n] - W[n] @ F
    return q if z is None else (q, alpha)


def dense(t, c, a, U, V):
    """diag(a) + tril(U V^T o decay, -1) + its transpose: the matrix the celerite matrices stand for."""
    dt = t[:, None] - t[None, :]
    K = np.einsum("nj,mj,nmj->nm", U, V, np.exp(-c[None, None, :] * np.abs(dt)[:, :, None]))
    K = np.tril(K, -1)
    return K + K.T + np.diag(a)


def draw(seed, N, J, *, gap=False, noise=(0.05, 0.5), t=None):
    """A seeded positive definite draw of width J: J // 2 complex terms a e^{-c tau} cos(d tau) (two columns each) and
    J % 2 real terms a e^{-c tau}; white noise uniform in noise x k(0); on the grid `t` if given (a batch that shares its
    times), else on its own.  Returns a dict with t, c, a, U, V, diag, k0, y."""
    rng = np.random.default_rng(seed)
    own = np.sort(rng.uniform(0.0, 0.1 * N + 1.0, N))
    if gap and N > 2:
        own[N // 2:] += 50.0
    t = own if t is None else t
    Jc, Jr = J // 2, J % 2
    amp = rng.uniform(0.5, 1.5, Jc + Jr) / (Jc + Jr)
    rate = rng.uniform(0.1, 2.0, Jc + Jr)
    freq = rng.uniform(0.5, 3.0, Jc)
    c, U, V = np.empty(J), np.empty((N, J)), np.empty((N, J))
    for k in range(Jr):
        c[k] = rate[k]
        U[:, k] = amp[k]
        V[:, k] = 1.0
    for k in range(Jc):
        i = Jr + 2 * k
        c[i] = c[i + 1] = rate[Jr + k]
        cs, sn = np.cos(freq[k] * t), np.sin(freq[k] * t)
        U[:, i], U[:, i + 1] = amp[Jr + k] * cs, amp[Jr + k] * sn
        V[:, i], V[:, i + 1] = cs, sn
    k0 = float(amp.sum())
    diag = rng.uniform(noise[0], noise[1], N) * k0
    return dict(t=t, c=c, a=k0 + diag, U=U, V=V, diag=diag, k0=k0, y=rng.normal(size=N))


def delete_one(Kfull, y, n):
    """Mean and variance of y_n given every other point, under y ~ N(0, Kfull): row and column n actually deleted."""
    keep = np.arange(Kfull.shape[0]) != n
    if not keep.any():
        return 0.0, Kfull[n, n]
    k = Kfull[keep, n]
    sol = np.linalg.solve(Kfull[np.ix_(keep, keep)], np.stack([y[keep], k], axis=1))
    return float(k @ sol[:, 0]), float(Kfull[n, n] - k @ sol[:, 1])


def err(x, xo, floor=None):
    """Worst violation ratio of the standing criterion |x - xo| <= 1e-10 |xo| + 1e-12 floor (floor: max |xo| unless
    given): <= 1 passes."""
    x, xo = np.asarray(x, dtype=float), np.asarray(xo, dtype=float)
    floor = float(np.max(np.abs(xo))) if floor is None else float(floor)
    return float(np.max(np.abs(x - xo) / (1e-10 * np.abs(xo) + 1e-12 * floor)))


def mean_floor(mu_o, y):
    """Floor of the standing criterion for a predicted mean: max |mu_o| -- except where every reference value is exactly 0
    (one point: leaving it out leaves the prior mean), where the criterion has no scale of its own and the data's is used:
    the mean is formed as y_n minus a correction, so it rounds relative to |y|."""
    m = float(np.max(np.abs(mu_o)))
    return m if m > 0.0 else float(np.max(np.abs(y)))
