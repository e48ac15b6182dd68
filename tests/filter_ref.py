# -*- coding: utf-8 -*-
"""numpy restatement of the streaming updates (celerite2_amd/csrc/c2_filter.hip, include/celerite2_amd_filter.h): the three
modes of one row body -- append, absorb, forecast -- on the public state layout, and the closed form of the state.  Test
infrastructure only -- nothing here is imported by the package.

A state of one series is the (SW,) vector [t_last, n, sum log d, sum z^2 / d, F (J), S (J x J, row-major)], SW = 4 + J + J^2,
F and S including the last row's own contribution and not yet propagated.  One row (t, a, u, v, y), p = exp(-c (t - t_last))
(p := 0 when n == 0):

    S = (p p^T) o S ;  F = p o F
    g = S u ;  d = a - u^T g ;  w = (v - g) / d ;  z = y - u^T F
    S = S + d w w^T ;  F = F + w z

which is inverse_diag_ref.factor and solve_lower of the whole series, in their op order."""
import numpy as np

from inverse_diag_ref import dense, draw, err, factor, solve_lower  # noqa: F401  (re-exported for the tests)

HEAD = 4


def state_words(J):
    return HEAD + J + J * J


def empty(J):
    return np.zeros(state_words(J))


def unpack(state, J):
    """(t_last, n, sum log d, sum z^2 / d, F (J,), S (J, J)) of a state vector; F and S are copies."""
    return state[0], state[1], state[2], state[3], state[HEAD:HEAD + J].copy(), state[HEAD + J:].reshape(J, J).copy()


def pack(tl, n, ld, q, F, S):
    return np.concatenate([[tl, n, ld, q], F, S.ravel()])


def _decay(c, t, tl, n):
    return np.zeros_like(c) if n == 0 else np.exp(-c * (t - tl))


def append(state, c, t, a, U, V, y):
    """Append the rows -> (new state, d (M,), W (M, J), z (M,), flag).  flag: the 1-based row with d <= 0 (the rows before it
    are filled in, the state returned is the one on entry), else 0."""
    M, J = U.shape
    tl, n, ld, q, F, S = unpack(state, J)
    d, W, z = np.full(M, np.nan), np.full((M, J), np.nan), np.full(M, np.nan)
    for m in range(M):
        p = _decay(c, t[m], tl, n)
        S = np.outer(p, p) * S
        F = p * F
        g = U[m] @ S
        d[m] = a[m] - g @ U[m]
        if d[m] <= 0:
            return state.copy(), d, W, z, m + 1
        W[m] = (V[m] - g) / d[m]
        z[m] = y[m] - U[m] @ F
        S = S + d[m] * np.outer(W[m], W[m])
        F = F + W[m] * z[m]
        tl, n, ld, q = t[m], n + 1, ld + np.log(d[m]), q + z[m] ** 2 / d[m]
    return pack(tl, n, ld, q, F, S), d, W, z, 0


def absorb(state, c, t, W, d, z):
    """The decay and the update line alone, on rows of an existing factorisation."""
    M, J = W.shape
    tl, n, ld, q, F, S = unpack(state, J)
    for m in range(M):
        p = _decay(c, t[m], tl, n)
        S = np.outer(p, p) * S + d[m] * np.outer(W[m], W[m])
        F = p * F + W[m] * z[m]
        tl, n, ld, q = t[m], n + 1, ld + np.log(d[m]), q + z[m] ** 2 / d[m]
    return pack(tl, n, ld, q, F, S)


def forecast(state, c, t, a, U):
    """mu = u^T (p o F), var = a - u^T ((p p^T) o S) u per query row, each from the same state."""
    M, J = U.shape
    tl, n, _, _, F, S = unpack(state, J)
    mu, var = np.empty(M), np.empty(M)
    for m in range(M):
        p = _decay(c, t[m], tl, n)
        mu[m] = U[m] @ (p * F)
        var[m] = a[m] - U[m] @ (np.outer(p, p) * S) @ U[m]
    return mu, var


def closed_form(t, c, W, d, z, n):
    """The state behind row n - 1 (n >= 1 rows absorbed) from the factors of the whole series:
    S = sum_k d_k (e_k o w_k)(e_k o w_k)^T, F = sum_k (e_k o w_k) z_k, e_k = exp(-c (t_{n-1} - t_k))."""
    Wp = W[:n] * np.exp(-c[None, :] * (t[n - 1] - t[:n])[:, None])
    S = np.einsum("nj,nk,n->jk", Wp, Wp, d[:n])
    F = np.einsum("nj,n->j", Wp, z[:n])
    return pack(t[n - 1], n, np.log(d[:n]).sum(), (z[:n] ** 2 / d[:n]).sum(), F, S)


def log_likelihood(state):
    return -0.5 * (state[3] + state[2] + state[1] * np.log(2 * np.pi))


def dense_forecast(K, y, n0):
    """Mean and variance of rows n0 .. N-1 of y ~ N(0, K), each conditioned on rows 0 .. n0-1 alone."""
    sol = np.linalg.solve(K[:n0, :n0], np.column_stack([y[:n0], K[:n0, n0:]]))
    return K[n0:, :n0] @ sol[:, 0], np.diag(K)[n0:] - np.einsum("mn,nm->m", K[n0:, :n0], sol[:, 1:])
