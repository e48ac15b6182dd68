# -*- coding: utf-8 -*-
"""oracle/exact.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Exact references for every gradient the project computes, in plain numpy float64, independent of the CPU restatement
(oracle/c2_oracle.cpp) and of its reverse passes:

  * closed forms on the dense matrix.  With K the covariance, alpha = K^-1 y and G = (alpha alpha^T - K^-1) / 2, the
    log-likelihood's derivative w.r.t. any parameter theta is sum_nm G_nm dK_nm / dtheta.  The semiseparable entries
    K_nm = sum_j U_nj V_mj exp(-c_j (t_n - t_m)), n > m, give the matrix-level gradients (t, c, a, U, V, y); the kernel
    k(tau) of the celerite terms gives the coefficient-level ones; K = T (x) alpha alpha^T + diag the Kronecker ones.
    The sweeps (solve / matmul, lower / upper) have vector-Jacobian products on the dense operator L = I + M,
    M = strict-lower(U W^T o E), whose matrix cotangent goes through the same (t, c, U, W) contraction.
  * complex-step differentiation (h = 1e-30) of analytic forwards -- the dense log-likelihood (|tau| written by index
    order, K^-1 y by LU, log det by slogdet) and the O(N) recursions (factor, forward solve, the four sweeps) -- for
    exactness independent of any hand derivation.  Every forward broadcasts over leading axes, so many perturbations run
    in one call.

Times are taken sorted; a tie (dt = 0) takes the derivative of the later row as the later one, which is what the
semiseparable form (and every kernel) computes.
"""
import numpy as np

from . import dense

__all__ = [
    "H", "dense_from_semiseparable", "loglik_G", "contract_lower", "loglik_grad", "loglik_grad_from_K",
    "terms_dense", "terms_grad", "kron_grad", "sweep_vjp", "dense_loglik_fwd", "terms_loglik_fwd", "factor_fwd",
    "recursive_loglik_fwd", "sweep_fwd", "cstep_grad", "cstep_jvp", "relerr",
]

H = 1e-30
LOG2PI = np.log(2.0 * np.pi)


def relerr(x, e):
    """max |x - e| / max |e| (1.0 for an all-zero e)."""
    x, e = np.asarray(x), np.asarray(e)
    if e.size == 0:
        return 0.0
    return float(np.max(np.abs(x - e)) / max(float(np.max(np.abs(e))), 1e-300))


def _low(N):
    return np.tril(np.ones((N, N), dtype=bool), -1)


# ---- closed forms -----------------------------------------------------------------------------------------------
def dense_from_semiseparable(t, c, a, U, V):
    """K with K_nn = a_n, K_nm = K_mn = sum_j U_nj V_mj exp(-c_j (t_n - t_m)) for n > m."""
    N, J = U.shape
    low = _low(N)
    dtl = np.where(low, t[:, None] - t[None, :], 0.0)
    Kl = np.zeros((N, N))
    for j in range(J):
        Kl += np.outer(U[:, j], V[:, j]) * np.exp(-c[j] * dtl)
    Kl = np.where(low, Kl, 0.0)
    return Kl + Kl.T + np.diag(a)


def loglik_G(K, y):
    """ll, G = (alpha alpha^T - K^-1) / 2, alpha = K^-1 y (y: (N,)), by Cholesky."""
    N = len(y)
    L = np.linalg.cholesky(K)
    Li = np.linalg.inv(L)
    Kinv = Li.T @ Li
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = Kinv @ y
    ll = -0.5 * float(y @ alpha) - float(np.sum(np.log(np.diag(L)))) - 0.5 * N * LOG2PI
    return ll, 0.5 * (np.outer(alpha, alpha) - Kinv), alpha


def contract_lower(P, t, c, U, W):
    """Cotangent P on the strict-lower entries M_nm = sum_j U_nj W_mj exp(-c_j (t_n - t_m)) (n > m; the rest of P is
    ignored) pushed to (bt, bc, bU, bW)."""
    N, J = U.shape
    low = _low(N)
    dtl = np.where(low, t[:, None] - t[None, :], 0.0)
    Pl = np.where(low, P, 0.0)
    bt = np.zeros(N); bc = np.zeros(J); bU = np.zeros((N, J)); bW = np.zeros((N, J))
    for j in range(J):
        A = Pl * np.exp(-c[j] * dtl)
        bU[:, j] = A @ W[:, j]
        bW[:, j] = A.T @ U[:, j]
        T = A * U[:, j][:, None] * W[:, j][None, :]
        bc[j] = -np.sum(T * dtl)
        bt -= c[j] * (T.sum(1) - T.sum(0))
    return bt, bc, bU, bW


def loglik_grad_from_K(K, y, t, c, U, V):
    """Gradient w.r.t. (t, c, a, U, V, y) with G taken from the given dense K (e.g. the reference's own K)."""
    ll, G, alpha = loglik_G(K, y)
    bt, bc, bU, bV = contract_lower(2.0 * G, t, c, U, V)
    return ll, (bt, bc, np.diag(G).copy(), bU, bV, -alpha)


def loglik_grad(t, c, a, U, V, y):
    """Exact log-likelihood and (bt, bc, ba, bU, bV, by) of ONE series from its dense semiseparable matrix."""
    return loglik_grad_from_K(dense_from_semiseparable(t, c, a, U, V), y, t, c, U, V)


def _tau_lower(x):
    """tau_nm = x_n - x_m by index order (n > m), mirrored; 0 on the diagonal; sign +1 below, -1 above."""
    N = len(x)
    low = _low(N)
    tl = np.where(low, x[:, None] - x[None, :], 0.0)
    return tl + tl.T, low.astype(np.float64) - low.T.astype(np.float64)


def terms_dense(ar, cr, ac, bc, cc, dc, x, diag):
    tau, _ = _tau_lower(x)
    K = dense.kernel_value(dense.Coeffs(ar, cr, ac, bc, cc, dc), tau)
    return K + np.diag(diag)


def terms_grad(ar, cr, ac, bc, cc, dc, x, diag, y):
    """Exact log-likelihood and (bar, bcr, bac, bbc, bcc, bdc, bx, bdiag, by) of ONE series from the dense kernel matrix
    of the celerite coefficients."""
    ar, cr, ac, bc, cc, dc = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (ar, cr, ac, bc, cc, dc))
    tau, sgn = _tau_lower(x)
    ll, G, alpha = loglik_G(terms_dense(ar, cr, ac, bc, cc, dc, x, diag), y)
    kp = np.zeros_like(tau)
    bar = np.empty(len(ar)); bcr = np.empty(len(ar))
    for j in range(len(ar)):
        e = np.exp(-cr[j] * tau)
        bar[j] = np.sum(G * e)
        bcr[j] = -ar[j] * np.sum(G * tau * e)
        kp -= cr[j] * ar[j] * e
    n = len(ac)
    bac, bbc, bcc, bdc = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    for j in range(n):
        e = np.exp(-cc[j] * tau)
        cs, sn = np.cos(dc[j] * tau), np.sin(dc[j] * tau)
        val = ac[j] * cs + bc[j] * sn
        der = -ac[j] * sn + bc[j] * cs
        bac[j] = np.sum(G * e * cs)
        bbc[j] = np.sum(G * e * sn)
        bcc[j] = -np.sum(G * tau * e * val)
        bdc[j] = np.sum(G * tau * e * der)
        kp += e * (dc[j] * der - cc[j] * val)
    bx = 2.0 * np.sum(G * kp * sgn, axis=1)
    return ll, (bar, bcr, bac, bbc, bcc, bdc, bx, np.diag(G).copy(), -alpha)


def kron_grad(t, c, a, U, V, alpha, diag, y):
    """Exact ll and (bt, bc, ba, bU, bV, balpha, bdiag, by) of ONE series of the 2-D model K = T (x) alpha alpha^T +
    diag (oracle/dense.py: kron_dense; T_nn = a_n, rows epoch-major).  (ba, bU, bV) are the partials with a, U, V
    independent (the collapsed parametrisation)."""
    N, J = U.shape
    M = len(alpha)
    T = dense_from_semiseparable(t, c, a, U, V)
    K = np.kron(T, np.outer(alpha, alpha)) + np.diag(np.asarray(diag).ravel())
    ll, G, al = loglik_G(K, np.asarray(y).ravel())
    G4 = G.reshape(N, M, N, M)
    GT = np.einsum("nmkl,m,l->nk", G4, alpha, alpha)
    bt, bc, bU, bV = contract_lower(2.0 * GT, t, c, U, V)
    balpha = 2.0 * np.einsum("nk,nmkl,l->m", T, G4, alpha)
    bdiag = np.einsum("nmnm->nm", G4).copy()
    return ll, (bt, bc, np.diag(GT).copy(), bU, bV, balpha, bdiag, -al.reshape(N, M))


def sweep_vjp(name, t, c, U, W, Y, bZ):
    """Dense forward Z and exact cotangents (bt, bc, bU, bW, bY) of a sweep, Y / bZ (N, nrhs):
    solve_lower Z = L^-1 Y, solve_upper Z = L^-T Y, matmul_lower Z = M Y, matmul_upper Z = M^T Y."""
    N = len(t)
    M = dense_from_semiseparable(t, c, np.zeros(N), U, W)
    M = np.tril(M, -1)
    L = np.eye(N) + M
    if name == "solve_lower":
        Z = np.linalg.solve(L, Y); bY = np.linalg.solve(L.T, bZ); P = -bY @ Z.T
    elif name == "solve_upper":
        Z = np.linalg.solve(L.T, Y); bY = np.linalg.solve(L, bZ); P = -Z @ bY.T
    elif name == "matmul_lower":
        Z = M @ Y; bY = M.T @ bZ; P = bZ @ Y.T
    elif name == "matmul_upper":
        Z = M.T @ Y; bY = M @ bZ; P = Y @ bZ.T
    else:
        raise ValueError(name)
    bt, bc, bU, bW = contract_lower(P, t, c, U, W)
    return Z, (bt, bc, bU, bW, bY)


# ---- analytic forwards (complex-step) ----------------------------------------------------------------------------
def dense_loglik_fwd(t, c, a, U, V, y):
    """Dense log-likelihood of (t, c, a, U, V, y) over any leading axes, analytic in every argument."""
    N, J = U.shape[-2:]
    low = _low(N)
    dtl = np.where(low, t[..., :, None] - t[..., None, :], 0.0)
    E = np.exp(-c[..., None, None, :] * dtl[..., None])
    Kl = np.einsum("...nj,...mj,...nmj->...nm", U, V, E) * low
    K = Kl + np.swapaxes(Kl, -1, -2) + a[..., :, None] * np.eye(N)
    return _dense_ll(K, y)


def _dense_ll(K, y):
    N = K.shape[-1]
    K, y = np.broadcast_arrays(K, y[..., :, None])
    y = y[..., 0]
    alpha = np.linalg.solve(K, y[..., None])[..., 0]
    sign, logabs = np.linalg.slogdet(K)
    logdet = logabs + (1j * np.angle(sign) if np.iscomplexobj(sign) else 0.0)
    return -0.5 * np.sum(y * alpha, axis=-1) - 0.5 * logdet - 0.5 * N * LOG2PI


def terms_loglik_fwd(ar, cr, ac, bc, cc, dc, x, diag, y):
    """Dense log-likelihood straight from the celerite coefficients over any leading axes, analytic (|tau| by index
    order: tau_nm = x_n - x_m for n > m on a sorted grid)."""
    N = x.shape[-1]
    low = _low(N)
    tl = np.where(low, x[..., :, None] - x[..., None, :], 0.0)
    tau = (tl + np.swapaxes(tl, -1, -2))[..., None]
    e = lambda r: r[..., None, None, :]
    K = np.sum(e(ar) * np.exp(-e(cr) * tau), axis=-1)
    K = K + np.sum(np.exp(-e(cc) * tau) * (e(ac) * np.cos(e(dc) * tau) + e(bc) * np.sin(e(dc) * tau)), axis=-1)
    K = K + diag[..., :, None] * np.eye(N)
    return _dense_ll(K, y)


def factor_fwd(t, c, a, U, V):
    """The O(N) factor recursion S_n = P (S_{n-1} + d W W^T) P, d_n = a_n - U^T S U, W_n = (V_n - S U) / d_n over any
    leading axes, analytic.  Returns d (..., N), W (..., N, J)."""
    N, J = U.shape[-2:]
    dt = np.diff(t, axis=-1)
    lead = np.broadcast_shapes(t.shape[:-1], c.shape[:-1], a.shape[:-1], U.shape[:-2], V.shape[:-2])
    dtype = np.result_type(t, c, a, U, V)
    d = np.empty(lead + (N,), dtype); W = np.empty(lead + (N, J), dtype)
    S = np.zeros(lead + (J, J), dtype)
    d[..., 0] = a[..., 0]
    W[..., 0, :] = V[..., 0, :] / a[..., 0, None]
    for n in range(1, N):
        p = np.exp(-c * dt[..., n - 1, None])
        S = S + d[..., n - 1, None, None] * W[..., n - 1, :, None] * W[..., n - 1, None, :]
        S = p[..., :, None] * S * p[..., None, :]
        Un = U[..., n, :]
        tmp = np.einsum("...i,...ij->...j", Un, S)
        d[..., n] = a[..., n] - np.sum(tmp * Un, axis=-1)
        W[..., n, :] = (V[..., n, :] - tmp) / d[..., n, None]
    return d, W


def sweep_fwd(name, t, c, U, W, Y):
    """The four O(N) sweeps over any leading axes, analytic; Y (..., N, nrhs)."""
    N, J = U.shape[-2:]
    dt = np.diff(t, axis=-1)
    lead = np.broadcast_shapes(t.shape[:-1], c.shape[:-1], U.shape[:-2], W.shape[:-2], Y.shape[:-2])
    nrhs = Y.shape[-1]
    dtype = np.result_type(t, c, U, W, Y)
    Z = np.zeros(lead + (N, nrhs), dtype)
    F = np.zeros(lead + (J, nrhs), dtype)
    solve = name.startswith("solve")
    if name.endswith("lower"):
        rows, left, right = range(N), U, W     # Z_n (+)= -/+ U_n F_n,  F_n = P (F_{n-1} + W_{n-1} X_{n-1}^T)
    else:
        rows, left, right = range(N - 1, -1, -1), W, U
    prev = None
    for n in rows:
        if prev is not None:
            p = np.exp(-c * dt[..., min(n, prev), None])
            X = Z[..., prev, :] if solve else Y[..., prev, :]
            F = p[..., :, None] * (F + right[..., prev, :, None] * X[..., None, :])
        acc = np.einsum("...j,...jk->...k", left[..., n, :], F)
        Z[..., n, :] = Y[..., n, :] - acc if solve else acc
        prev = n
    return Z


def recursive_loglik_fwd(t, c, a, U, V, y):
    """Log-likelihood by the O(N) recursions (factor, forward solve), over any leading axes, analytic."""
    d, W = factor_fwd(t, c, a, U, V)
    z = sweep_fwd("solve_lower", t, c, U, W, y[..., None])[..., 0]
    N = t.shape[-1]
    return -0.5 * np.sum(z * z / d, axis=-1) - 0.5 * np.sum(np.log(d), axis=-1) - 0.5 * N * LOG2PI


def cstep_grad(f, args, wrt=None, chunk=512, h=H):
    """Full gradient of the scalar analytic f(*args) w.r.t. args[i] for i in `wrt` (default all), by complex step: one
    perturbed element per leading-axis slot, `chunk` of them per call."""
    args = [np.asarray(x, dtype=np.float64) for x in args]
    wrt = range(len(args)) if wrt is None else wrt
    out = [None] * len(args)
    for i in wrt:
        x = args[i]
        g = np.empty(x.size)
        for s in range(0, x.size, chunk):
            k = min(chunk, x.size - s)
            pert = np.zeros((k, x.size), dtype=np.complex128)
            pert[np.arange(k), s + np.arange(k)] = 1j * h
            xi = x.reshape(1, -1) + pert
            call = [a[None].astype(np.complex128) if j != i else xi.reshape((k,) + x.shape) for j, a in enumerate(args)]
            g[s:s + k] = np.imag(f(*call)) / h
        out[i] = g.reshape(x.shape)
    return out


def cstep_jvp(f, args, directions, h=H):
    """Exact directional derivatives of the analytic f(*args): `directions` is a list of K tuples, one direction array
    (or None) per argument; returns the K derivatives (real arrays of f's shape) from ONE call over a leading axis K."""
    args = [np.asarray(x, dtype=np.float64) for x in args]
    K = len(directions)
    call = []
    for i, x in enumerate(args):
        v = np.zeros((K,) + x.shape)
        for k, dirs in enumerate(directions):
            if dirs[i] is not None:
                v[k] = dirs[i]
        call.append(x[None] + 1j * h * v)
    return np.imag(f(*call)) / h
