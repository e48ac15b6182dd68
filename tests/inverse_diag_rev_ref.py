# -*- coding: utf-8 -*-
"""numpy restatement of the inverse-diagonal sweep WITH its saved states and of its reverse pass
(celerite2_amd/csrc/c2_invdiag.hip with the workspace flag, csrc/c2_invdiag_rev.hip), and the dense closed form of the
leave-one-out log predictive density and its gradient.  Test infrastructure only -- nothing here is imported by the package.

Forward (inverse_diag_ref.inverse_diag), for n = N-1 .. 0, storing the state ENTERING row n:
    Mws[n] = M ;  Fws[n] = F   (F with u_{n+1} alpha_{n+1} already added; both 0 at n = N-1)
    p = exp(-c (t_{n+1} - t_n)) (1 at n = N-1) ;  G = (p p^T) o M ;  g = G w ;  q_n = 1/d_n + w.g
    alpha_n = z_n / d_n - w.(p o F)
    M <- G - u g^T - g u^T + q_n u u^T ;  F <- p o F + u alpha_n

Reverse, n = 0 .. N-1, adjoint state Mb, Fb = 0: the recurrence in `adjoint` below.

The objective (Rasmussen & Williams 5.4.2), with q = diag(K^-1), alpha = K^-1 r:
    loo = sum_n (log q_n - alpha_n^2 / q_n) / 2 - N log(2 pi) / 2
    bq_n = 1 / (2 q_n) + alpha_n^2 / (2 q_n^2) ,  balpha_n = -alpha_n / q_n
and, dense: d loo = sum_nm A_nm dK_nm with A = sym(-K^-1 diag(bq) K^-1 - (K^-1 balpha) alpha^T), b r = K^-1 balpha.
"""
import numpy as np

from inverse_diag_ref import dense  # noqa: F401  (re-exported for the tests)

LOG2PI = float(np.log(2.0 * np.pi))


def forward_states(t, c, U, W, d, z=None):
    """(q, alpha, Mws, Fws) over any leading axes, analytic (complex arguments allowed): t (..., N), c (..., J),
    U, W (..., N, J), d, z (..., N).  alpha, Fws are None without z."""
    N, J = U.shape[-2:]
    lead = np.broadcast_shapes(t.shape[:-1], c.shape[:-1], U.shape[:-2], W.shape[:-2], d.shape[:-1],
                               () if z is None else z.shape[:-1])
    dt = np.result_type(t, c, U, W, d, *(() if z is None else (z,)))
    q = np.empty(lead + (N,), dtype=dt)
    alpha = None if z is None else np.empty(lead + (N,), dtype=dt)
    Mws = np.zeros(lead + (N, J, J), dtype=dt)
    Fws = None if z is None else np.zeros(lead + (N, J), dtype=dt)
    M = np.zeros(lead + (J, J), dtype=dt)
    F = np.zeros(lead + (J,), dtype=dt)
    for n in range(N - 1, -1, -1):
        Mws[..., n, :, :] = M
        if z is not None:
            Fws[..., n, :] = F
        p = np.ones_like(c) if n == N - 1 else np.exp(-c * (t[..., n + 1] - t[..., n])[..., None])
        u, w = U[..., n, :], W[..., n, :]
        G = p[..., :, None] * p[..., None, :] * M
        g = np.einsum("...ij,...j->...i", G, w)
        q[..., n] = 1.0 / d[..., n] + np.sum(w * g, axis=-1)
        M = (G - u[..., :, None] * g[..., None, :] - g[..., :, None] * u[..., None, :]
             + q[..., n, None, None] * u[..., :, None] * u[..., None, :])
        if z is not None:
            Fp = p * F
            alpha[..., n] = z[..., n] / d[..., n] - np.sum(w * Fp, axis=-1)
            F = Fp + u * alpha[..., n, None]
    return q, alpha, Mws, Fws


def adjoint(t, c, U, W, d, z, q, alpha, Mws, Fws, bq, balpha):
    """(bt, bc, bU, bW, bd, bz) of ONE series from the cotangents bq, balpha (N,) and the saved states; z, alpha, Fws,
    balpha None together (then bz is None)."""
    N, J = U.shape
    hz = z is not None
    bt, bc, bU, bW, bd = np.zeros(N), np.zeros(J), np.zeros((N, J)), np.zeros((N, J)), np.zeros(N)
    bz = np.zeros(N) if hz else None
    Mb, Fb = np.zeros((J, J)), np.zeros(J)
    for n in range(N):
        p = np.ones(J) if n == N - 1 else np.exp(-c * (t[n + 1] - t[n]))
        u, w, M = U[n], W[n], Mws[n]
        F = Fws[n] if hz else np.zeros(J)
        G = np.outer(p, p) * M
        g = G @ w
        Fp = p * F
        a_ = (balpha[n] + u @ Fb) if hz else 0.0
        bu = (alpha[n] * Fb) if hz else np.zeros(J)
        Fbp = Fb - a_ * w
        bw = -a_ * Fp
        if hz:
            bz[n] = a_ / d[n]
            bd[n] = -a_ * z[n] / d[n] ** 2
        Mu = Mb @ u
        q_ = bq[n] + u @ Mu
        gb = -2.0 * Mu + q_ * w
        bu = bu - 2.0 * (Mb @ g) + 2.0 * q[n] * Mu
        bd[n] += -q_ / d[n] ** 2
        bw = bw + q_ * g + G @ gb
        Gb = Mb + 0.5 * (np.outer(gb, w) + np.outer(w, gb))
        pb = 2.0 * (Gb * M) @ p + F * Fbp
        Mb = np.outer(p, p) * Gb
        Fb = p * Fbp
        bU[n], bW[n] = bu, bw
        if n < N - 1:
            dt = t[n + 1] - t[n]
            bc += -dt * pb * p
            x = -np.sum(c * pb * p)
            bt[n + 1] += x
            bt[n] -= x
    return bt, bc, bU, bW, bd, bz


def loo_value(q, alpha):
    return 0.5 * np.sum(np.log(q) - alpha * alpha / q, axis=-1) - 0.5 * q.shape[-1] * LOG2PI


def loo_cotangents(q, alpha):
    return 0.5 / q + 0.5 * alpha * alpha / (q * q), -alpha / q


def dense_loo(K, r):
    """loo, the matrix cotangent A (d loo = sum_nm A_nm dK_nm, symmetric) and b r = K^-1 balpha, from the dense K."""
    L = np.linalg.cholesky(K)
    Li = np.linalg.inv(L)
    Kinv = Li.T @ Li
    Kinv = 0.5 * (Kinv + Kinv.T)
    q, alpha = np.diag(Kinv).copy(), Kinv @ r
    bq, ba = loo_cotangents(q, alpha)
    Kba = Kinv @ ba
    A = -(Kinv * bq[None, :]) @ Kinv - np.outer(Kba, alpha)
    return float(loo_value(q, alpha)), 0.5 * (A + A.T), Kba


def dense_loo_grad(t, c, a, U, V, y):
    """Exact loo and (bt, bc, ba, bU, bV, by) of ONE series from its dense semiseparable matrix (oracle.exact)."""
    from oracle import exact

    val, A, by = dense_loo(exact.dense_from_semiseparable(t, c, a, U, V), y)
    bt, bc, bU, bV = exact.contract_lower(2.0 * A, t, c, U, V)
    return val, (bt, bc, np.diag(A).copy(), bU, bV, by)


def terms_contract(G, ar, cr, ac, bc, cc, dc, x):
    """The matrix cotangent G (d f = sum_nm G_nm dK_nm, symmetric) of the dense kernel matrix of the celerite coefficients
    pushed to (bar, bcr, bac, bbc, bcc, bdc, bx, bdiag): oracle.exact.terms_grad's contraction with G given."""
    ar, cr, ac, bc, cc, dc = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (ar, cr, ac, bc, cc, dc))
    N = len(x)
    low = np.tril(np.ones((N, N), dtype=bool), -1)
    tl = np.where(low, x[:, None] - x[None, :], 0.0)
    tau, sgn = tl + tl.T, low.astype(np.float64) - low.T.astype(np.float64)
    kp = np.zeros_like(tau)
    bar, bcr = np.empty(len(ar)), np.empty(len(ar))
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
    return bar, bcr, bac, bbc, bcc, bdc, bx, np.diag(G).copy()
