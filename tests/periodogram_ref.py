# -*- coding: utf-8 -*-
"""numpy restatement of the whitened-sinusoid sweep (celerite2_amd/csrc/c2_periodogram.hip: trial::k_trial_sweep on trial::Sinusoid) and of what it and the torch
finish (celerite2_amd/periodogram.py) are checked against: dense algebra on the matrix the celerite matrices stand for,
dense generalized least squares per frequency, and the classical floating-mean periodogram in closed form.  Test
infrastructure only -- nothing here is imported by the package.

Notation as linear_model_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay), <a, b> = sum_n a_n b_n / d_n.  For
every angular frequency w, with x_n = fl(w * fl(t_n - t_ref)) (two roundings: the way numpy evaluates w * (t - t_ref)):

    F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x 2, zero at row 0; p_n = exp(-c (t_n - t_{n-1})))
    z_n = (cos x_n, sin x_n) - F^T u_n
    T  += [z_c z_c, z_c z_s, z_s z_s, z_c Z0_n, z_s Z0_n] / d_n
"""
import numpy as np

from linear_model_ref import dense, design, draw, err, factor, sweep  # noqa: F401  (re-exported for the tests)


def grid(t, F=65, lo=1.0, hi=20.0):
    """F angular frequencies from `lo` to `hi` cycles over the baseline of t (one cycle over the baseline is the lowest
    frequency at which a sinusoid is told from a constant); the unit grid when the baseline is zero (N = 1)."""
    span = float(np.max(t) - np.min(t))
    return 2.0 * np.pi / (span if span > 0 else 1.0) * np.linspace(lo, hi, F)


def whitened_sinusoids(t, c, U, W, d, Z0, freq, t_ref=0.0):
    """The sweep in the kernel's order for one series, the frequencies (the lanes) along a numpy axis: one state, nothing
    stored per row, rows 0 .. N-1; row 0 takes the general step with p = 1 and w_{-1} z_{-1} = 0; F^T u_n in four
    interleaved partial sums; z scaled by a reciprocal of d_n once, then multiplied.  The staged blocks move data only.
    Returns T (F, 3 + 2 Q0)."""
    N, J = U.shape
    Q0, nf = Z0.shape[1], len(freq)
    Fc, Fs = np.zeros((J, nf)), np.zeros((J, nf))
    T = np.zeros((nf, 3 + 2 * Q0))
    wprev, zc, zs, tprev = np.zeros(J), np.zeros(nf), np.zeros(nf), t[0]
    for n in range(N):
        p = np.exp(c * (tprev - t[n]))
        tprev = t[n]
        x = freq * (t[n] - t_ref)                  # the difference is rounded, then the product
        cs, sn = np.cos(x), np.sin(x)
        Fc = p[:, None] * (Fc + wprev[:, None] * zc[None, :])
        Fs = p[:, None] * (Fs + wprev[:, None] * zs[None, :])
        ac, as_ = np.zeros((4, nf)), np.zeros((4, nf))
        for j in range(J):
            ac[j & 3] += Fc[j] * U[n, j]
            as_[j & 3] += Fs[j] * U[n, j]
        zc = cs - ((ac[0] + ac[1]) + (ac[2] + ac[3]))
        zs = sn - ((as_[0] + as_[1]) + (as_[2] + as_[3]))
        rd = 1.0 / d[n]
        zcd, zsd = zc * rd, zs * rd
        T[:, 0] += zc * zcd
        T[:, 1] += zcd * zs
        T[:, 2] += zs * zsd
        T[:, 3:3 + Q0] += zcd[:, None] * Z0[n][None, :]
        T[:, 3 + Q0:] += zsd[:, None] * Z0[n][None, :]
        wprev = W[n]
    return T


def whitened_sinusoids_batched(t, c, U, W, d, Z0, freq, t_ref=0.0):
    """`whitened_sinusoids` for a whole batch at once: t (B, N), c (B, J), U, W (B, N, J), d (B, N), Z0 (B, N, Q0),
    freq (B, F) -> (B, F, 3 + 2 Q0).  The same statements with a leading axis (F^T u_n in one sum: the order inside a row
    is below the criterion)."""
    B, N, J = U.shape
    Q0, nf = Z0.shape[2], freq.shape[1]
    Fc, Fs = np.zeros((B, J, nf)), np.zeros((B, J, nf))
    T = np.zeros((B, nf, 3 + 2 * Q0))
    wprev, zc, zs, tprev = np.zeros((B, J)), np.zeros((B, nf)), np.zeros((B, nf)), t[:, 0]
    for n in range(N):
        p = np.exp(c * (tprev - t[:, n])[:, None])
        tprev = t[:, n]
        x = freq * (t[:, n] - t_ref)[:, None]
        Fc = p[:, :, None] * (Fc + wprev[:, :, None] * zc[:, None, :])
        Fs = p[:, :, None] * (Fs + wprev[:, :, None] * zs[:, None, :])
        zc = np.cos(x) - np.einsum("bjf,bj->bf", Fc, U[:, n])
        zs = np.sin(x) - np.einsum("bjf,bj->bf", Fs, U[:, n])
        rd = (1.0 / d[:, n])[:, None]
        zcd, zsd = zc * rd, zs * rd
        T[:, :, 0] += zc * zcd
        T[:, :, 1] += zcd * zs
        T[:, :, 2] += zs * zsd
        T[:, :, 3:3 + Q0] += zcd[:, :, None] * Z0[:, n][:, None, :]
        T[:, :, 3 + Q0:] += zsd[:, :, None] * Z0[:, n][:, None, :]
        wprev = W[:, n]
    return T


def null_products(Z0, d):
    """S0 (Q0, Q0) = Z0^T diag(1/d) Z0."""
    return Z0.T @ (Z0 / d[:, None])


def columns(t, freq, t_ref=0.0):
    """(cos, sin), each (N, F), of the phase as the kernel forms it."""
    x = freq[None, :] * (t - t_ref)[:, None]
    return np.cos(x), np.sin(x)


def dense_products(K, t, Y0, freq, t_ref=0.0):
    """T (F, 3 + 2 Q0) from dense algebra: the products of the two columns of every frequency and of Y0 = L Z0 under K^-1."""
    C, S = columns(t, freq, t_ref)
    KiC, KiS, KiY = np.linalg.solve(K, C), np.linalg.solve(K, S), np.linalg.solve(K, Y0)
    return np.concatenate([np.stack([(C * KiC).sum(0), (C * KiS).sum(0), (S * KiS).sum(0)], axis=1), C.T @ KiY, S.T @ KiY], axis=1)


def _chi2(Lc, X, y):
    """min_beta (y - X beta)^T K^-1 (y - X beta) and the minimiser, by least squares on the whitened problem (K = Lc Lc^T)."""
    yw = np.linalg.solve(Lc, y)
    if X.shape[1] == 0:
        return float(yw @ yw), np.zeros(0)
    Xw = np.linalg.solve(Lc, X)
    beta = np.linalg.lstsq(Xw, yw, rcond=None)[0]
    r = yw - Xw @ beta
    return float(r @ r), beta


def dense_periodogram(K, t, A0, y, freq, t_ref=0.0):
    """Two dense generalized-least-squares fits per frequency, sharing no formula with the package: chi2 of y on A0 (N, P0; P0
    may be 0) and on [A0 | cos | sin].  Returns (dchi2 (F,), amplitude (F, 2), chi2_null)."""
    Lc = np.linalg.cholesky(K)
    chi2_0, _ = _chi2(Lc, A0, y)
    C, S = columns(t, freq, t_ref)
    dchi2, amp = np.empty(len(freq)), np.empty((len(freq), 2))
    for f in range(len(freq)):
        chi2_1, beta = _chi2(Lc, np.concatenate([A0, C[:, f:f + 1], S[:, f:f + 1]], axis=1), y)
        dchi2[f], amp[f] = chi2_0 - chi2_1, beta[-2:]
    return dchi2, amp, chi2_0


def classical_gls(t, y, sigma2, freq, t_ref=0.0):
    """The floating-mean (generalized) Lomb-Scargle periodogram of Zechmeister & Kuerster (2009, eqs. 4-15) from weighted
    sums, weights 1 / sigma2 normalised to one: p (F,) in [0, 1]."""
    w = (1.0 / sigma2) / np.sum(1.0 / sigma2)
    C, S = columns(t, freq, t_ref)
    Y, Cm, Sm = np.sum(w * y), w @ C, w @ S
    YY = np.sum(w * y * y) - Y * Y
    YC, YS = (w * y) @ C - Y * Cm, (w * y) @ S - Y * Sm
    CC, SS, CS = w @ (C * C) - Cm * Cm, w @ (S * S) - Sm * Sm, w @ (C * S) - Cm * Sm
    D = CC * SS - CS * CS
    return (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D)


def case(seed, N, J, P0=1, F=65):
    """One series: draw's dict with d, W (its factors), A0 = design(t, P0) (N, P0; a constant first column), Y0 = [A0 | y],
    Z0 = L^-1 Y0 and the grid freq."""
    D = draw(seed, N, J)
    D["d"], D["W"] = factor(D["t"], D["c"], D["a"], D["U"], D["V"])
    D["A0"] = design(D["t"], P0) if P0 else np.zeros((N, 0))
    D["Y0"] = np.concatenate([D["A0"], D["y"][:, None]], axis=1)
    D["Z0"] = sweep(D["t"], D["c"], D["U"], D["W"], D["Y0"])[0]
    D["freq"] = grid(D["t"], F)
    return D
