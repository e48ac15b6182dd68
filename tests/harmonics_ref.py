# -*- coding: utf-8 -*-
"""numpy restatement of the whitened-harmonics sweep (celerite2_amd/csrc/c2_harmonics.hip) and of what it and the torch
finish (celerite2_amd/harmonics.py) are checked against: dense algebra on the matrix the celerite matrices stand for and
dense generalized least squares per frequency.  Test infrastructure only -- nothing here is imported by the package.

Notation as periodogram_ref.  For every angular frequency w and H harmonics the NC = 2 H columns are ordered
(c_1, s_1, ..., c_H, s_H) with c_h = cos x_h, s_h = sin x_h, x_h,n = fl(fl(h w) * fl(t_n - t_ref)) -- three roundings, the way
numpy evaluates (h * w) * (t - t_ref):

    F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x NC, zero at row 0; p_n = exp(-c (t_n - t_{n-1})))
    z_n = a_n - F^T u_n
    T  += [z_i z_j (i <= j, row-major over the upper triangle), z_i Z0_n (i major)] / d_n
"""
import numpy as np

from periodogram_ref import _chi2, case, dense, err, grid, null_products  # noqa: F401  (re-exported for the tests)


def width(H, Q0):
    return H * (2 * H + 1) + 2 * H * Q0


def tri(i, j, NC):
    """Where <z_i, z_j> (i <= j) stands in T."""
    return i * NC - (i * (i - 1)) // 2 + (j - i)


def harmonic_frequencies(freq, H):
    """(H, ...) = fl(h * freq), h = 1 .. H."""
    return np.stack([float(h) * np.asarray(freq) for h in range(1, H + 1)])


def columns(t, freq, H, t_ref=0.0):
    """(NC, N, F): the columns as the kernel forms them."""
    out = []
    for wh in harmonic_frequencies(freq, H):
        x = wh[None, :] * (t - t_ref)[:, None]
        out += [np.cos(x), np.sin(x)]
    return np.stack(out)


def whitened_harmonics(t, c, U, W, d, Z0, freq, H, t_ref=0.0):
    """The sweep in the kernel's order for one series, the frequencies along a numpy axis: one state per column, nothing
    stored per row, row 0 the general step with p = 1 and w_{-1} z_{-1} = 0; F^T u_n in four interleaved partial sums; z
    scaled by a reciprocal of d_n once, then multiplied.  Returns T (F, H (2 H + 1) + 2 H Q0)."""
    N, J = U.shape
    Q0, nf, NC = Z0.shape[1], len(freq), 2 * H
    HEAD = H * (2 * H + 1)
    wh = harmonic_frequencies(freq, H)                       # (H, F)
    Fst = np.zeros((NC, J, nf))
    T = np.zeros((nf, width(H, Q0)))
    wprev, z, tprev = np.zeros(J), np.zeros((NC, nf)), t[0]
    for n in range(N):
        p = np.exp(c * (tprev - t[n]))
        tprev = t[n]
        x = wh * (t[n] - t_ref)                              # the difference is rounded, then the product
        a = np.empty((NC, nf))
        a[0::2], a[1::2] = np.cos(x), np.sin(x)
        Fst = p[None, :, None] * (Fst + wprev[None, :, None] * z[:, None, :])
        acc = np.zeros((4, NC, nf))
        for j in range(J):
            acc[j & 3] += Fst[:, j] * U[n, j]
        z = a - ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        zd = z * (1.0 / d[n])
        for i in range(NC):
            T[:, tri(i, i, NC)] += z[i] * zd[i]
            for j in range(i + 1, NC):
                T[:, tri(i, j, NC)] += zd[i] * z[j]
            T[:, HEAD + i * Q0:HEAD + (i + 1) * Q0] += zd[i][:, None] * Z0[n][None, :]
        wprev = W[n]
    return T


def whitened_harmonics_batched(t, c, U, W, d, Z0, freq, H, t_ref=0.0):
    """`whitened_harmonics` for a whole batch at once: t (B, N), c (B, J), U, W (B, N, J), d (B, N), Z0 (B, N, Q0),
    freq (B, F) -> (B, F, width).  The same statements with a leading axis (F^T u_n in one sum: the order inside a row is
    below the criterion)."""
    B, N, J = U.shape
    Q0, nf, NC = Z0.shape[2], freq.shape[1], 2 * H
    HEAD = H * (2 * H + 1)
    wh = harmonic_frequencies(freq, H)                       # (H, B, F)
    Fst = np.zeros((NC, B, J, nf))
    T = np.zeros((B, nf, width(H, Q0)))
    wprev, z, tprev = np.zeros((B, J)), np.zeros((NC, B, nf)), t[:, 0]
    for n in range(N):
        p = np.exp(c * (tprev - t[:, n])[:, None])
        tprev = t[:, n]
        x = wh * (t[:, n] - t_ref)[None, :, None]
        a = np.empty((NC, B, nf))
        a[0::2], a[1::2] = np.cos(x), np.sin(x)
        Fst = p[None, :, :, None] * (Fst + wprev[None, :, :, None] * z[:, :, None, :])
        z = a - np.einsum("ibjf,bj->ibf", Fst, U[:, n])
        zd = z * (1.0 / d[:, n])[None, :, None]
        for i in range(NC):
            T[:, :, tri(i, i, NC)] += z[i] * zd[i]
            for j in range(i + 1, NC):
                T[:, :, tri(i, j, NC)] += zd[i] * z[j]
            T[:, :, HEAD + i * Q0:HEAD + (i + 1) * Q0] += zd[i][:, :, None] * Z0[:, n][:, None, :]
        wprev = W[:, n]
    return T


def dense_products(K, t, Y0, freq, H, t_ref=0.0):
    """T (F, width) from dense algebra: the products of the NC columns of every frequency and of Y0 = L Z0 under K^-1."""
    C = columns(t, freq, H, t_ref)                           # (NC, N, F)
    NC, Q0 = 2 * H, Y0.shape[1]
    KiC = np.stack([np.linalg.solve(K, Ci) for Ci in C])
    KiY = np.linalg.solve(K, Y0)
    T = np.zeros((len(freq), width(H, Q0)))
    for i in range(NC):
        for j in range(i, NC):
            T[:, tri(i, j, NC)] = (C[i] * KiC[j]).sum(0)
        T[:, H * (2 * H + 1) + i * Q0:H * (2 * H + 1) + (i + 1) * Q0] = C[i].T @ KiY
    return T


def dense_harmonics(K, t, A0, y, freq, H, t_ref=0.0):
    """Two dense generalized-least-squares fits per frequency, sharing no formula with the package: chi2 of y on A0 (N, P0; P0
    may be 0) and on [A0 | the 2 H columns].  Returns (dchi2 (F,), amplitude (F, 2 H), chi2_null)."""
    Lc = np.linalg.cholesky(K)
    chi2_0, _ = _chi2(Lc, A0, y)
    C = columns(t, freq, H, t_ref)
    dchi2, amp = np.empty(len(freq)), np.empty((len(freq), 2 * H))
    for f in range(len(freq)):
        chi2_1, beta = _chi2(Lc, np.concatenate([A0, C[:, :, f].T], axis=1), y)
        dchi2[f], amp[f] = chi2_0 - chi2_1, beta[-2 * H:]
    return dchi2, amp, chi2_0


def waveform(amp, freq, t, t_ref=0.0):
    """sum_h alpha_h cos x_h + beta_h sin x_h at t for one frequency."""
    out = np.zeros_like(t)
    for h in range(1, len(amp) // 2 + 1):
        x = (float(h) * freq) * (t - t_ref)
        out += amp[2 * h - 2] * np.cos(x) + amp[2 * h - 1] * np.sin(x)
    return out
