# -*- coding: utf-8 -*-
"""numpy restatement of the whitened-transit sweep (celerite2_amd/csrc/c2_transit.hip: trial::k_trial_sweep on trial::Transit) and of what it and the torch finish
(celerite2_amd/transit.py) are checked against: dense algebra on the matrix the celerite matrices stand for, two dense
generalized-least-squares fits per trial, and the classical weighted box-least-squares statistic in closed form.  Test
infrastructure only -- nothing here is imported by the package.

Notation as linear_model_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay), <a, b> = sum_n a_n b_n / d_n.  A trial is
(period P, epoch t0, duration w, ingress tau); P = 0 is a single event.  The template rule of the public header, each line
rounded once:

    invP = 1 / P;  x = t_n - t0;  q = rint(x invP) (0 when P == 0);  phi = x - q P;  u = 0.5 w - |phi|
    b_n = 0 if u < 0;  1 if u >= tau;  u / tau otherwise

    f <- p_n o (f + w_{n-1} z_{n-1})        (f: J, zero at row 0; p_n = exp(-c (t_n - t_{n-1})))
    z_n = b_n - f^T u_n
    T  += [z z, z Z0_n] / d_n
"""
import numpy as np

from linear_model_ref import dense, design, draw, err, factor, sweep  # noqa: F401  (re-exported for the tests)
from periodogram_ref import _chi2, null_products  # noqa: F401


def template(t, trials):
    """b (..., N, K) by the header's rule for t (..., N) and trials (..., K, 4): the statements of the kernel, in its order."""
    P, t0, w, tau = [trials[..., None, :, i] for i in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        invP = np.where(P != 0.0, 1.0 / np.where(P != 0.0, P, 1.0), 0.0)
        x = t[..., :, None] - t0
        q = np.rint(x * invP)
        phi = x - q * P
        u = 0.5 * w - np.abs(phi)
        ramp = u / np.where(tau != 0.0, tau, 1.0)
    return np.where(u >= tau, 1.0, np.where((u >= 0.0) & (u < tau), ramp, 0.0))


def template_independent(t, trials):
    """The same template built another way, for the dense oracles: the phase from np.fmod on a shifted, non-negative
    argument (no rint, no reciprocal of P), the shape from a clip of the scaled distance to the edge.  (N, K)."""
    out = np.empty((len(t), len(trials)))
    for k, (P, t0, w, tau) in enumerate(trials):
        x = t - t0
        if P > 0:
            shift = (np.floor(np.max(np.abs(x)) / P) + 2.0) * P
            x = np.fmod(x + shift + 0.5 * P, P) - 0.5 * P
        dist = 0.5 * w - np.abs(x)                      # > 0 inside the outer edges
        out[:, k] = (dist >= 0.0).astype(float) if tau == 0 else np.clip(dist / tau, 0.0, 1.0)
    return out


def whitened_transits(t, c, U, W, d, Z0, trials):
    """The sweep in the kernel's order for one series, the trials (the lanes) along a numpy axis: one state, nothing stored
    per row, rows 0 .. N-1; row 0 takes the general step with p = 1 and w_{-1} z_{-1} = 0; f^T u_n in four interleaved
    partial sums; z scaled by a reciprocal of d_n once, then multiplied.  The staged blocks move data only.
    Returns T (K, 1 + Q0)."""
    N, J = U.shape
    Q0, nk = Z0.shape[1], len(trials)
    b = template(t, trials)
    F = np.zeros((J, nk))
    T = np.zeros((nk, 1 + Q0))
    wprev, z, tprev = np.zeros(J), np.zeros(nk), t[0]
    for n in range(N):
        p = np.exp(c * (tprev - t[n]))
        tprev = t[n]
        F = p[:, None] * (F + wprev[:, None] * z[None, :])
        acc = np.zeros((4, nk))
        for j in range(J):
            acc[j & 3] += F[j] * U[n, j]
        z = b[n] - ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        zd = z * (1.0 / d[n])
        T[:, 0] += z * zd
        T[:, 1:] += zd[:, None] * Z0[n][None, :]
        wprev = W[n]
    return T


def whitened_transits_batched(t, c, U, W, d, Z0, trials):
    """`whitened_transits` for a whole batch at once: t (B, N), c (B, J), U, W (B, N, J), d (B, N), Z0 (B, N, Q0),
    trials (B, K, 4) -> (B, K, 1 + Q0).  The same statements with a leading axis (f^T u_n in one sum: the order inside a row
    is below the criterion)."""
    B, N, J = U.shape
    Q0, nk = Z0.shape[2], trials.shape[1]
    b = template(t, trials)                               # (B, N, K)
    F = np.zeros((B, J, nk))
    T = np.zeros((B, nk, 1 + Q0))
    wprev, z, tprev = np.zeros((B, J)), np.zeros((B, nk)), t[:, 0]
    for n in range(N):
        p = np.exp(c * (tprev - t[:, n])[:, None])
        tprev = t[:, n]
        F = p[:, :, None] * (F + wprev[:, :, None] * z[:, None, :])
        z = b[:, n] - np.einsum("bjk,bj->bk", F, U[:, n])
        zd = z * (1.0 / d[:, n])[:, None]
        T[:, :, 0] += z * zd
        T[:, :, 1:] += zd[:, :, None] * Z0[:, n][:, None, :]
        wprev = W[:, n]
    return T


def dense_products(K, t, Y0, trials):
    """T (K, 1 + Q0) from dense algebra: the products of every trial's template, built the independent way, and of
    Y0 = L Z0 under K^-1."""
    Bm = template_independent(t, trials)
    KiB = np.linalg.solve(K, Bm)
    return np.concatenate([(Bm * KiB).sum(0)[:, None], KiB.T @ Y0], axis=1)


def dense_search(K, t, A0, y, trials):
    """Two dense generalized-least-squares fits per trial, sharing no formula with the package: chi2 of y on A0 (N, P0; P0
    may be 0) and on [A0 | b_k], and the variance of the depth from the inverse of the whitened normal matrix.  Returns
    (dchi2 (K,), depth (K,), depth_err (K,), chi2_null)."""
    Lc = np.linalg.cholesky(K)
    chi2_0, _ = _chi2(Lc, A0, y)
    Bm = template_independent(t, trials)
    dchi2, depth, derr = np.empty(len(trials)), np.empty(len(trials)), np.empty(len(trials))
    for k in range(len(trials)):
        X = np.concatenate([A0, Bm[:, k:k + 1]], axis=1)
        chi2_1, beta = _chi2(Lc, X, y)
        Xw = np.linalg.solve(Lc, X)
        cov = np.linalg.inv(Xw.T @ Xw)
        dchi2[k], depth[k], derr[k] = chi2_0 - chi2_1, beta[-1], np.sqrt(cov[-1, -1])
    return dchi2, depth, derr, chi2_0


def classical_bls(t, y, sigma2, trials):
    """Weighted box least squares with a floating mean (Kovacs, Zucker & Mazeh 2002, section 2, with weights
    1 / sigma2 normalised to one): r = the weight in transit, s = the weighted mean-subtracted flux in transit;
    depth = s / (r (1 - r)) and dchi2 = (sum 1 / sigma2) s^2 / (r (1 - r)).  Boxes only.  Returns (dchi2 (K,), depth (K,))."""
    wsum = np.sum(1.0 / sigma2)
    wt = (1.0 / sigma2) / wsum
    yc = y - np.sum(wt * y)
    Bm = template_independent(t, trials)
    assert np.all((Bm == 0.0) | (Bm == 1.0))
    r, s = wt @ Bm, (wt * yc) @ Bm
    return wsum * s * s / (r * (1.0 - r)), s / (r * (1.0 - r))


def _edge(a, lo, hi, pick):
    """A midpoint between two neighbours of the sorted distinct distances `a` with at least `lo` of them below and `hi` of
    them above where there are that many; among the admissible gaps the `pick`-th widest half."""
    if len(a) == 1:
        return a[0] + 1.0
    i_lo, i_hi = min(lo, len(a) - 1), max(len(a) - hi, 1)
    idx = np.arange(i_lo, max(i_lo, i_hi) + 1)               # (too few points for both: the ones below come first)
    gaps = a[idx] - a[idx - 1]
    order = idx[np.argsort(-gaps)]
    i = order[pick % max(1, (len(order) + 1) // 2)]
    return 0.5 * (a[i - 1] + a[i])


def trials_for(t, K=65, kinds=("fold-box", "fold-trap", "single-box", "single-trap"), seed=0, outside=False):
    """(K, 4) trials built from the drawn times so that every template edge, |phi| = w / 2 and |phi| = w / 2 - tau, falls at a
    midpoint between two neighbouring (folded) sample distances: no sample decides differently under a last-bit change of
    its phase, however the template is built.  `kinds` rotate lane by lane.  Periods are a fifth to a half of the span (so a
    fold's w stays well below P / 2 whenever the series has a few points), epochs are drawn over the span -- with `outside`,
    single events are sorted by epoch and the first and last quarter lie before t_0 and after t_{N-1} with every sample out
    of transit.  Where the series allows it, two samples at least are in transit and two out of it (`counts`)."""
    rng = np.random.default_rng(seed)
    span = float(t[-1] - t[0]) if len(t) > 1 and t[-1] > t[0] else 1.0
    out = np.zeros((K, 4))
    epochs = np.sort(rng.uniform(t[0], t[0] + span, K))
    for k in range(K):
        kind = kinds[k % len(kinds)]
        P = span / rng.uniform(2.0, 5.0) if kind.startswith("fold") else 0.0
        t0 = rng.uniform(t[0], t[0] + span) if not outside else epochs[k]
        tr = np.array([[P, t0, 1.0, 0.0]])
        x = t - t0
        phi = np.abs(x - np.rint(x / P) * P) if P > 0 else np.abs(x)
        a = np.unique(phi)
        if outside and (k < K // 4 or k >= K - K // 4):
            side = -1.0 if k < K // 4 else 1.0
            t0 = (t[0] if side < 0 else t[-1]) + side * span * (0.3 + 0.01 * (K // 4 - k if side < 0 else k))   # (ascending in k)
            h = 0.1 * span                                # every |phi| >= 0.3 span: all out of transit
            a_in = np.array([0.0])
        else:
            if P > 0:
                a = a[a < 0.4 * P] if np.sum(a < 0.4 * P) >= 4 else a
            h = _edge(a, 2, 2, k)
            a_in = a[a < h]
        tau = 0.0
        if kind.endswith("trap"):
            inner = _edge(a_in, 1, 1, k // 2) if len(a_in) >= 2 else 0.5 * a_in[0]
            tau = h - min(inner, h)
            tau = min(tau, h)                             # tau <= w / 2
        out[k] = (P, t0, 2.0 * h, tau)
    return out


def counts(t, trials):
    """(samples with b > 0, samples with b == 0) per trial, by the rule."""
    b = template(t, trials)
    return (b > 0).sum(axis=0), (b == 0).sum(axis=0)


def case(seed, N, J, P0=1, K=65, **kw):
    """One series: draw's dict with d, W (its factors), A0 = design(t, P0) (N, P0; a constant first column), Y0 = [A0 | y],
    Z0 = L^-1 Y0 and the midpoint-edge trials."""
    D = draw(seed, N, J)
    D["d"], D["W"] = factor(D["t"], D["c"], D["a"], D["U"], D["V"])
    D["A0"] = design(D["t"], P0) if P0 else np.zeros((N, 0))
    D["Y0"] = np.concatenate([D["A0"], D["y"][:, None]], axis=1)
    D["Z0"] = sweep(D["t"], D["c"], D["U"], D["W"], D["Y0"])[0]
    D["trials"] = trials_for(D["t"], K, seed=seed, **kw)
    return D
