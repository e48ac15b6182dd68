# -*- coding: utf-8 -*-
"""numpy restatement of the tabulated-shape column (trial::Shape, celerite2_amd/csrc/c2_trial_columns.hpp), of the sweep that whitens it
(c2_shapes.hip) and of the projection onto it (c2_trial_project.hip), and of what they and the torch finish
(celerite2_amd/shapes.py) are checked against: dense algebra on the matrix the celerite matrices stand for with the column
built another way, and two dense generalized-least-squares fits per trial.  Test infrastructure only -- nothing here is
imported by the package.

Notation as linear_model_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay), <a, b> = sum_n a_n b_n / d_n.  A trial is
(period P, epoch t0, width w, shape index s); P = 0 is a single event; a bank is (NS, S).  The rule of the public header,
each line rounded once:

    invP = 1 / P (0 when P == 0);  ginv = fl(S - 1) / w;  is = (s >= 0 and s < NS) ? int(s) : 0
    x = t_n - t0;  q = rint(x invP);  phi = x - q P;  u = 0.5 w - |phi|;  v = phi + 0.5 w
    g = v ginv;  g = g > 0 ? g : 0;  g = g < S - 1 ? g : S - 1;  i = min(int(floor(g)), S - 2);  fr = g - i
    dlt = shape[is][i + 1] - shape[is][i];  b_n = 0 if u < 0 else shape[is][i] + fr dlt

    f <- p_n o (f + w_{n-1} z_{n-1})        (f: J, zero at row 0; p_n = exp(-c (t_n - t_{n-1})))
    z_n = b_n - f^T u_n
    T  += [z z, z Z0_n] / d_n
"""
import numpy as np

import transit_ref as TR
from linear_model_ref import dense, design, draw, err, factor, sweep  # noqa: F401  (re-exported for the tests)
from periodogram_ref import _chi2, null_products  # noqa: F401


def column(t, trials, shapes):
    """b (..., N, K) by the header's rule for t (..., N), trials (..., K, 4) and the bank (NS, S) | (..., NS, S): the
    statements of the kernel, in its order."""
    NS, S = shapes.shape[-2:]
    P, t0, w, s = [trials[..., None, :, i] for i in range(4)]
    with np.errstate(all="ignore"):
        invP = np.where(P != 0.0, 1.0 / np.where(P != 0.0, P, 1.0), 0.0)
        top = np.float64(S - 1)
        ginv = top / w
        ok = (s >= 0.0) & (s < float(NS))
        idx = np.where(ok, s, 0.0).astype(np.int64)          # (truncation; NaN fails both comparisons)
        x = t[..., :, None] - t0
        q = np.rint(x * invP)
        phi = x - q * P
        u = 0.5 * w - np.abs(phi)
        v = phi + 0.5 * w
        g = v * ginv
        g = np.where(g > 0.0, g, 0.0)
        g = np.where(g < top, g, top)
        i = np.minimum(np.floor(g).astype(np.int64), S - 2)
        fr = g - i
        idx = np.broadcast_to(idx, i.shape)
        if shapes.ndim == 2:
            a, c = shapes[idx, i], shapes[idx, i + 1]
        else:                                                  # (B, NS, S) beside t (B, N), trials (B, K, 4)
            bb = np.arange(shapes.shape[0])[:, None, None]
            a, c = shapes[bb, idx, i], shapes[bb, idx, i + 1]
        dlt = c - a
        b = a + fr * dlt
    return np.where(u < 0.0, 0.0, b)


def column_independent(t, trials, shapes):
    """The same column built another way, for the dense oracles: the phase from a fold in np.longdouble (no reciprocal of P,
    the difference t - t0 exact), the shape from np.interp on phi / (w / 2) over np.linspace(-1, 1, S), zero outside.
    One series and a shared bank: (N, K)."""
    S = shapes.shape[-1]
    out = np.empty((len(t), len(trials)))
    nodes = np.linspace(-1.0, 1.0, S)
    for k, (P, t0, w, s) in enumerate(trials):
        x = t.astype(np.longdouble) - np.longdouble(t0)
        if P > 0:
            x = x - np.rint(x / np.longdouble(P)) * np.longdouble(P)
        xi = (x / (np.longdouble(w) / 2)).astype(float)
        out[:, k] = np.interp(xi, nodes, shapes[int(s)], left=0.0, right=0.0)
    return out


def whitened_shapes(t, c, U, W, d, Z0, trials, shapes):
    """The sweep in the kernel's order for one series, the trials (the lanes) along a numpy axis: one state, nothing stored
    per row, rows 0 .. N-1; row 0 takes the general step with p = 1 and w_{-1} z_{-1} = 0; f^T u_n in four interleaved
    partial sums; z scaled by a reciprocal of d_n once, then multiplied.  The staged blocks move data only.
    Returns T (K, 1 + Q0)."""
    N, J = U.shape
    Q0, nk = Z0.shape[1], len(trials)
    b = column(t, trials, shapes)
    F = np.zeros((J, nk))
    T = np.zeros((nk, 1 + Q0))
    wprev, z, tprev = np.zeros(J), np.zeros(nk), t[0]
    with np.errstate(all="ignore"):
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


def whitened_shapes_batched(t, c, U, W, d, Z0, trials, shapes):
    """`whitened_shapes` for a whole batch at once: t (B, N), c (B, J), U, W (B, N, J), d (B, N), Z0 (B, N, Q0), trials
    (B, K, 4), shapes (NS, S) | (B, NS, S) -> (B, K, 1 + Q0).  The same statements with a leading axis (f^T u_n in one sum:
    the order inside a row is below the criterion)."""
    B, N, J = U.shape
    Q0, nk = Z0.shape[2], trials.shape[1]
    b = column(t, trials, shapes)                          # (B, N, K)
    F = np.zeros((B, J, nk))
    T = np.zeros((B, nk, 1 + Q0))
    wprev, z, tprev = np.zeros((B, J)), np.zeros((B, nk)), t[:, 0]
    with np.errstate(all="ignore"):
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


def projections(t, alpha, trials, shapes):
    """P (K, 1, R) = sum_n b_k(t_n) alpha[n, r] for one series: t (N,), alpha (N, R).  The sum in np.longdouble."""
    col = column(t, trials, shapes).astype(np.longdouble)                    # (N, K)
    with np.errstate(all="ignore"):
        return np.einsum("nk,nr->kr", col, alpha.astype(np.longdouble)).astype(float)[:, None, :]


def projections_batched(t, alpha, trials, shapes):
    """(B, K, 1, R) for alpha (B, N, R); t (N,) | (B, N), trials and the bank shared or per series."""
    B = alpha.shape[0]
    return np.stack([projections(t[b] if t.ndim == 2 else t, alpha[b], trials[b] if trials.ndim == 3 else trials,
                                 shapes[b] if shapes.ndim == 3 else shapes) for b in range(B)])


def dense_products(K, t, Y0, trials, shapes):
    """T (K, 1 + Q0) from dense algebra: the products of every trial's column, built the independent way, and of
    Y0 = L Z0 under K^-1."""
    Bm = column_independent(t, trials, shapes)
    KiB = np.linalg.solve(K, Bm)
    return np.concatenate([(Bm * KiB).sum(0)[:, None], KiB.T @ Y0], axis=1)


def dense_search(K, t, A0, y, trials, shapes):
    """Two dense generalized-least-squares fits per trial, sharing no formula with the package: chi2 of y on A0 (N, P0; P0
    may be 0) and on [A0 | b_k], and the variance of the amplitude from the inverse of the whitened normal matrix.  Returns
    (dchi2 (K,), amplitude (K,), amplitude_err (K,), chi2_null)."""
    Lc = np.linalg.cholesky(K)
    chi2_0, _ = _chi2(Lc, A0, y)
    Bm = column_independent(t, trials, shapes)
    dchi2, amp, aerr = np.empty(len(trials)), np.empty(len(trials)), np.empty(len(trials))
    for k in range(len(trials)):
        X = np.concatenate([A0, Bm[:, k:k + 1]], axis=1)
        chi2_1, beta = _chi2(Lc, X, y)
        Xw = np.linalg.solve(Lc, X)
        cov = np.linalg.inv(Xw.T @ Xw)
        dchi2[k], amp[k], aerr[k] = chi2_0 - chi2_1, beta[-1], np.sqrt(cov[-1, -1])
    return dchi2, amp, aerr, chi2_0


def bank(NS=3, S=9, seed=0):
    """(NS, S) ASYMMETRIC shapes: shape 0 a skewed bump with zero edges, the others random positive profiles with unequal
    ends, so that a left / right or a shape mix-up moves every product."""
    rng = np.random.default_rng(1000 + seed)
    x = np.linspace(0.0, 1.0, S)
    out = [np.sin(np.pi * x ** 0.6) * (1.0 + 0.5 * x)]
    for n in range(1, NS):
        out.append(rng.uniform(0.2, 1.0, S) * (1.0 + n * x))
    out = np.array(out)
    return out / out.max(axis=1, keepdims=True)


def trials_for(t, K=65, NS=1, seed=0, kinds=("fold-box", "single-box"), **kw):
    """(K, 4) trials (P, t0, w, s) with both edges of every event at midpoints between neighbouring (folded) sample distances
    (transit_ref.trials_for's boxes), the shape index rotating lane by lane over the bank."""
    out = TR.trials_for(t, K, kinds=kinds, seed=seed, **kw)
    assert np.all(out[:, 3] == 0.0)
    out[:, 3] = np.arange(K) % NS
    return out


def counts(t, trials):
    """(samples inside the event, samples outside it) per trial, by the rule's u."""
    inside = column(t, trials, np.ones((1, 2))) > 0
    return inside.sum(axis=0), (~inside).sum(axis=0)


def case(seed, N, J, P0=1, K=65, NS=3, S=9, shift=0.0, **kw):
    """One series: draw's dict with d, W (its factors), A0 = design(t, P0) (N, P0; a constant first column), Y0 = [A0 | y],
    Z0 = L^-1 Y0, an asymmetric bank and the midpoint-edge trials.  shift: added to every time before anything is made of
    them (the celerite matrices depend on differences only)."""
    D = draw(seed, N, J)
    D["t"] = D["t"] + shift
    D["d"], D["W"] = factor(D["t"], D["c"], D["a"], D["U"], D["V"])
    D["A0"] = design(D["t"], P0) if P0 else np.zeros((N, 0))
    D["Y0"] = np.concatenate([D["A0"], D["y"][:, None]], axis=1)
    D["Z0"] = sweep(D["t"], D["c"], D["U"], D["W"], D["Y0"])[0]
    D["shapes"] = bank(NS, S, seed)
    D["trials"] = trials_for(D["t"], K, NS, seed=seed, **kw)
    return D
