# -*- coding: utf-8 -*-
"""numpy restatement of the whitened-Keplerian sweep (celerite2_amd/csrc/c2_kepler.hip: trial::k_trial_sweep on trial::Keplerian) and of what it and the torch finish
(celerite2_amd/kepler.py) are checked against: a bracketed extended-precision solution of Kepler's equation, dense algebra on
the matrix the celerite matrices stand for, and two dense generalized-least-squares fits per trial.  Test infrastructure
only -- nothing here is imported by the package.

Notation as linear_model_ref: K + D = L diag(d) L^T, L = I + tril(U W^T o decay), <a, b> = sum_n a_n b_n / d_n.  A trial is
(angular frequency w, eccentricity e, time of periastron tp).  The rule of the public header
(include/celerite2_amd_kepler.h), each line rounded once:

    x = fl(w * fl(t_n - tp));  q = rint(fl(x * INV_2PI));  r = fma(-q, TWO_PI, x) (exact);  a = |r|
    E - e sin E = a by the starter, three Danby steps, a fourth on the rotated pair, the pair rotated once more (solve)
    g = 1 / (1 - e c);  cos nu = (c - e) g;  sin nu = copysign(1, r) sqrt(1 - e^2) s g

    F <- p_n o (F + w_{n-1} z_{n-1}^T)      (F: J x 2, zero at row 0; p_n = exp(-c (t_n - t_{n-1})))
    z_n = (cos nu_n, sin nu_n) - F^T u_n
    T  += [z_c z_c, z_c z_s, z_s z_s, z_c Z0_n, z_s Z0_n] / d_n

Where the kernel fuses a product into an fma and numpy rounds it first, or takes a reciprocal by Newton steps where numpy
divides, the two differ in the last bit: far below the criterion.  The reduction is the exception: r is exact in both.
"""
from fractions import Fraction

import numpy as np

from linear_model_ref import dense, design, draw, err, factor, sweep  # noqa: F401  (re-exported for the tests)
from periodogram_ref import _chi2, null_products  # noqa: F401

TWO_PI = float.fromhex("0x1.921fb54442d18p+2")      # fl(2 pi)
INV_2PI = float.fromhex("0x1.45f306dc9c883p-3")     # fl(1 / fl(2 pi))
MAX_ECC = 0.99
assert TWO_PI == 2.0 * np.pi and INV_2PI == 1.0 / TWO_PI


def reduce(x):
    """r of the header's rule for a float x, in exact rational arithmetic: q = rint(fl(x * INV_2PI)) in double, then
    x - q * TWO_PI as a Fraction, rounded once to double (the fma).  The rounding changes nothing: the value is a double."""
    x = float(x)
    q = float(np.rint(x * INV_2PI))
    return float(Fraction(x) - Fraction(q) * Fraction(TWO_PI))


def _two_prod(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker, Veltkamp's split): the fma's product without an fma."""
    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def reduce_array(x):
    """`reduce` on an array: q TWO_PI as an exact sum of two doubles, x - hi (exact: the two are within a factor of two, or
    hi = 0) and then - lo (exact because the result is a double).  tests/test_kepler.py pins it to `reduce` bit for bit."""
    x = np.asarray(x, dtype=float)
    q = np.rint(x * INV_2PI)
    hi, lo = _two_prod(q, np.full_like(x, TWO_PI))
    return (x - hi) - lo


def _danby(E, a, e, s, c):
    """Danby's quartic step at E with (s, c) = (sin E, cos E)."""
    f = (E - e * s) - a
    f2, f3 = e * s, e * c
    f1 = 1.0 - f3
    d1 = -f * (1.0 / f1)
    d2 = -f * (1.0 / (0.5 * d1 * f2 + f1))
    return -f * (1.0 / (d2 * d2 * (f3 * (1.0 / 6.0)) + (0.5 * d2 * f2 + f1)))


def solve(r, e):
    """The lane's solver, statement by statement: (E, cos nu, sin nu) for the reduced mean anomaly r and the eccentricity e
    (arrays that broadcast).  E carries the sign of r; the kernel never forms the last E, only its sine and cosine."""
    r, e = np.broadcast_arrays(np.asarray(r, dtype=float), np.asarray(e, dtype=float))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b = np.sqrt(1.0 - e * e)
        se, ce = np.sin(e), np.cos(e)
        a = np.abs(r)
        s, c = np.sin(a), np.cos(a)
        sae = s * ce + c * se
        E0, E1 = a + e, e * s * (1.0 / ((1.0 - sae) + s)) + a
        E = np.where(E1 < E0, E1, E0)
        for _ in range(3):
            s, c = np.sin(E), np.cos(E)
            delta = _danby(E, a, e, s, c)
            E = E + delta
        d2 = delta * delta
        sd = delta * (d2 * (d2 * (1.0 / 120.0) - 1.0 / 6.0) + 1.0)
        cd = d2 * (d2 * (1.0 / 24.0) - 0.5) + 1.0
        s, c = s * cd + c * sd, c * cd - s * sd
        delta = _danby(E, a, e, s, c)
        E = E + delta
        s, c = c * delta + s, -s * delta + c
        g = 1.0 / (-e * c + 1.0)
        return np.copysign(1.0, r) * E, (c - e) * g, np.copysign(1.0, r) * ((b * s) * g)


def columns(t, trials):
    """(cos nu, sin nu), each (..., N, K), for t (..., N) and trials (..., K, 3), as the kernel forms them."""
    w, e, tp = [trials[..., None, :, i] for i in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        x = w * (t[..., :, None] - tp)                       # the difference is rounded, then the product
        _, cnu, snu = solve(reduce_array(x), e)
    return cnu, snu


def whitened_keplerians(t, c, U, W, d, Z0, trials):
    """The sweep in the kernel's order for one series, the trials (the lanes) along a numpy axis: one state, nothing stored
    per row, rows 0 .. N-1; row 0 takes the general step with p = 1 and w_{-1} z_{-1} = 0; F^T u_n in four interleaved
    partial sums; z scaled by a reciprocal of d_n once, then multiplied.  The staged blocks move data only.
    Returns T (K, 3 + 2 Q0)."""
    N, J = U.shape
    Q0, nk = Z0.shape[1], len(trials)
    C, S = columns(t, trials)
    Fc, Fs = np.zeros((J, nk)), np.zeros((J, nk))
    T = np.zeros((nk, 3 + 2 * Q0))
    wprev, zc, zs, tprev = np.zeros(J), np.zeros(nk), np.zeros(nk), t[0]
    for n in range(N):
        p = np.exp(c * (tprev - t[n]))
        tprev = t[n]
        Fc = p[:, None] * (Fc + wprev[:, None] * zc[None, :])
        Fs = p[:, None] * (Fs + wprev[:, None] * zs[None, :])
        ac, as_ = np.zeros((4, nk)), np.zeros((4, nk))
        for j in range(J):
            ac[j & 3] += Fc[j] * U[n, j]
            as_[j & 3] += Fs[j] * U[n, j]
        zc = C[n] - ((ac[0] + ac[1]) + (ac[2] + ac[3]))
        zs = S[n] - ((as_[0] + as_[1]) + (as_[2] + as_[3]))
        rd = 1.0 / d[n]
        zcd, zsd = zc * rd, zs * rd
        T[:, 0] += zc * zcd
        T[:, 1] += zcd * zs
        T[:, 2] += zs * zsd
        T[:, 3:3 + Q0] += zcd[:, None] * Z0[n][None, :]
        T[:, 3 + Q0:] += zsd[:, None] * Z0[n][None, :]
        wprev = W[n]
    return T


def whitened_keplerians_batched(t, c, U, W, d, Z0, trials):
    """`whitened_keplerians` for a whole batch at once: t (B, N), c (B, J), U, W (B, N, J), d (B, N), Z0 (B, N, Q0),
    trials (B, K, 3) -> (B, K, 3 + 2 Q0).  The same statements with a leading axis (F^T u_n in one sum: the order inside a
    row is below the criterion)."""
    B, N, J = U.shape
    Q0, nk = Z0.shape[2], trials.shape[1]
    C, S = columns(t, trials)                              # (B, N, K) each
    Fc, Fs = np.zeros((B, J, nk)), np.zeros((B, J, nk))
    T = np.zeros((B, nk, 3 + 2 * Q0))
    wprev, zc, zs, tprev = np.zeros((B, J)), np.zeros((B, nk)), np.zeros((B, nk)), t[:, 0]
    for n in range(N):
        p = np.exp(c * (tprev - t[:, n])[:, None])
        tprev = t[:, n]
        Fc = p[:, :, None] * (Fc + wprev[:, :, None] * zc[:, None, :])
        Fs = p[:, :, None] * (Fs + wprev[:, :, None] * zs[:, None, :])
        zc = C[:, n] - np.einsum("bjk,bj->bk", Fc, U[:, n])
        zs = S[:, n] - np.einsum("bjk,bj->bk", Fs, U[:, n])
        rd = (1.0 / d[:, n])[:, None]
        zcd, zsd = zc * rd, zs * rd
        T[:, :, 0] += zc * zcd
        T[:, :, 1] += zcd * zs
        T[:, :, 2] += zs * zsd
        T[:, :, 3:3 + Q0] += zcd[:, :, None] * Z0[:, n][:, None, :]
        T[:, :, 3 + Q0:] += zsd[:, :, None] * Z0[:, n][:, None, :]
        wprev = W[:, n]
    return T


# ---- independent of the solver under test ---------------------------------------------------------------------------------
def converged(r, e):
    """E with E - e sin E = r by bisection in np.longdouble on [r - e, r + e] (the root lies there: |e sin E| <= e), 90
    halvings.  Shares nothing with `solve`."""
    r, e = np.broadcast_arrays(np.asarray(r, dtype=np.longdouble), np.asarray(e, dtype=np.longdouble))
    lo, hi = r - e, r + e
    for _ in range(90):
        mid = 0.5 * (lo + hi)
        above = mid - e * np.sin(mid) > r
        hi, lo = np.where(above, mid, hi), np.where(above, lo, mid)
    return 0.5 * (lo + hi)


def columns_converged(r, e):
    """(cos nu, sin nu) in np.longdouble from `converged`, by the textbook formulas."""
    e = np.asarray(e, dtype=np.longdouble)
    E = converged(r, e)
    g = 1.0 / (1.0 - e * np.cos(E))
    return (np.cos(E) - e) * g, np.sqrt(1.0 - e * e) * np.sin(E) * g


def columns_independent(t, trials):
    """(cos nu, sin nu), each (N, K) in double, for the dense oracles: the mean anomaly reduced in extended precision by
    2 pi itself (no rint of a double product, no double 2 pi), Kepler's equation by bisection."""
    w, e, tp = [trials[None, :, i] for i in range(3)]
    M = (w * (t[:, None] - tp)).astype(np.longdouble)
    two_pi = 2.0 * np.arctan2(np.longdouble(0.0), np.longdouble(-1.0))
    r = M - two_pi * np.floor(M / two_pi + 0.5)
    C, S = columns_converged(r, e)
    return C.astype(float), S.astype(float)


def dense_products(K, t, Y0, trials):
    """T (K, 3 + 2 Q0) from dense algebra: the products of the two columns of every trial, built the independent way, and of
    Y0 = L Z0 under K^-1."""
    C, S = columns_independent(t, trials)
    KiC, KiS, KiY = np.linalg.solve(K, C), np.linalg.solve(K, S), np.linalg.solve(K, Y0)
    return np.concatenate([np.stack([(C * KiC).sum(0), (C * KiS).sum(0), (S * KiS).sum(0)], axis=1), C.T @ KiY, S.T @ KiY], axis=1)


def dense_keplerian(K, t, A0, y, trials):
    """Two dense generalized-least-squares fits per trial, sharing no formula with the package: chi2 of y on A0 (N, P0; P0
    may be 0) and on [A0 | cos nu | sin nu], the columns from `converged`.  Returns (dchi2 (K,), amplitude (K, 2), chi2_null)."""
    Lc = np.linalg.cholesky(K)
    chi2_0, _ = _chi2(Lc, A0, y)
    C, S = columns_independent(t, trials)
    dchi2, amp = np.empty(len(trials)), np.empty((len(trials), 2))
    for k in range(len(trials)):
        chi2_1, beta = _chi2(Lc, np.concatenate([A0, C[:, k:k + 1], S[:, k:k + 1]], axis=1), y)
        dchi2[k], amp[k] = chi2_0 - chi2_1, beta[-2:]
    return dchi2, amp, chi2_0


def trials_for(t, K=65, seed=0, e_max=MAX_ECC, e_list=(0.0, 1e-9, None, MAX_ECC)):
    """(K, 3) trials on the drawn times: one to eight cycles over the baseline, eccentricities rotating lane by lane through
    `e_list` (None: uniform on [0, e_max)), periastron drawn over three baselines around the series -- inside and outside
    the span."""
    rng = np.random.default_rng(seed)
    span = float(t[-1] - t[0]) if len(t) > 1 and t[-1] > t[0] else 1.0
    w = 2.0 * np.pi / span * rng.uniform(1.0, 8.0, K)
    e = np.array([rng.uniform(0.0, e_max) if e_list[k % len(e_list)] is None else min(e_list[k % len(e_list)], e_max)
                  for k in range(K)])
    tp = rng.uniform(t[0] - span, t[0] + 2.0 * span, K)
    return np.stack([w, e, tp], axis=1)


def case(seed, N, J, P0=1, K=65, **kw):
    """One series: draw's dict with d, W (its factors), A0 = design(t, P0) (N, P0; a constant first column), Y0 = [A0 | y],
    Z0 = L^-1 Y0 and the trials."""
    D = draw(seed, N, J)
    D["d"], D["W"] = factor(D["t"], D["c"], D["a"], D["U"], D["V"])
    D["A0"] = design(D["t"], P0) if P0 else np.zeros((N, 0))
    D["Y0"] = np.concatenate([D["A0"], D["y"][:, None]], axis=1)
    D["Z0"] = sweep(D["t"], D["c"], D["U"], D["W"], D["Y0"])[0]
    D["trials"] = trials_for(D["t"], K, seed=seed, **kw)
    return D
