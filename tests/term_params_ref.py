# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: a complex-safe numpy restatement of "program -> celerite coefficients" (the reference's
python/celerite2/terms.py:515-521, 554-569, 644-691, 729-745, 791-812) and, next to it, the hand-written reverse the
device kernel c2_term_coefficients_rev implements.  The forward is analytic in P wherever max(., eps) does not switch
(np.maximum is not analytic: it is taken on the real part, and the clamped branch is the constant eps), so
oracle.exact.cstep_grad of it is the exact Jacobian.  Reads nothing outside the repository.

A program is a list of records, plain dicts:
    kind   "real" | "complex" | "sho" | "matern32" | "rotation"
    cols   columns of P the term reads: (a, c) | (a, b, c, d) | (S0|sigma, w0|rho, Q|tau) | (sigma, rho) |
           (sigma, period, Q0, dQ, f)
    par    sho only: bit 0 sigma instead of S0, bit 1 rho instead of w0, bit 2 tau instead of Q
    regime sho only: "under" | "over" | "mixed"
    eps    sho, rotation (1e-5), matern32 (0.01)
Coefficient slots follow program order, reals and complex terms each concatenated (terms.py:233-235)."""
import numpy as np

SIGMA, RHO, TAU = 1, 2, 4


def rec(kind, cols, par=0, regime=None, eps=None):
    if eps is None:
        eps = 0.01 if kind == "matern32" else 1e-5
    return dict(kind=kind, cols=tuple(cols), par=par, regime=regime, eps=eps)


def widths(r):
    """(real slots, complex slots) of one record."""
    if r["kind"] == "real":
        return 1, 0
    if r["kind"] == "sho":
        return {"under": (0, 1), "over": (2, 0), "mixed": (2, 1)}[r["regime"]]
    return (0, 2) if r["kind"] == "rotation" else (0, 1)


def _clamp(g, eps):
    """max(g, eps) with the clamped branch the constant eps (real part decides)."""
    return np.where(np.real(g) > eps, g, eps)


def _sho_params(par, p0, p1, p2):
    w0 = 2 * np.pi / p1 if par & RHO else p1
    Q = 0.5 * w0 * p2 if par & TAU else p2
    S0 = p0**2 / (w0 * Q) if par & SIGMA else p0
    return S0, w0, Q


def _under(S0, w0, Q, eps):
    f = np.sqrt(_clamp(4.0 * Q**2 - 1.0, eps))
    a = S0 * w0 * Q
    c = 0.5 * w0 / Q
    return a, a / f, c, c * f


def _over(S0, w0, Q, eps):
    f = np.sqrt(_clamp(1.0 - 4.0 * Q**2, eps))
    A = 0.5 * S0 * w0 * Q
    C = 0.5 * w0 / Q
    return A * (1.0 + 1.0 / f), A * (1.0 - 1.0 / f), C * (1.0 - f), C * (1.0 + f)


def _rot(sigma, period, Q0, dQ, f):
    amp = sigma**2 / (1 + f)
    Q1 = 0.5 + Q0 + dQ
    w1 = 4 * np.pi * Q1 / (period * np.sqrt(4 * Q1**2 - 1))
    S1 = amp / (w1 * Q1)
    Q2 = 0.5 + Q0
    w2 = 8 * np.pi * Q2 / (period * np.sqrt(4 * Q2**2 - 1))
    S2 = f * amp / (w2 * Q2)
    return amp, (S1, w1, Q1), (S2, w2, Q2)


def coefficients(program, P):
    """P (..., NP), real or complex -> (ar, cr, ac, bc, cc, dc), each (..., Jr | Jc)."""
    P = np.asarray(P)
    col = lambda r, k: P[..., r["cols"][k]]
    R = [[], []]
    C = [[], [], [], []]
    zero = np.zeros(P.shape[:-1], dtype=P.dtype)
    for r in program:
        k = r["kind"]
        if k == "real":
            R[0].append(col(r, 0)); R[1].append(col(r, 1))
        elif k == "complex":
            for i in range(4):
                C[i].append(col(r, i))
        elif k == "sho":
            S0, w0, Q = _sho_params(r["par"], col(r, 0), col(r, 1), col(r, 2))
            un, ov = _under(S0, w0, Q, r["eps"]), _over(S0, w0, Q, r["eps"])
            if r["regime"] == "under":
                for i in range(4):
                    C[i].append(un[i])
            elif r["regime"] == "over":
                R[0] += [ov[0], ov[1]]; R[1] += [ov[2], ov[3]]
            else:
                over = np.real(Q) < 0.5
                rate = 0.5 * w0 / Q
                R[0] += [np.where(over, ov[0], zero), np.where(over, ov[1], zero)]
                R[1] += [np.where(over, ov[2], rate), np.where(over, ov[3], rate)]
                C[0].append(np.where(over, zero, un[0])); C[1].append(np.where(over, zero, un[1]))
                C[2].append(np.where(over, rate, un[2])); C[3].append(np.where(over, zero, un[3]))
        elif k == "matern32":
            sigma, rho, eps = col(r, 0), col(r, 1), r["eps"]
            w0 = np.sqrt(3.0) / rho
            S0 = sigma**2 / w0
            C[0].append(w0 * S0); C[1].append(w0 * w0 * S0 / eps); C[2].append(w0); C[3].append(zero + eps)
        elif k == "rotation":
            _, s1, s2 = _rot(*(col(r, i) for i in range(5)))
            for s in (s1, s2):
                un = _under(*s, r["eps"])
                for i in range(4):
                    C[i].append(un[i])
        else:
            raise ValueError(k)
    st = lambda v: np.stack(v, axis=-1) if v else np.empty(P.shape[:-1] + (0,), dtype=P.dtype)
    return tuple(st(v) for v in R + C)


# ---- the hand-written reverse (real arithmetic; what the device kernel does) ----------------------------------------------
def _under_rev(S0, w0, Q, eps, ga, gb, gc, gd):
    g = 4.0 * Q**2 - 1.0
    f = np.sqrt(np.maximum(g, eps))
    a, c = S0 * w0 * Q, 0.5 * w0 / Q
    ba = ga + gb / f
    bc = gc + gd * f
    bf = gd * c - gb * a / f**2
    bS0 = ba * w0 * Q
    bw0 = ba * S0 * Q + bc * 0.5 / Q
    bQ = ba * S0 * w0 - bc * c / Q + np.where(g > eps, bf * 4.0 * Q / f, 0.0)
    return bS0, bw0, bQ


def _over_rev(S0, w0, Q, eps, ga0, ga1, gc0, gc1):
    g = 1.0 - 4.0 * Q**2
    f = np.sqrt(np.maximum(g, eps))
    A, C = 0.5 * S0 * w0 * Q, 0.5 * w0 / Q
    bA = ga0 * (1.0 + 1.0 / f) + ga1 * (1.0 - 1.0 / f)
    bC = gc0 * (1.0 - f) + gc1 * (1.0 + f)
    bf = A * (ga1 - ga0) / f**2 + C * (gc1 - gc0)
    bS0 = bA * 0.5 * w0 * Q
    bw0 = bA * 0.5 * S0 * Q + bC * 0.5 / Q
    bQ = bA * 0.5 * S0 * w0 - bC * C / Q - np.where(g > eps, bf * 4.0 * Q / f, 0.0)
    return bS0, bw0, bQ


def coefficients_rev(program, P, cots):
    """cots = (bar, bcr, bac, bbc, bcc, bdc), each (B, Jr | Jc); P (B, NP) real -> bP (B, NP)."""
    P = np.asarray(P, dtype=np.float64)
    bar, bcr, bac, bbc, bcc, bdc = cots
    bP = np.zeros_like(P)
    jr = jc = 0
    for r in program:
        k, cols = r["kind"], r["cols"]
        p = [P[:, c] for c in cols]
        if k == "real":
            bP[:, cols[0]] += bar[:, jr]; bP[:, cols[1]] += bcr[:, jr]
        elif k == "complex":
            for i, g in enumerate((bac, bbc, bcc, bdc)):
                bP[:, cols[i]] += g[:, jc]
        elif k == "sho":
            par = r["par"]
            S0, w0, Q = _sho_params(par, *p)
            if r["regime"] != "over":
                un = _under_rev(S0, w0, Q, r["eps"], bac[:, jc], bbc[:, jc], bcc[:, jc], bdc[:, jc])
            if r["regime"] != "under":
                ov = _over_rev(S0, w0, Q, r["eps"], bar[:, jr], bar[:, jr + 1], bcr[:, jr], bcr[:, jr + 1])
            if r["regime"] == "under":
                bS0, bw0, bQ = un
            elif r["regime"] == "over":
                bS0, bw0, bQ = ov
            else:   # the inactive side's cotangents are ignored
                bS0, bw0, bQ = (np.where(Q < 0.5, o, u) for o, u in zip(ov, un))
            g0 = bS0
            if par & SIGMA:
                g0 = bS0 * 2.0 * p[0] / (w0 * Q)
                bw0 = bw0 - bS0 * S0 / w0
                bQ = bQ - bS0 * S0 / Q
            g2 = bQ
            if par & TAU:
                g2 = bQ * 0.5 * w0
                bw0 = bw0 + bQ * 0.5 * p[2]
            g1 = -bw0 * w0 / p[1] if par & RHO else bw0
            for i, g in enumerate((g0, g1, g2)):
                bP[:, cols[i]] += g
        elif k == "matern32":
            sigma, rho, eps = p[0], p[1], r["eps"]
            w0 = np.sqrt(3.0) / rho
            S0 = sigma**2 / w0
            bS0 = bac[:, jc] * w0 + bbc[:, jc] * w0 * w0 / eps
            bw0 = bac[:, jc] * S0 + bbc[:, jc] * 2.0 * w0 * S0 / eps + bcc[:, jc] - bS0 * S0 / w0
            bP[:, cols[0]] += bS0 * 2.0 * sigma / w0
            bP[:, cols[1]] -= bw0 * w0 / rho
        elif k == "rotation":
            sigma, period, Q0, dQ, f = p
            amp, (S1, w1, Q1), (S2, w2, Q2) = _rot(*p)
            bS1, bw1, bQ1 = _under_rev(S1, w1, Q1, r["eps"], bac[:, jc], bbc[:, jc], bcc[:, jc], bdc[:, jc])
            bS2, bw2, bQ2 = _under_rev(S2, w2, Q2, r["eps"], bac[:, jc + 1], bbc[:, jc + 1], bcc[:, jc + 1], bdc[:, jc + 1])
            bamp = bS1 / (w1 * Q1) + bS2 * f / (w2 * Q2)
            bf = bS2 * amp / (w2 * Q2)
            bw1 = bw1 - bS1 * S1 / w1; bQ1 = bQ1 - bS1 * S1 / Q1
            bw2 = bw2 - bS2 * S2 / w2; bQ2 = bQ2 - bS2 * S2 / Q2
            g1, g2 = 4 * Q1**2 - 1, 4 * Q2**2 - 1
            bQ1 = bQ1 + bw1 * w1 / Q1 - bw1 * w1 * 4.0 * Q1 / g1
            bQ2 = bQ2 + bw2 * w2 / Q2 - bw2 * w2 * 4.0 * Q2 / g2
            bf = bf - bamp * amp / (1.0 + f)
            bP[:, cols[0]] += bamp * 2.0 * sigma / (1.0 + f)
            bP[:, cols[1]] -= (bw1 * w1 + bw2 * w2) / period
            bP[:, cols[2]] += bQ1 + bQ2
            bP[:, cols[3]] += bQ1
            bP[:, cols[4]] += bf
        wr, wc = widths(r)
        jr += wr; jc += wc
    return bP


def zero_inactive_rate_cotangents(program, P, cots):
    """Random cotangents for a Jacobian check of a MIXED term: what the likelihood sends to the inactive side's RATES is
    proportional to that side's amplitudes, i.e. exactly zero (d k / d cr = -ar tau exp(-cr tau) at ar = 0), and the
    reverse relies on it; the inactive AMPLITUDE cotangents stay arbitrary (they do not vanish, and must not matter)."""
    cots = [np.array(c) for c in cots]
    jr = jc = 0
    for r in program:
        if r["kind"] == "sho" and r["regime"] == "mixed":
            Q = _sho_params(r["par"], *(np.asarray(P)[:, c] for c in r["cols"]))[2]
            over = Q < 0.5
            cots[1][~over, jr] = 0.0; cots[1][~over, jr + 1] = 0.0
            cots[4][over, jc] = 0.0; cots[5][over, jc] = 0.0
        wr, wc = widths(r)
        jr += wr; jc += wc
    return cots


# the 12 parameter sets of tests/golden/make_golden_ref.py (`coef_cases`), as (program, P)
GOLDEN_CASES = {
    "real": ([rec("real", (0, 1))], [1.3, 0.4]),
    "complex": ([rec("complex", (0, 1, 2, 3))], [0.8, 0.03, 1.0, 0.1]),
    "sho_under": ([rec("sho", (0, 1, 2), regime="under")], [5.0, 0.1, 3.45]),
    "sho_over": ([rec("sho", (0, 1, 2), regime="over")], [1.2, 0.3, 0.1]),
    "sho_near_half_lo": ([rec("sho", (0, 1, 2), regime="over")], [1.0, 1.0, 0.5 - 1e-9]),
    "sho_near_half_hi": ([rec("sho", (0, 1, 2), regime="under")], [1.0, 1.0, 0.5 + 1e-9]),
    "sho_sigma_rho_tau": ([rec("sho", (0, 1, 2), par=SIGMA | RHO | TAU, regime="under")], [1.5, 3.0, 2.0]),
    "sho_sigma_rho_Q": ([rec("sho", (0, 1, 2), par=SIGMA | RHO, regime="over")], [0.7, 1.1, 0.3]),
    "matern32": ([rec("matern32", (0, 1))], [0.5, 2.0]),
    "matern32_eps": ([rec("matern32", (0, 1), eps=1e-3)], [1.5, 0.7]),
    "rotation": ([rec("rotation", range(5))], [1.5, 3.45, 1.3, 1.05, 0.5]),
    "sum": ([rec("sho", (0, 1, 2), regime="under"), rec("real", (3, 4)), rec("matern32", (5, 6))],
            [5.0, 0.1, 3.45, 1.0, 0.1, 0.5, 2.0]),
}


# ---- draws the CPU and the GPU tests share -------------------------------------------------------------------------------
def draw_Q(rng, n, side):
    """Q with |4 Q^2 - 1| >= 0.05 (the cancellation in 4 Q^2 - 1 magnifies a rounding of Q by 1 / |4 Q^2 - 1|)."""
    lo, hi = np.sqrt(0.95) / 2, np.sqrt(1.05) / 2
    under = rng.uniform(hi, 6.0, n)
    over = rng.uniform(0.05, lo, n)
    if side == "under":
        return under
    if side == "over":
        return over
    return np.where(np.arange(n) % 2 == 0, under, over)   # mixed: half each side


def draw(kind, rng, n, par=0, regime=None):
    """(program, P (n, NP)) for one term of `kind`."""
    if kind == "real":
        return [rec("real", (0, 1))], np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(0.05, 0.5, n)], 1)
    if kind == "complex":
        a, c, d = rng.uniform(0.5, 2.0, n), rng.uniform(0.02, 0.3, n), rng.uniform(0.2, 3.0, n)
        return [rec("complex", (0, 1, 2, 3))], np.stack([a, a * c / d * rng.uniform(0, 0.9, n), c, d], 1)
    if kind == "matern32":
        return [rec("matern32", (0, 1))], np.stack([rng.uniform(0.3, 2.0, n), rng.uniform(0.5, 5.0, n)], 1)
    if kind == "rotation":
        cols = [rng.uniform(0.5, 2.0, n), rng.uniform(1.0, 6.0, n), rng.uniform(0.2, 3.0, n), rng.uniform(0.1, 2.0, n),
                rng.uniform(0.1, 1.0, n)]
        return [rec("rotation", range(5))], np.stack(cols, 1)
    assert kind == "sho"
    Q = draw_Q(rng, n, regime)
    w0 = rng.uniform(0.2, 3.0, n)
    S0 = rng.uniform(0.2, 3.0, n)
    p1 = 2 * np.pi / w0 if par & RHO else w0
    p2 = 2 * Q / w0 if par & TAU else Q
    p0 = np.sqrt(S0 * w0 * Q) if par & SIGMA else S0
    return [rec("sho", (0, 1, 2), par=par, regime=regime)], np.stack([p0, p1, p2], 1)
