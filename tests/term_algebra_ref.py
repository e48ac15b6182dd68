# -*- coding: utf-8 -*-
"""TEST INFRASTRUCTURE: a complex-safe numpy restatement of the term ALGEBRA -- "expression -> celerite coefficients and
diagonal shift" (the reference's python/celerite2/terms.py:238-301 TermProduct, 304-330 TermDiff, 350-410 TermConvolution,
on top of the leaves of tests/term_params_ref.py) -- and, next to it, the hand-written reverse the device kernel
c2_term_expr_coefficients_rev implements.  The forward is written in real-analytic operations only (complex numbers of
the convolution as pairs), so oracle.exact-style complex steps of it give the exact Jacobian.  Reads nothing outside
the repository.

An expression is (records, operations): the leaf records of term_params_ref, then operations in post-order, plain dicts
    op   "sum" | "product" | "diff" | "convolve"
    a, b operands: 4-tuples (r0, nr, c0, nc) of REGISTERS -- real registers hold (ar, cr), complex ones (ac, bc, cc, dc);
         the leaves fill registers [0, Jr) / [0, Jc) in program order, every operation appends its result (`out`)
    col  convolve only: the column of P that holds delta
exactly what ops.TermExpr(records, operations, NP).records / .operations hold.  `resolve` fills in `out` (and turns an
integer operand i into the result of operation i) for expressions written by hand."""
import numpy as np

import term_params_ref as R


def resolve(records, operations):
    """operations with a / b given as ranges or as indices of earlier operations -> with a, b, out as ranges."""
    nr = sum(R.widths(r)[0] for r in records)
    nc = sum(R.widths(r)[1] for r in records)
    done = []
    for o in operations:
        rng = []
        for key in ("a", "b"):
            v = o.get(key)
            if v is None:
                v = (0, 0, 0, 0)
            elif isinstance(v, int):
                v = done[v]["out"]
            rng.append(tuple(v))
        a, b = rng
        if o["op"] == "sum":
            wr, wc = a[1] + b[1], a[3] + b[3]
        elif o["op"] == "product":
            wr, wc = a[1] * b[1], a[1] * b[3] + b[1] * a[3] + 2 * a[3] * b[3]
        else:
            wr, wc = a[1], a[3]
        done.append(dict(op=o["op"], a=a, b=b, out=(nr, wr, nc, wc), col=o.get("col", -1)))
        nr, nc = nr + wr, nc + wc
    return done


def _registers(records, P):
    co = R.coefficients(records, P)
    Rr = [(co[0][..., j], co[1][..., j]) for j in range(co[0].shape[-1])]
    Cr = [tuple(co[i][..., j] for i in range(2, 6)) for j in range(co[2].shape[-1])]
    return Rr, Cr


def _forward(records, operations, P):
    """All registers after the forward walk, and the shift."""
    P = np.asarray(P)
    Rr, Cr = _registers(records, P)
    shift = np.zeros(P.shape[:-1], dtype=P.dtype)
    for o in operations:
        (ar0, anr, ac0, anc), (br0, bnr, bc0, bnc) = o["a"], o["b"]
        A_r, A_c = Rr[ar0:ar0 + anr], Cr[ac0:ac0 + anc]
        B_r, B_c = Rr[br0:br0 + bnr], Cr[bc0:bc0 + bnc]
        assert o["out"][0] == len(Rr) and o["out"][2] == len(Cr)
        if o["op"] == "sum":
            Rr += A_r + B_r
            Cr += A_c + B_c
        elif o["op"] == "product":
            for aj, cj in A_r:
                for ak, ck in B_r:
                    Rr.append((aj * ak, cj + ck))
            for X, Y in ((A_r, B_c), (B_r, A_c)):
                for aj, cj in X:
                    for ak, bk, ck, dk in Y:
                        Cr.append((aj * ak, aj * bk, cj + ck, dk))
            for aj, bj, cj, dj in A_c:
                for ak, bk, ck, dk in B_c:
                    Cr.append((0.5 * (aj * ak + bj * bk), 0.5 * (bj * ak - aj * bk), cj + ck, dj - dk))
                    Cr.append((0.5 * (aj * ak - bj * bk), 0.5 * (bj * ak + aj * bk), cj + ck, dj + dk))
        elif o["op"] == "diff":
            for a, c in A_r:
                Rr.append((-a * c**2, c))
            for a, b, c, d in A_c:
                q = (d - c) * (d + c)   # d^2 - c^2 without the cancellation of two rounded squares, as the kernel forms it
                Cr.append((a * q + 2 * b * c * d, b * q - 2 * a * c * d, c, d))
        elif o["op"] == "convolve":   # (a - i b) <- (a - i b) F(z), shift += Re (a - i b) G(z), z = (c - i d) delta
            dt = P[..., o["col"]]
            for a, c in A_r:
                (Fr, _), (Gr, _) = conv_FG_pairs(c * dt, 0.0 * c)
                Rr.append((a * Fr, c))
                shift = shift + a * Gr
            for a, b, c, d in A_c:
                F, G = conv_FG_pairs(c * dt, -d * dt)
                w = _pmul((a, -b), F)
                Cr.append((w[0], -w[1], c, d))
                shift = shift + _pmul((a, -b), G)[0]
        else:
            raise ValueError(o["op"])
    return Rr, Cr, shift


def result_range(records, operations):
    if operations:
        return operations[-1]["out"]
    return (0, sum(R.widths(r)[0] for r in records), 0, sum(R.widths(r)[1] for r in records))


def coefficients(expr, P):
    """P (..., NP), real or complex -> (ar, cr, ac, bc, cc, dc, shift): (..., Jr | Jc) and (...,)."""
    records, operations = expr
    P = np.asarray(P)
    Rr, Cr, shift = _forward(records, operations, P)
    r0, nr, c0, nc = result_range(records, operations)
    st = lambda v: np.stack(v, axis=-1) if v else np.empty(P.shape[:-1] + (0,), dtype=P.dtype)
    out = [st([Rr[r0 + j][f] for j in range(nr)]) for f in range(2)]
    out += [st([Cr[c0 + j][f] for j in range(nc)]) for f in range(4)]
    return tuple(out) + (shift,)


def kappa(expr, P):
    """The loss of relative accuracy of the reference's convolution formulas, max over the convolved terms of 2 / |z|^2 with
    z = (c + i d) delta (cosh z - 1 ~ z^2 / 2: a perturbation eps of cosh z is eps cosh z / (cosh z - 1) of the result);
    1 without a convolution.  Per series: shape P.shape[:-1]."""
    records, operations = expr
    P = np.asarray(P, dtype=np.float64)
    k = np.ones(P.shape[:-1])
    if operations and operations[-1]["op"] == "convolve":
        o = operations[-1]
        Rr, Cr, _ = _forward(records, operations[:-1], P)
        dt = P[..., o["col"]]
        for _, c in Rr[o["a"][0]:o["a"][0] + o["a"][1]]:
            k = np.maximum(k, 2.0 / (c * dt) ** 2)
        for _, _, c, d in Cr[o["a"][2]:o["a"][2] + o["a"][3]]:
            k = np.maximum(k, 2.0 / ((c * c + d * d) * dt * dt))
    return k


# ---- the two functions of the convolution ------------------------------------------------------------------------------
# F(z) = 2 (cosh z - 1) / z^2 and G(z) = 2 (z - sinh z) / z^2 at z = x + i y.  The reference's closed forms lose 2 / |z|^2
# in relative accuracy at small z (their derivatives more), so below |z| = 1/2 the power series are summed, as the device
# kernel does.  The forward needs them COMPLEX-STEP SAFE: x and y may themselves carry a complex step, so the complex number
# z is a PAIR (x, y) with the arithmetic written out in real-analytic operations; the choice of branch looks at real parts.
SERIES = 9
_FK = [2.0 / float(np.prod(np.arange(1, 2 * k + 3, dtype=np.float64))) for k in range(SERIES)]        # 2 / (2k+2)!
_GK = [-2.0 / float(np.prod(np.arange(1, 2 * k + 4, dtype=np.float64))) for k in range(SERIES)]       # -2 / (2k+3)!
_DFK = [2.0 * (k + 1) * 2.0 / float(np.prod(np.arange(1, 2 * k + 5, dtype=np.float64))) for k in range(SERIES)]


def _pmul(u, v):
    return u[0] * v[0] - u[1] * v[1], u[0] * v[1] + u[1] * v[0]


def _pdiv(u, v):
    n = v[0] * v[0] + v[1] * v[1]
    return (u[0] * v[0] + u[1] * v[1]) / n, (u[1] * v[0] - u[0] * v[1]) / n


def conv_FG_pairs(x, y):
    """(F, G) at z = x + i y, each a pair (real part, imaginary part); analytic in x and y."""
    z = (x, y)
    w = _pmul(z, z)
    f, g = (0.0 * x, 0.0 * x), (0.0 * x, 0.0 * x)
    for k in range(SERIES - 1, -1, -1):
        f = _pmul(f, w); f = (f[0] + _FK[k], f[1])
        g = _pmul(g, w); g = (g[0] + _GK[k], g[1])
    g = _pmul(z, g)
    with np.errstate(all="ignore"):
        ch, sh, cy, sy = np.cosh(x), np.sinh(x), np.cos(y), np.sin(y)
        F = _pdiv((2 * (ch * cy - 1), 2 * sh * sy), w)
        G = _pdiv((2 * (x - sh * cy), 2 * (y - ch * sy)), w)
    small = np.real(x) ** 2 + np.real(y) ** 2 < 0.25
    pick = lambda u, v: (np.where(small, u[0], v[0]), np.where(small, u[1], v[1]))
    return pick(f, F), pick(g, G)


# ---- the hand-written reverse (real parameters, numpy complex numbers for the convolution: what the device kernel does) ----
def _conv_fg(z):
    """F, G, F', G' at complex z: series below |z| = 1/2, closed forms F' = 2 sinh z / z^2 - 2 F / z, G' = -F - 2 G / z above."""
    z = np.asarray(z, dtype=np.complex128)
    w = z * z
    f = g = df = dg = np.zeros_like(z)
    for k in range(SERIES - 1, -1, -1):
        f = f * w + _FK[k]
        g = g * w + _GK[k]
        df = df * w + _DFK[k]
        dg = dg * w + (2 * k + 1) * _GK[k]
    with np.errstate(all="ignore"):
        F = 2 * (np.cosh(z) - 1) / w
        G = 2 * (z - np.sinh(z)) / w
        dF = 2 * np.sinh(z) / w - 2 * F / z
        dG = -F - 2 * G / z
    small = np.abs(z) ** 2 < 0.25
    return np.where(small, f, F), np.where(small, z * g, G), np.where(small, z * df, dF), np.where(small, dg, dG)


def coefficients_rev(expr, P, cots, bshift=None):
    """cots = (bar, bcr, bac, bbc, bcc, bdc), each (B, Jr | Jc), bshift (B,) or None; P (B, NP) real -> bP (B, NP)."""
    records, operations = expr
    P = np.asarray(P, dtype=np.float64)
    B = P.shape[0]
    Rr, Cr, _ = _forward(records, operations, P)
    gR = [[np.zeros(B), np.zeros(B)] for _ in Rr]
    gC = [[np.zeros(B) for _ in range(4)] for _ in Cr]
    r0, nr, c0, nc = result_range(records, operations)
    for j in range(nr):
        gR[r0 + j][0] += cots[0][:, j]; gR[r0 + j][1] += cots[1][:, j]
    for j in range(nc):
        for f in range(4):
            gC[c0 + j][f] += cots[2 + f][:, j]
    gs = np.zeros(B) if bshift is None else np.asarray(bshift, dtype=np.float64)
    for o in reversed(operations):
        (ar0, anr, ac0, anc), (br0, bnr, bc0, bnc), (dr0, _, dc0, _) = o["a"], o["b"], o["out"]
        if o["op"] == "sum":
            for j in range(anr):
                for f in range(2):
                    gR[ar0 + j][f] += gR[dr0 + j][f]
            for j in range(bnr):
                for f in range(2):
                    gR[br0 + j][f] += gR[dr0 + anr + j][f]
            for j in range(anc):
                for f in range(4):
                    gC[ac0 + j][f] += gC[dc0 + j][f]
            for j in range(bnc):
                for f in range(4):
                    gC[bc0 + j][f] += gC[dc0 + anc + j][f]
        elif o["op"] == "product":
            q = dr0
            for j in range(anr):
                for k in range(bnr):
                    ga, gc = gR[q]
                    gR[ar0 + j][0] += ga * Rr[br0 + k][0]; gR[br0 + k][0] += ga * Rr[ar0 + j][0]
                    gR[ar0 + j][1] += gc; gR[br0 + k][1] += gc
                    q += 1
            q = dc0
            for (xr0, xnr), (yc0, ync) in (((ar0, anr), (bc0, bnc)), ((br0, bnr), (ac0, anc))):
                for j in range(xnr):
                    for k in range(ync):
                        ga, gb, gc, gd = gC[q]
                        aj = Rr[xr0 + j][0]
                        gR[xr0 + j][0] += ga * Cr[yc0 + k][0] + gb * Cr[yc0 + k][1]
                        gR[xr0 + j][1] += gc
                        gC[yc0 + k][0] += ga * aj; gC[yc0 + k][1] += gb * aj
                        gC[yc0 + k][2] += gc; gC[yc0 + k][3] += gd
                        q += 1
            for j in range(anc):
                for k in range(bnc):
                    aj, bj = Cr[ac0 + j][:2]
                    ak, bk = Cr[bc0 + k][:2]
                    (ga0, gb0, gc0, gd0), (ga1, gb1, gc1, gd1) = gC[q], gC[q + 1]
                    gC[ac0 + j][0] += 0.5 * ((ga0 + ga1) * ak + (gb1 - gb0) * bk)
                    gC[ac0 + j][1] += 0.5 * ((ga0 - ga1) * bk + (gb0 + gb1) * ak)
                    gC[bc0 + k][0] += 0.5 * ((ga0 + ga1) * aj + (gb0 + gb1) * bj)
                    gC[bc0 + k][1] += 0.5 * ((ga0 - ga1) * bj + (gb1 - gb0) * aj)
                    gC[ac0 + j][2] += gc0 + gc1; gC[bc0 + k][2] += gc0 + gc1
                    gC[ac0 + j][3] += gd0 + gd1; gC[bc0 + k][3] += gd1 - gd0
                    q += 2
        elif o["op"] == "diff":
            for j in range(anr):
                a, c = Rr[ar0 + j]
                ga, gc = gR[dr0 + j]
                gR[ar0 + j][0] += -ga * c**2
                gR[ar0 + j][1] += gc - 2 * a * c * ga
            for j in range(anc):
                a, b, c, d = Cr[ac0 + j]
                ga, gb, gc, gd = gC[dc0 + j]
                q, m = (d - c) * (d + c), 2 * c * d
                gC[ac0 + j][0] += ga * q - gb * m
                gC[ac0 + j][1] += ga * m + gb * q
                gC[ac0 + j][2] += gc + 2 * (ga * (b * d - a * c) - gb * (b * c + a * d))
                gC[ac0 + j][3] += gd + 2 * (ga * (a * d + b * c) + gb * (b * d - a * c))
        elif o["op"] == "convolve":
            dt = P[:, o["col"]]
            for j in range(anr):
                a, c = Rr[ar0 + j]
                F, G, dF, dG = (v.real for v in _conv_fg(c * dt))
                ga, gc = gR[dr0 + j]
                gR[ar0 + j][0] += ga * F + gs * G
                gR[ar0 + j][1] += gc + dt * a * (ga * dF + gs * dG)
            for j in range(anc):
                a, b, c, d = Cr[ac0 + j]
                F, G, dF, dG = _conv_fg((c - 1j * d) * dt)
                al = a - 1j * b
                ga, gb, gc, gd = gC[dc0 + j]
                gw = ga - 1j * gb
                gal = np.conj(F) * gw + np.conj(G) * gs
                gz = np.conj(al * dF) * gw + np.conj(al * dG) * gs
                gC[ac0 + j][0] += gal.real; gC[ac0 + j][1] -= gal.imag
                gC[ac0 + j][2] += gc + dt * gz.real; gC[ac0 + j][3] += gd - dt * gz.imag
    Jr, Jc = sum(R.widths(r)[0] for r in records), sum(R.widths(r)[1] for r in records)
    st = lambda v: np.stack(v, axis=-1) if v else np.empty((B, 0))
    leaf_cots = [st([gR[j][f] for j in range(Jr)]) for f in range(2)] + [st([gC[j][f] for j in range(Jc)]) for f in range(4)]
    return R.coefficients_rev(records, P, leaf_cots)


def exact_jacobian(expr, P, cots, bshift, h=1e-30):
    """d/dP of sum(cots * coefficients) + bshift * shift by complex step, series by series: (B, NP)."""
    P = np.asarray(P, dtype=np.float64)

    def f(Pc):
        co = coefficients(expr, Pc)
        return sum(np.sum(g * c, axis=-1) for g, c in zip(cots, co[:6])) + bshift * co[6]

    want = np.empty_like(P)
    for k in range(P.shape[1]):
        d = np.zeros(P.shape[1]); d[k] = 1.0
        want[:, k] = np.imag(f(P + 1j * h * d)) / h
    return want


def zero_inactive_rate_cotangents(expr, P, cots):
    """term_params_ref.zero_inactive_rate_cotangents for an expression: random RESULT cotangents are arbitrary in the
    amplitudes, but what the likelihood sends to a rate is proportional to that term's amplitude -- so the rate cotangent
    of every result term whose amplitudes are exactly zero (it descends from the inactive side of a mixed SHO) is zero."""
    co = coefficients(expr, np.asarray(P, dtype=np.float64))
    cots = [np.array(c) for c in cots]
    cots[1][co[0] == 0.0] = 0.0
    dead = (co[2] == 0.0) & (co[3] == 0.0)
    cots[4][dead] = 0.0
    cots[5][dead] = 0.0
    return cots


# ---- cases and draws the CPU and the GPU tests share ------------------------------------------------------------------------
DELTA, DELTA_BIG = 0.05, 0.08


def build_cases(T, v):
    """The fourteen fixture kernels from the term classes `T`; v(x) wraps every parameter (float, or tensor for the device)."""
    sho = lambda: T.SHOTerm(S0=v(5.0), w0=v(0.8), Q=v(3.45), regime="under")
    sho2 = lambda: T.SHOTerm(sigma=v(1.2), rho=v(2.5), Q=v(1.7), regime="under")
    over = lambda: T.SHOTerm(S0=v(1.2), w0=v(0.3), Q=v(0.1), regime="over")
    real = lambda: T.RealTerm(a=v(1.3), c=v(0.4))
    mat = lambda: T.Matern32Term(sigma=v(0.5), rho=v(2.0))
    rot = lambda: T.RotationTerm(sigma=v(1.5), period=v(3.45), Q0=v(1.3), dQ=v(1.05), f=v(0.5))
    return {
        "prod_sho_real": lambda: sho() * real(),
        "prod_sho_sho": lambda: sho() * sho2(),
        "prod_over_mat": lambda: over() * mat(),
        "prod_of_sums": lambda: (sho() + real()) * (mat() + real()),
        "prod_rot_real": lambda: rot() * real(),
        "nested": lambda: (sho() * real()) * sho2() + real(),
        "diff_sho": lambda: T.TermDiff(sho()),
        "diff_mat": lambda: T.TermDiff(mat()),
        "diff_rot_plus": lambda: T.TermDiff(rot()) + real(),
        "conv_sho": lambda: T.TermConvolution(sho(), DELTA),
        "conv_over": lambda: T.TermConvolution(over(), DELTA),
        "conv_sum": lambda: T.TermConvolution(sho() + real(), DELTA),
        "conv_prod": lambda: T.TermConvolution(sho() * real() + mat(), DELTA),
        "conv_big": lambda: T.TermConvolution(sho() + real(), DELTA_BIG),
        "w8": lambda: (sho() + sho2()) * sho(),        # not a fixture: width 8, for the lane mappings that need it
    }


CASES = ["prod_sho_real", "prod_sho_sho", "prod_over_mat", "prod_of_sums", "prod_rot_real", "nested", "diff_sho", "diff_mat",
         "diff_rot_plus", "conv_sho", "conv_over", "conv_sum", "conv_prod", "conv_big"]


def join(*draws):
    """Several (records, P) of term_params_ref.draw side by side: columns renumbered, P concatenated."""
    records, cols, at = [], [], 0
    for recs, P in draws:
        for r in recs:
            records.append(dict(r, cols=tuple(c + at for c in r["cols"])))
        cols.append(P)
        at += P.shape[1]
    return records, np.concatenate(cols, axis=1)


def leaf_range(records, i):
    """The register range of leaf record i."""
    w = [R.widths(r) for r in records]
    return (sum(x[0] for x in w[:i]), w[i][0], sum(x[1] for x in w[:i]), w[i][1])


LEAVES = {"real": dict(kind="real"), "complex": dict(kind="complex"), "matern32": dict(kind="matern32"),
          "rotation": dict(kind="rotation"), "under": dict(kind="sho", par=R.SIGMA | R.RHO, regime="under"),
          "over": dict(kind="sho", par=R.TAU, regime="over"), "mixed": dict(kind="sho", par=0, regime="mixed")}


def draw_leaf(name, rng, n):
    return R.draw(rng=rng, n=n, **LEAVES[name])


def draw_delta(rng, n):
    return rng.uniform(0.01, 0.6, n)[:, None]     # both sides of the series / closed-form switch for the rates drawn


def draw_operation(op, x, y, rng, n):
    """(expr, P) for one operation on one or two drawn leaves."""
    if op == "product":
        records, P = join(draw_leaf(x, rng, n), draw_leaf(y, rng, n))
        ops_ = [dict(op="product", a=leaf_range(records, 0), b=leaf_range(records, 1))]
    elif op == "diff":
        records, P = draw_leaf(x, rng, n)
        if x == "complex":
            # The derivative's amplitudes a (d^2 - c^2) + 2 b c d and b (d^2 - c^2) - 2 a c d are differences once d < c, and
            # term_params_ref.draw lets c (up to 0.3) exceed d (from 0.2): one draw in a few thousand then sits on a zero of
            # the first amplitude, where ITS condition number (sum of |terms| / |result|, 2.7e3 in the draw that showed it)
            # decides how far two correctly rounded evaluation orders part -- no property of either.  Comparisons at 1e-13
            # (450 roundings) are meaningful for condition numbers of a few: keep d >= 1.5 c (then every term of the first
            # amplitude is positive and the second has condition <= 2.7), with b scaled so that b d / (a c) stays as drawn.
            d = np.maximum(P[:, 3], 1.5 * P[:, 2])
            P[:, 1] *= P[:, 3] / d
            P[:, 3] = d
        ops_ = [dict(op="diff", a=leaf_range(records, 0))]
    else:
        records, P = draw_leaf(x, rng, n)
        P = np.concatenate([P, draw_delta(rng, n)], axis=1)
        ops_ = [dict(op="convolve", a=leaf_range(records, 0), col=P.shape[1] - 1)]
    return (records, resolve(records, ops_)), P


PRODUCTS = [("real", "real"), ("real", "complex"), ("under", "real"), ("under", "matern32"), ("over", "rotation"),
            ("complex", "complex"), ("over", "over"), ("rotation", "under")]


def nested_expr(rng, n):
    """conv((sho * real) * sho2 + real + diff(matern32), delta): every operation kind, sums of leaves and of results."""
    records, P = join(draw_leaf("under", rng, n), draw_leaf("real", rng, n), draw_leaf("under", rng, n), draw_leaf("real", rng, n),
                      draw_leaf("matern32", rng, n))
    P = np.concatenate([P, draw_delta(rng, n)], axis=1)
    L = lambda i: leaf_range(records, i)
    ops_ = [dict(op="product", a=L(0), b=L(1)), dict(op="product", a=0, b=L(2)), dict(op="sum", a=1, b=L(3)),
            dict(op="diff", a=L(4)), dict(op="sum", a=2, b=3), dict(op="convolve", a=4, col=P.shape[1] - 1)]
    return (records, resolve(records, ops_)), P
