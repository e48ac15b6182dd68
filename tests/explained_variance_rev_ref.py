# -*- coding: utf-8 -*-
"""numpy restatement of the explained-variance sweep WITH ITS WORKSPACE and of its reverse
(celerite2_amd/csrc/c2_predvar.hip, c2_predvar_rev.hip).  Test infrastructure only -- nothing here is imported by the package.

Notation as predict_at_ref: n(m) is the last data row with t_n <= s_m, -1 in front of the data.

(i)   `forward_ws`: predict_at_ref.explained_variance row by row, keeping X (M, J), Sws[n] = S'_n and Rws[n] = R_n (the state
      AFTER row n's update, in either sweep).  Any dtype: float64, long double, complex (for complex-step derivatives).
(ii)  `reverse_rows`: both reverse passes as per-row loops.
      Pass A undoes the backward sweep, walking upwards with Rb = 0: the queries with n(m) = n - 1, then data row n.
          query:  lag = t_n - s ;  eps = exp(-c lag) ;  x = eps o X_m
                  Rb += br_m x x^T ;  bx = 2 br_m R_n x ;  bVs_m = eps o bx
                  k = x o bx ;  bc -= lag k ;  bt_n -= c.k ;  bts_m += c.k
          data:   p = exp(-c (t_{n+1} - t_n)) ;  G = (p p^T) o R_{n+1}            (n = N - 1: G = 0, p = 1)
                  g = G w ;  q = 1 / d_n + w.g ;  Mu = Rb u ;  qb = u.Mu ;  gb = -2 Mu + qb w
                  bU_n = -2 Rb g + 2 q Mu ;  bd_n = -qb / d_n^2 ;  bW_n = qb g + G gb
                  Gb = Rb + (gb w^T + w gb^T) / 2
                  n < N - 1:  pb = 2 (Gb o R_{n+1}) p ;  k = pb o p ;  bc -= (t_{n+1} - t_n) k ;  bt_{n+1} -= c.k ;  bt_n += c.k
                  Rb <- (p p^T) o Gb
      Pass B undoes the forward sweep, walking downwards with Sb = 0: the queries with n(m) = n (last first), then row n.
          query:  lag = s - t_n ;  e = exp(-c lag) ;  uL = u* o e ;  h = S'_n uL ;  bX = bVs_m
                  bh = br_m uL - e o bX ;  be = -h o bX ;  buL = br_m h + S'_n bh
                  Sb += (bh uL^T + uL bh^T) / 2 ;  bUs_m = e o buL ;  be += u* o buL
                  k = e o be ;  bc -= lag k ;  bts_m -= c.k ;  bt_n += c.k
          data:   bd_n += w^T Sb w ;  bW_n += 2 d_n Sb w
                  n > 0:  p = exp(-c (t_n - t_{n-1})) ;  pb = 2 (Sb o S'_{n-1}) p ;  k = pb o p
                          bc -= (t_n - t_{n-1}) k ;  bt_n -= c.k ;  bt_{n-1} += c.k ;  Sb <- (p p^T) o Sb
      Queries behind the last row get bVs = 0, queries in front of the data bUs = 0.
(iii) `emulate_forward` / `emulate_reverse`: the device kernels' event loops statement by statement -- the merge with its tie
      rule, the ring with requests ahead, the carried bt, the two workspace columns -- so that their bookkeeping is checked
      where no device is.  Pinned to (i) and (ii) by tests/test_explained_variance_rev.py.
(iv)  `dense_variance`: k0 - diag(K*^T (K + D)^-1 K*) in float64 torch with the masks and signed lags of general_rev_ref.
"""
import numpy as np

RD, PD = 8, 4          # kRing, kPend of csrc/c2_merge_ring.hpp
SPARE = 2 * RD


def last_rows(t, ts):
    return np.searchsorted(np.real(t), np.real(ts), side="right") - 1


def forward_ws(t, ts, c, U, W, d, Us, Vs):
    """(r (M,), X (M, J), Sws (N, J, J), Rws (N, J, J)) of one series."""
    N, J = U.shape
    M = len(ts)
    dt = np.result_type(t, ts, c, U, W, d, Us, Vs)
    nq = last_rows(t, ts)
    r = np.zeros(M, dtype=dt)
    X = np.array(Vs, dtype=dt)
    Sws, Rws = np.zeros((N, J, J), dtype=dt), np.zeros((N, J, J), dtype=dt)
    S = np.zeros((J, J), dtype=dt)
    for n in range(N):
        if n > 0:
            p = np.exp(-c * (t[n] - t[n - 1]))
            S = np.outer(p, p) * S
        S = S + d[n] * np.outer(W[n], W[n])
        Sws[n] = S
        for m in np.nonzero(nq == n)[0]:
            e = np.exp(-c * (ts[m] - t[n]))
            uL = Us[m] * e
            h = S @ uL
            r[m] = uL @ h
            X[m] = Vs[m] - e * h
    R = np.zeros((J, J), dtype=dt)
    for n in range(N - 1, -1, -1):
        if n < N - 1:
            p = np.exp(-c * (t[n + 1] - t[n]))
            G = np.outer(p, p) * R
        else:
            G = R
        g = G @ W[n]
        q = 1.0 / d[n] + W[n] @ g
        R = G - np.outer(U[n], g) - np.outer(g, U[n]) + q * np.outer(U[n], U[n])
        Rws[n] = R
        for m in np.nonzero(nq == n - 1)[0]:
            x = np.exp(-c * (t[n] - ts[m])) * X[m]
            r[m] += x @ R @ x
    return r, X, Sws, Rws


def reverse_rows(t, ts, c, U, W, d, Us, Vs, X, Sws, Rws, br):
    """(bt (N,), bts (M,), bc (J,), bU, bW (N, J), bd (N,), bUs, bVs (M, J)) of one series, per-row loops."""
    N, J = U.shape
    M = len(ts)
    dt = np.result_type(t, c, U, br)
    nq = last_rows(t, ts)
    bt, bts, bc = np.zeros(N, dtype=dt), np.zeros(M, dtype=dt), np.zeros(J, dtype=dt)
    bU, bW, bd = np.zeros((N, J), dtype=dt), np.zeros((N, J), dtype=dt), np.zeros(N, dtype=dt)
    bUs, bVs = np.zeros((M, J), dtype=dt), np.zeros((M, J), dtype=dt)
    Rb = np.zeros((J, J), dtype=dt)
    for n in range(N):
        for m in np.nonzero(nq == n - 1)[0]:
            lag = t[n] - ts[m]
            eps = np.exp(-c * lag)
            x = eps * X[m]
            Rb = Rb + br[m] * np.outer(x, x)
            bx = 2.0 * br[m] * (Rws[n] @ x)
            bVs[m] = eps * bx
            k = x * bx
            bc -= lag * k
            bt[n] -= c @ k
            bts[m] += c @ k
        u, w = U[n], W[n]
        if n < N - 1:
            p = np.exp(-c * (t[n + 1] - t[n]))
            G = np.outer(p, p) * Rws[n + 1]
        else:
            p = np.ones(J, dtype=dt)
            G = np.zeros((J, J), dtype=dt)
        g = G @ w
        q = 1.0 / d[n] + w @ g
        Mu = Rb @ u
        qb = u @ Mu
        gb = -2.0 * Mu + qb * w
        bU[n] = -2.0 * (Rb @ g) + 2.0 * q * Mu
        bd[n] = -qb / d[n] ** 2
        bW[n] = qb * g + G @ gb
        Gb = Rb + 0.5 * (np.outer(gb, w) + np.outer(w, gb))
        if n < N - 1:
            pb = 2.0 * ((Gb * Rws[n + 1]) @ p)
            k = pb * p
            bc -= (t[n + 1] - t[n]) * k
            bt[n + 1] -= c @ k
            bt[n] += c @ k
        Rb = np.outer(p, p) * Gb
    Sb = np.zeros((J, J), dtype=dt)
    for n in range(N - 1, -1, -1):
        for m in np.nonzero(nq == n)[0][::-1]:
            lag = ts[m] - t[n]
            e = np.exp(-c * lag)
            uL = Us[m] * e
            h = Sws[n] @ uL
            bX = bVs[m]
            bh = br[m] * uL - e * bX
            be = -h * bX
            buL = br[m] * h + Sws[n] @ bh
            Sb = Sb + 0.5 * (np.outer(bh, uL) + np.outer(uL, bh))
            bUs[m] = e * buL
            be = be + Us[m] * buL
            k = e * be
            bc -= lag * k
            bts[m] -= c @ k
            bt[n] += c @ k
        w = W[n]
        Sw = Sb @ w
        bd[n] += w @ Sw
        bW[n] += 2.0 * d[n] * Sw
        if n > 0:
            lag = t[n] - t[n - 1]
            p = np.exp(-c * lag)
            pb = 2.0 * ((Sb * Sws[n - 1]) @ p)
            k = pb * p
            bc -= lag * k
            bt[n] -= c @ k
            bt[n - 1] += c @ k
            Sb = np.outer(p, p) * Sb
    return bt, bts, bc, bU, bW, bd, bUs, bVs


# ------------------------------------------------------------------------------------------------------------------
# the kernels' event loops

def _ring_walk(N, M, up, tb, tsb, dD, dA, dB, qD, qA, qB, J, event):
    """The merged walk of k_predvar / k_predvar_rev for one series: the ring (NaN where nothing has arrived), requests RD
    positions ahead that arrive PD events later, the tie rule.  Calls event(kind, n, m, slots) with kind in "d", "q", None
    (positions n, m of the next data row and query), and slots = the ring arrays (T, D, A, B)."""
    rowN = (lambda s: s) if up else (lambda s: N - 1 - s)
    rowM = (lambda s: s) if up else (lambda s: M - 1 - s)
    NS = 2 * RD + 1
    rgT, rgD = np.full(NS, np.nan), np.full(NS, np.nan)
    rgA, rgB = np.full((NS, J), np.nan), np.full((NS, J), np.nan)
    rgT[SPARE] = 0.0; rgD[SPARE] = 1.0; rgA[SPARE] = 0.0; rgB[SPARE] = 0.0
    for q in range(RD):
        rn, rm = rowN(q if q < N else N - 1), rowM(q if q < M else M - 1)
        rgT[q] = tb[rn]; rgD[q] = dD[rn]; rgA[q] = dA[rn]; rgB[q] = dB[rn]
        rgT[RD + q] = tsb[rm]; rgD[RD + q] = qD[rm]; rgA[RD + q] = qA[rm]; rgB[RD + q] = qB[rm]
    pend = [dict(t=0.0, d=1.0, a=np.zeros(J), b=np.zeros(J), slot=SPARE) for _ in range(PD)]
    n = m = 0
    total = N + M
    it = 0
    while it < total:
        for k in range(PD):
            pk = pend[k]
            rgT[pk["slot"]] = pk["t"]; rgD[pk["slot"]] = pk["d"]; rgA[pk["slot"]] = pk["a"]; rgB[pk["slot"]] = pk["b"]
            tn, tq = rgT[n & (RD - 1)], rgT[RD + (m & (RD - 1))]
            hasn, hasm = n < N, m < M
            isd = hasn and ((not hasm) or ((tn <= tq) if up else (tn > tq)))
            isq = (not isd) and hasm
            pos = n if isd else m
            len1 = (N if isd else M) - 1
            so = ((pos & (RD - 1)) + (0 if isd else RD)) if (isd or isq) else SPARE
            sreq = pos + RD if pos + RD < len1 else len1
            rreq = (len1 - sreq) if not up else sreq
            assert 0 <= rreq <= len1
            if isd:
                pend[k] = dict(t=tb[rreq], d=dD[rreq], a=dA[rreq].copy(), b=dB[rreq].copy(), slot=so)
            else:
                pend[k] = dict(t=tsb[rreq], d=qD[rreq], a=qA[rreq].copy(), b=qB[rreq].copy(), slot=so)
            event("d" if isd else ("q" if isq else None), n, m, so, (rgT, rgD, rgA, rgB))
            n += 1 if isd else 0
            m += 1 if isq else 0
        it += PD
    assert n == N and m == M, (n, N, m, M)


def emulate_forward(t, ts, c, U, W, d, Us, Vs):
    """The two launches of k_predvar<G, BACK, WS = true> for one series: (r, X, Sws, Rws)."""
    N, J = U.shape
    M = len(ts)
    r, X = np.full(M, np.nan), np.full((M, J), np.nan)
    Sws, Rws = np.full((N, J, J), np.nan), np.full((N, J, J), np.nan)
    for back in (False, True):
        St = np.zeros((J, J))
        st = dict(tref=0.0)
        rowN = (lambda s: N - 1 - s) if back else (lambda s: s)
        rowM = (lambda s: M - 1 - s) if back else (lambda s: s)

        def event(kind, n, m, so, ring, back=back, st=st, rowN=rowN, rowM=rowM):
            nonlocal St
            rgT, rgD, rgA, rgB = ring
            isd, isq = kind == "d", kind == "q"
            tev = rgT[so] if kind else 0.0
            ea, eb, dslot = rgA[so].copy(), rgB[so].copy(), rgD[so]
            dn = dslot if (isd or not back) else 1.0
            dtt = ((tev - st["tref"]) if back else (st["tref"] - tev)) if n > 0 else 0.0
            e = np.exp(c * dtt)
            if not back:
                v = ea if isd else ea * e
                pj = e if isd else np.ones(J)
                dw = dn * ea if isd else np.zeros(J)
                h = St @ v
                St = np.outer(pj, pj) * St + np.outer(dw, v)
                s = v @ h
                if isq:
                    X[rowM(m)] = eb - e * h
                    r[rowM(m)] = s
                if isd:
                    Sws[rowN(n)] = St
            else:
                v = e * ea
                pj = e if isd else np.ones(J)
                un = eb if isd else np.zeros(J)
                h = St @ v
                s = v @ h
                qn = 1.0 / dn + s
                ee = (qn * un - pj * h) if isd else np.zeros(J)
                xx = np.outer(pj, np.ones(J)) * St - np.outer(un, h)       # x[j, i] = pj_j St[j, i] - h_i un_j
                St = np.outer(ee, un) + xx * pj[None, :]
                if isq:
                    r[rowM(m)] = dslot + s
                if isd:
                    Rws[rowN(n)] = St
            if isd:
                st["tref"] = tev

        if not back:
            _ring_walk(N, M, True, t, ts, d, W, W, np.ones(M), Us, Vs, J, event)
        else:
            _ring_walk(N, M, False, t, ts, d, W, U, r, X, X, J, event)
    return r, X, Sws, Rws


def emulate_reverse(t, ts, c, U, W, d, Us, Vs, X, Sws, Rws, br):
    """The two launches of k_predvar_rev for one series, the lanes j = 0 .. J-1 as numpy vectors: pass A (BACK = true, walks
    up, reads Rws) then pass B (BACK = false, walks down, reads Sws and adds to what pass A wrote)."""
    N, J = U.shape
    M = len(ts)
    bt, bts, bc = np.full(N, np.nan), np.full(M, np.nan), np.full(J, np.nan)
    bU, bW, bd = np.full((N, J), np.nan), np.full((N, J), np.nan), np.full(N, np.nan)
    bUs, bVs = np.full((M, J), np.nan), np.full((M, J), np.nan)
    for back in (True, False):
        up = back
        ws = Rws if back else Sws
        rowN = (lambda s: s) if up else (lambda s: N - 1 - s)
        rowM = (lambda s: s) if up else (lambda s: M - 1 - s)
        col = lambda pos: ws[rowN(min(pos, N - 1))]      # lane j holds column j; the records are symmetric
        st = dict(St=np.zeros((J, J)), bcj=np.zeros(J), carry=0.0, cur=col(0), nxt=col(1))

        def event(kind, n, m, so, ring, back=back, up=up, st=st, rowN=rowN, rowM=rowM, col=col):
            rgT, rgD, rgA, rgB = ring
            isd, isq = kind == "d", kind == "q"
            hasn = n < N
            tn, tq, tn1 = rgT[n & (RD - 1)], rgT[RD + (m & (RD - 1))], rgT[(n + 1) & (RD - 1)]
            ea, eb, ds = rgA[so].copy(), rgB[so].copy(), rgD[so]
            lastd = n + 1 >= N
            live = isq and hasn
            if isd:
                lag = 0.0 if lastd else ((tn1 - tn) if up else (tn - tn1))
            else:
                lag = ((tn - tq) if up else (tq - tn)) if live else 0.0
            assert lag >= 0.0
            e = np.exp(-(c * lag))
            St, cur, nxt = st["St"], st["cur"], st["nxt"]
            zero = np.zeros(J)
            if isd:
                row = rowN(n)
                step = not lastd
                if back:
                    u, w, p = eb, ea, e
                    pw = p * w if step else zero
                    hM, Mu = nxt @ pw, St @ u
                    g = p * hM
                    q = 1.0 / ds + w @ g
                    qb = u @ Mu
                    gb = qb * w - 2.0 * Mu
                    pg = p * gb if step else zero
                    Mg, hG = St @ g, nxt @ pg
                    bU[row] = 2.0 * q * Mu - 2.0 * Mg
                    bW[row] = qb * g + p * hG
                    bd[row] = -qb * (1.0 / ds) ** 2
                    Gb = St + 0.5 * (np.outer(gb, w) + np.outer(w, gb))
                    ps = (Gb * nxt) @ p
                    St = np.outer(p, p) * Gb
                    k = 2.0 * ps * p if step else zero
                    st["bcj"] = -lag * k + st["bcj"]
                    x = c @ k
                    bt[row] = st["carry"] + x
                    st["carry"] = -x
                else:
                    w = ea
                    p = e if step else np.ones(J)
                    Sw = St @ w
                    ps = (St * nxt) @ p
                    k = 2.0 * ps * p if step else zero
                    st["bcj"] = -lag * k + st["bcj"]
                    x = c @ k
                    bW[row] += 2.0 * ds * Sw
                    bd[row] += w @ Sw
                    bt[row] += st["carry"] - x
                    st["carry"] = x
                    St = np.outer(p, p) * St
                cur, nxt = nxt, col(n + 2)
            elif isq:
                row = rowM(m)
                brq = ds if live else 0.0
                if back:
                    x = e * ea
                    h = cur @ x
                    bx = 2.0 * brq * h
                    k = x * bx
                    st["bcj"] = -lag * k + st["bcj"]
                    ck = c @ k
                    bVs[row] = e * bx if live else zero
                    bts[row] = ck if live else 0.0
                    if live:
                        st["carry"] = st["carry"] - ck
                    St = St + brq * np.outer(x, x)
                else:
                    us = ea
                    bX = eb if live else zero
                    uL = us * e
                    h = cur @ uL
                    bh = brq * uL - e * bX
                    be = -h * bX
                    buL = brq * h + cur @ bh
                    be = us * buL + be
                    k = e * be
                    st["bcj"] = -lag * k + st["bcj"]
                    ck = c @ k
                    bUs[row] = e * buL if live else zero
                    if live:
                        bts[row] -= ck
                        st["carry"] = st["carry"] + ck
                    St = St + 0.5 * (np.outer(bh, uL) + np.outer(uL, bh))
            st["St"], st["cur"], st["nxt"] = St, cur, nxt

        if back:
            _ring_walk(N, M, True, t, ts, d, W, U, br, X, X, J, event)
            bc[:] = st["bcj"]
        else:
            _ring_walk(N, M, False, t, ts, d, W, W, br, Us, bVs, J, event)
            bc += st["bcj"]
    return bt, bts, bc, bU, bW, bd, bUs, bVs


# ------------------------------------------------------------------------------------------------------------------
# the dense closed form under torch autograd

def dense_variance(t, ts, c, a, U, V, Us, Vs, k0):
    """k0 - diag(K*^T (K + D)^-1 K*) (..., M) in float64 torch, differentiable; leading batch axes allowed, t / ts / c
    shared or not.  Masks and SIGNED lags as general_rev_ref.dense_operator: abs has derivative 0 at a tie."""
    import torch
    from general_rev_ref import dense_operator
    N = t.shape[-1]
    L = dense_operator(t, t, c, U, V, True)                                  # t_n - t_m >= 0
    strict = torch.tril(torch.ones(N, N, dtype=torch.bool), -1)
    L = torch.where(strict, L, torch.zeros_like(L))
    K = L + L.transpose(-1, -2) + torch.diag_embed(a)
    Ks = dense_operator(ts, t, c, Us, V, True) + dense_operator(ts, t, c, Vs, U, False)   # (..., M, N)
    sol = torch.linalg.solve(K, Ks.transpose(-1, -2))                        # (..., N, M)
    return k0 - (Ks.transpose(-1, -2) * sol).sum(-2)


def query_grid(kind, t, rng, M):
    """Sorted query times: predict_at_ref.queries ("mixed"), every query in front of the data, every query behind it,
    or ties with data rows and repeated queries."""
    from predict_at_ref import queries
    if kind == "mixed":
        return queries(t, rng, M)
    if kind == "front":
        return np.sort(t[0] - rng.uniform(0.01, 2.0, M))
    if kind == "behind":
        return np.sort(t[-1] + rng.uniform(0.0, 2.0, M))      # (may tie with the last row: still n(m) = N - 1)
    assert kind == "ties"
    ts = rng.uniform(t[0] - 0.3, t[-1] + 0.3, M)
    k = min(len(t), M)
    ts[:k:2] = t[:k:2]
    if M >= 3:
        ts[M - 1] = ts[M - 2]
    return np.sort(ts)


GRID_KINDS = ("mixed", "front", "behind", "ties")
