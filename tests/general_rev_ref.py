# -*- coding: utf-8 -*-
"""Two references for general_matmul_lower / general_matmul_upper and their reverse pass
(celerite2_amd/csrc/c2_general_rev.hip).  Test infrastructure only -- nothing here is imported by the package.

(i)  `forward` / `reverse`: the recurrence in numpy, ONE series, both variants, in walk coordinates: position s = 0 .. M-1
     along t2 and q = 0 .. N-1 along t1; walk time tau = t and array row = position (lower), tau = -t and array row =
     M-1-s / N-1-q (upper).  Row s feeds output q iff tau2[s] <= tau1[q] (lower) / tau2[s] < tau1[q] (upper).
         F_0 = V_0^T Y_0 ;  F_s = p_s o F_{s-1} + V_s^T Y_s ,  p_s = exp(-c (tau2[s] - tau2[s-1]))
         Z_q += (U_q o e_q) F_{s(q)} ,  e_q = exp(-c (tau1[q] - tau2[s(q)]))
     `forward` writes the workspace with the reference's quirks (forward.hpp:285-392): rows never absorbed, and the upper
     variant's start row, are left as they were -- here NaN, so that a reverse pass that reads them shows.
     `reverse` walks the events backwards with G (J x nrhs); bc is summed event by event from non-negative lags.
(ii) `dense`: the dense operator in float64 torch, differentiated by torch autograd on the CPU.  The mask is
     t1_n - t2_m >= 0 (lower) / < 0 (upper) and the lag is taken SIGNED under the mask, not through abs: abs has derivative 0
     at a tie, where the correct one-sided derivative in t1 / t2 is not 0.
Beside them `emulate_kernel` restates the device kernel's event loop (ring, requests ahead, accumulating launches), so that
its bookkeeping is checked where no device is."""
import numpy as np
import torch


def _walk(t1, t2, lower):
    """tau1, tau2 in walk order and the array rows of the positions."""
    N, M = len(t1), len(t2)
    if lower:
        return t1.copy(), t2.copy(), np.arange(N), np.arange(M)
    return -t1[::-1], -t2[::-1], np.arange(N)[::-1], np.arange(M)[::-1]


def _feeds(tau2s, tau1q, lower):
    return tau2s <= tau1q if lower else tau2s < tau1q


def forward(t1, t2, c, U, V, Y, lower, fill=np.nan):
    """(Z (N, nrhs), F (M, J, nrhs)) of one series; F rows the reference does not write hold `fill`."""
    N, M, J, K = len(t1), len(t2), len(c), Y.shape[1]
    tau1, tau2, rn, rm = _walk(t1, t2, lower)
    Z = np.zeros((N, K))
    F = np.full((M, J, K), fill)
    Fs = np.outer(V[rm[0]], Y[rm[0]])
    if lower:
        F[0] = Fs
    s = 0
    for q in range(N):
        if not _feeds(tau2[0], tau1[q], lower):
            continue
        while s + 1 < M and _feeds(tau2[s + 1], tau1[q], lower):
            s += 1
            Fs = np.exp(-c * (tau2[s] - tau2[s - 1]))[:, None] * Fs + np.outer(V[rm[s]], Y[rm[s]])
            F[rm[s]] = Fs
        e = np.exp(-c * (tau1[q] - tau2[s]))
        Z[rn[q]] = (U[rn[q]] * e) @ Fs
    return Z, F


def reverse(t1, t2, c, U, V, Y, F, bZ, lower):
    """(bt1 (N,), bt2 (M,), bc (J,), bU (N, J), bV (M, J), bY (M, nrhs)) of one series from the workspace F."""
    N, M, J, K = len(t1), len(t2), len(c), Y.shape[1]
    tau1, tau2, rn, rm = _walk(t1, t2, lower)
    bt1, bt2, bc = np.zeros(N), np.zeros(M), np.zeros(J)
    bU, bV, bY = np.zeros((N, J)), np.zeros((M, J)), np.zeros((M, K))
    S = int(np.sum(_feeds(tau2, tau1[N - 1], lower)))   # rows the forward absorbed: positions 0 .. S-1
    G = np.zeros((J, K))
    q = N - 1
    sg = 1.0 if lower else -1.0
    for s in range(S - 1, -1, -1):
        Fs = np.outer(V[rm[0]], Y[rm[0]]) if s == 0 else F[rm[s]]   # (the start row: never read from the workspace)
        while q >= 0 and _feeds(tau2[s], tau1[q], lower):
            lag = tau1[q] - tau2[s]
            e = np.exp(-c * lag)
            u = U[rn[q]]
            bu = e * (Fs @ bZ[rn[q]])
            bU[rn[q]] = bu
            bc -= lag * u * bu
            G += np.outer(u * e, bZ[rn[q]])
            bt1[rn[q]] = -sg * np.sum(c * u * bu)
            q -= 1
        v, y = V[rm[s]], Y[rm[s]]
        bv = G @ y
        bV[rm[s]] = bv
        bY[rm[s]] = v @ G
        bt2[rm[s]] = sg * np.sum(c * v * bv)
        if s >= 1:
            lag = tau2[s] - tau2[s - 1]
            bc -= lag * np.sum(G * (Fs - np.outer(v, y)), axis=1)
            G = np.exp(-c * lag)[:, None] * G
    return bt1, bt2, bc, bU, bV, bY


def dense_operator(t1, t2, c, U, V, lower):
    """K (..., N, M) in torch: sum_j U_nj V_mj exp(-c_j lag_nm) under the mask, lag signed under the mask."""
    diff = t1[..., :, None] - t2[..., None, :]
    mask = diff >= 0 if lower else diff < 0
    lag = torch.where(mask, diff if lower else -diff, torch.zeros_like(diff))
    E = torch.exp(-c[..., None, None, :] * lag[..., None])                     # (..., N, M, J)
    K = (U[..., :, None, :] * V[..., None, :, :] * E).sum(-1)
    return torch.where(mask, K, torch.zeros_like(K))


def dense(t1, t2, c, U, V, Y, bZ, lower):
    """Z and (bt1, bt2, bc, bU, bV, bY) by torch autograd on the CPU; numpy in (any leading batch axes, t1 / t2 / c shared
    or not), numpy out -- the gradients of shared arguments come out summed over the batch, as autograd gives them."""
    args = [torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True) for x in (t1, t2, c, U, V, Y)]
    Z = dense_operator(*args[:5], lower) @ args[5]
    grads = torch.autograd.grad(Z, args, torch.tensor(np.asarray(bZ), dtype=torch.float64))
    return Z.detach().numpy(), tuple(g.numpy() for g in grads)


RD, PD = 8, 4          # kRing, kPend of csrc/c2_merge_ring.hpp
SPARE = 2 * RD


def emulate_kernel(t1, t2, c, U, V, Y, F, bZ, lower, out, k, acc):
    """One launch of k_general_rev (csrc/c2_general_rev.hip) for ONE series and right-hand side k, statement by statement, the
    lanes j = 0 .. J-1 as numpy vectors: the binary search for S, the zeros of the rows never absorbed, the ring (slots =
    index mod RD of the backward walk; data slots, output slots, a spare) filled with NaN so that a read of a row that has
    not arrived shows, the requests RD indices ahead that arrive PD events later, the predicated event.  `out`: the six
    arrays (bt1, bt2, bc, bU, bV, bY), written (acc false) or added to (acc true) as the launches for k = 0, 1, ... do."""
    N, M, J = len(t1), len(t2), len(c)
    nrhs = Y.shape[1]
    bt1, bt2, bc, bU, bV, bY = out
    tq = t1[N - 1 if lower else 0]
    lo, hi = 0, M
    while lo < hi:
        mid = (lo + hi) >> 1
        tm = t2[mid if lower else M - 1 - mid]
        if (tm <= tq) if lower else (tm > tq):
            lo = mid + 1
        else:
            hi = mid
    S = lo
    arrM = lambda m: S - 1 - m if lower else M - S + m
    arrN = lambda n: N - 1 - n if lower else n
    for p in range(S, M):
        row = p if lower else M - 1 - p
        bY[row, k] = 0.0
        if not acc:
            bt2[row] = 0.0
            bV[row] = 0.0
    NS = 2 * RD + 1
    rgT, rgX = np.full(NS, np.nan), np.full(NS, np.nan)
    rgA, rgB = np.full((NS, J), np.nan), np.full((NS, J), np.nan)
    rgT[SPARE] = 0; rgX[SPARE] = 0; rgA[SPARE] = 0; rgB[SPARE] = 0
    for q in range(RD):
        tm = xm = 0.0; am = np.zeros(J); fm = np.zeros(J)
        if S > 0:
            mm = q if q < S else S - 1
            row = arrM(mm)
            tm = t2[row] if lower else -t2[row]
            xm = Y[row, k]
            am = V[row].copy()
            fm = am * xm if mm == S - 1 else F[row, :, k].copy()
        rn = arrN(q if q < N else N - 1)
        rgT[q] = tm; rgX[q] = xm; rgA[q] = am; rgB[q] = fm
        rgT[RD + q] = t1[rn] if lower else -t1[rn]; rgX[RD + q] = bZ[rn, k]
        rgA[RD + q] = U[rn]; rgB[RD + q] = 0
    pend = [dict(t=0.0, x=0.0, a=np.zeros(J), f=np.zeros(J), slot=SPARE) for _ in range(PD)]
    n = m = 0
    Gs = np.zeros(J); bcj = np.zeros(J)
    total = N + M
    it = 0
    while it < total:
        if not (n < N or m < S):
            break
        for i in range(PD):
            pk = pend[i]
            rgT[pk["slot"]] = pk["t"]; rgX[pk["slot"]] = pk["x"]; rgA[pk["slot"]] = pk["a"]; rgB[pk["slot"]] = pk["f"]
            sd, sq = m & (RD - 1), RD + (n & (RD - 1))
            tm, tq_, tm1 = rgT[sd], rgT[sq], rgT[(m + 1) & (RD - 1)]
            hasm, hasn = m < S, n < N
            isout = hasn and ((not hasm) or ((tm <= tq_) if lower else (tm < tq_)))
            isrow = (not isout) and hasm
            so = sq if isout else (sd if isrow else SPARE)
            pos = m if isrow else n
            len1 = (S if isrow else N) - 1
            sreq = pos + RD if pos + RD < len1 else len1
            rreq = arrM(sreq) if isrow else arrN(sreq)
            assert 0 <= rreq < (M if isrow else N)
            rt = (t2 if isrow else t1)[rreq]
            rx = (Y if isrow else bZ)[rreq, k]
            ra = (V if isrow else U)[rreq].copy()
            rf = F[rreq, :, k].copy() if isrow else np.zeros(J)
            pend[i] = dict(t=rt if lower else -rt, x=rx, a=ra, f=(ra * rx if (isrow and sreq == len1) else rf), slot=so)
            a, x = rgA[so].copy(), rgX[so]
            f = rgB[sd].copy() if hasm else np.zeros(J)
            fed = isout and hasm
            step = isrow and m + 1 < S
            lag = tq_ - tm if fed else (tm - tm1 if step else 0.0)
            assert lag >= 0
            e = np.exp(-(c * lag))
            w = e * (f * x) if isout else Gs * x
            r = a * w if isout else Gs * (f - a * x)
            bcj = -lag * r + bcj
            red1 = np.sum(c * (a * w)); red2 = np.sum(a * Gs)
            Gs = (a * e) * x + Gs if isout else (e * Gs if isrow else Gs)
            if isout or isrow:
                row = arrN(n) if isout else arrM(m)
                pj = bU if isout else bV
                ps = bt1 if isout else bt2
                bt = 0.0 - red1 if (isout == lower) else red1
                if acc:
                    pj[row] += w; ps[row] += bt
                else:
                    pj[row] = w; ps[row] = bt
                if isrow:
                    bY[row, k] = red2
            n += 1 if isout else 0
            m += 1 if isrow else 0
        it += PD
    assert n == N and m == S, (n, N, m, S)
    if acc:
        bc += bcj
    else:
        bc[:] = bcj


# ------------------------------------------------------------------------------------------------------------------
# inputs

GRID_KINDS = ("interleaved", "t1_before", "t1_behind", "ties", "offset")


def grids(kind, N, M, rng):
    """Sorted (t1 (N,), t2 (M,)) of one of the kinds the tests walk through."""
    t1 = np.sort(rng.uniform(0.0, 10.0, N))
    t2 = np.sort(rng.uniform(0.0, 10.0, M))
    if kind == "t1_before":       # every output in front of the first row
        t1 = t1 - 11.0
    elif kind == "t1_behind":     # every output behind the last row
        t1 = t1 + 11.0
    elif kind == "ties":          # exact ties between the grids, a repeated t2 value, a repeated t1 value
        k = min(N, M)
        t1[:k:2] = t2[:k:2]
        if M >= 3:
            t2[M // 2] = t2[M // 2 - 1]
        if N >= 4:
            t1[N - 1] = t1[N - 2]
        t1, t2 = np.sort(t1), np.sort(t2)
    elif kind == "offset":
        t1, t2 = t1 + 2450000.0, t2 + 2450000.0
    return t1, t2


def inputs(kind, B, N, M, J, K, seed, lower):
    """A batch whose neighbouring series differ: (t1 (B,N), t2 (B,M), c (B,J), U (B,N,J), V (B,M,J), Y (B,M,K), bZ (B,N,K)).
    For the upper variant "before" and "behind" swap sides, so that the kind names what the WALK sees."""
    rng = np.random.default_rng(seed)
    t1, t2 = np.empty((B, N)), np.empty((B, M))
    for b in range(B):
        k = kind
        if not lower and kind in ("t1_before", "t1_behind"):
            k = "t1_behind" if kind == "t1_before" else "t1_before"
        t1[b], t2[b] = grids(k, N, M, rng)
    c = rng.uniform(0.05, 1.5, (B, J))
    U, V = rng.normal(size=(B, N, J)), rng.normal(size=(B, M, J))
    Y, bZ = rng.normal(size=(B, M, K)), rng.normal(size=(B, N, K))
    return t1, t2, c, U, V, Y, bZ


def close(got, want, name="", rtol=1e-10, floor=1e-12):
    """The project's criterion (tests/test_gpu_exact_gradients.py): 1e-10 relative per element plus a floor of 1e-12 of the
    array's largest entry.  Returns the worst ratio error / bound (<= 1 passes) and asserts it."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if want.size == 0:
        return 0.0
    bound = rtol * np.abs(want) + floor * max(float(np.max(np.abs(want))), np.finfo(np.float64).tiny)
    ratio = float(np.max(np.abs(got - want) / bound))
    assert np.all(np.isfinite(got)) and ratio <= 1.0, "%s: %.3g of the criterion" % (name, ratio)
    return ratio
