# -*- coding: utf-8 -*-
"""numpy restatement of the reverse of a streaming forecast and of a streaming absorb (celerite2_amd/csrc/c2_filter_stream_rev.hip,
include/celerite2_amd_filter_stream_rev.h) on the public state layout, for one series, and torch float64 restatements of
filter_ref.forecast and filter_ref.absorb for autograd to differentiate.  Test infrastructure only -- nothing here is imported
by the package.  The restatements compose with filter_rev_ref.append_rev: a state cotangent has the layout of the state, its S
block the symmetric representative.

Forecast, per query row, each from the same state (p := 0 when n == 0), Dt = t_m - t_last, x = p o u, h = S x:

    ba = bvar        xb = bmu F - 2 bvar h        bU = p o xb        pi = x o xb
    bc -= Dt pi      Dtb = -sum_j c_j pi_j        bt = Dtb           bstate[0] -= Dtb
    bF += bmu x      bS -= bvar x x^T

Absorb, per row backwards, St = (p p^T) o S0, Ft = p o F0 the decayed entry state of the row, lb, qb words [2], [3]:

    bd = lb / d - qb z^2 / d^2 + w^T Sb w        bz = 2 qb z / d + Fb . w        bW = z Fb + 2 d Sb w
    pi = 2 (Sb o St) 1 + Fb o Ft                 Sb <- (p p^T) o Sb              Fb <- p o Fb
    bc -= Dt pi      Dtb = -sum_j c_j pi_j       bt_m += Dtb                     bt_{m-1} -= Dtb"""
import numpy as np

import filter_ref as F
import filter_rev_ref as R

HEAD = F.HEAD


def forecast_rev(state, c, t, U, bmu, bvar, count=None):
    """-> (bstate (SW,), bt (M,), bc (J,), ba (M,), bU (M, J)) of one series."""
    M, J = U.shape
    count = M if count is None else min(max(int(count), 0), M)
    tl, n, _, _, Fv, S = F.unpack(state, J)
    bt, ba, bU, bc = np.zeros(M), np.zeros(M), np.zeros((M, J)), np.zeros(J)
    bF, bS, btl = np.zeros(J), np.zeros((J, J)), 0.0
    for m in range(count):
        empty = n == 0
        p = np.zeros(J) if empty else np.exp(-c * (t[m] - tl))
        x = p * U[m]
        h = S @ x
        ba[m] = bvar[m]
        xb = bmu[m] * Fv - 2.0 * bvar[m] * h
        bU[m] = p * xb
        pi = x * xb
        if not empty:   # (a stale t_last of an empty state is never multiplied)
            bc -= (t[m] - tl) * pi
            bt[m] = -np.sum(c * pi)
            btl -= bt[m]
        bF += bmu[m] * x
        bS -= bvar[m] * np.outer(x, x)
    return np.concatenate([[btl, 0.0, 0.0, 0.0], bF, bS.ravel()]), bt, bc, ba, bU


def absorb_rev(state, c, t, W, d, z, bstate, count=None):
    """-> (bstate_in (SW,), bt (M,), bc (J,), bW (M, J), bd (M,), bz (M,), ws (M, J + J^2)) of one series."""
    M, J = W.shape
    count = M if count is None else min(max(int(count), 0), M)
    bt, bW, bd, bz, bc = np.zeros(M), np.zeros((M, J)), np.zeros(M), np.zeros(M), np.zeros(J)
    if count == 0:   # the forward call passed this series through
        return bstate.copy(), bt, bc, bW, bd, bz, np.full((M, R.workspace_words(J)), np.nan)
    ws = R.replay(state, c, t, W, d, z, count)
    lb, qb = bstate[2], bstate[3]
    Fb = bstate[HEAD:HEAD + J].copy()
    Sb = bstate[HEAD + J:].reshape(J, J)
    Sb = 0.5 * (Sb + Sb.T)
    carry = bstate[0]
    for m in range(count - 1, -1, -1):
        F0, S0 = ws[m, :J], ws[m, J:].reshape(J, J)
        emp = m == 0 and state[1] == 0
        tp = state[0] if m == 0 else t[m - 1]
        p = np.zeros(J) if emp else np.exp(-c * (t[m] - tp))
        St, Ft = np.outer(p, p) * S0, p * F0
        w = W[m]
        Sw = Sb @ w
        bd[m] = lb / d[m] - qb * z[m] ** 2 / d[m] ** 2 + w @ Sw
        bz[m] = 2 * qb * z[m] / d[m] + Fb @ w
        bW[m] = z[m] * Fb + 2 * d[m] * Sw
        pi = 2 * (Sb * St).sum(axis=1) + Fb * Ft
        Sb = np.outer(p, p) * Sb
        Fb = p * Fb
        if emp:
            Db = 0.0
        else:
            bc -= (t[m] - tp) * pi
            Db = -np.sum(c * pi)
        bt[m] = carry + Db
        carry = -Db
    bstate_in = np.concatenate([[carry + 0.0, bstate[1], lb, qb], Fb, Sb.ravel()])
    return bstate_in, bt, bc, bW, bd, bz, ws


def torch_forecast(state, c, t, a, U):
    """filter_ref.forecast in torch float64: -> (mu (M,), var (M,)), for autograd.  n == 0: p = 0 whatever t_last holds."""
    import torch

    M, J = U.shape
    tl = state[0]
    Fv, S = state[HEAD:HEAD + J], state[HEAD + J:].reshape(J, J)
    empty = float(state[1].detach()) == 0.0
    mu, var = [], []
    for m in range(M):
        p = torch.zeros_like(c) if empty else torch.exp(-c * (t[m] - tl))
        x = p * U[m]
        mu.append(x @ Fv)
        var.append(a[m] - x @ (S @ x))
    return torch.stack(mu), torch.stack(var)


def torch_absorb(state, c, t, W, d, z):
    """filter_ref.absorb in torch float64: -> state_out (SW,), for autograd."""
    import torch

    M, J = W.shape
    tl, n, ld, q = state[0], state[1], state[2], state[3]
    Fv, S = state[HEAD:HEAD + J], state[HEAD + J:].reshape(J, J)
    empty = float(n.detach()) == 0.0
    for m in range(M):
        p = torch.zeros_like(c) if empty else torch.exp(-c * (t[m] - tl))
        S = torch.outer(p, p) * S + d[m] * torch.outer(W[m], W[m])
        Fv = p * Fv + W[m] * z[m]
        tl, n, ld, q = t[m], n + 1.0, ld + torch.log(d[m]), q + z[m] * z[m] / d[m]
        empty = False
    return torch.cat([torch.stack([tl, n, ld, q]), Fv, S.reshape(-1)])
