# -*- coding: utf-8 -*-
"""numpy restatement of the reverse of a streaming append (celerite2_amd/csrc/c2_filter_rev.hip,
include/celerite2_amd_filter_rev.h) on the public state layout, for one series, and a torch float64 restatement of the append
itself for autograd to differentiate.  Test infrastructure only -- nothing here is imported by the package.

A state cotangent has the layout of the state: [b t_last, b n, b sum log d, b sum z^2 / d, b F (J), b S (J x J)], its S block
the symmetric representative.  Per row, backwards, with S0, F0 the state the row starts from, p its decay (0 for the first row
of an empty series), St = (p p^T) o S0, Ft = p o F0, g = St u, and lb, qb words [2], [3] of the cotangent:

    db = bd + lb / d - qb z^2 / d^2 + w^T Sb w        zb = bz + 2 qb z / d + Fb . w
    wb = bW + z Fb + 2 d Sb w
    by = zb        ub = -zb Ft        Ftb = Fb - zb u
    bV = wb / d    gb = -wb / d       db -= (wb . w) / d
    ba = db        ub -= db g         gb -= db u
    Stb = Sb + (gb u^T + u gb^T) / 2                  bU = ub + St gb
    pb = 2 (Stb o S0) p + Ftb o F0
    Sb <- (p p^T) o Stb      Fb <- p o Ftb
    bc -= Dt (p o pb)        Dtb = -sum_j c_j p_j pb_j        bt_m += Dtb     bt_{m-1} -= Dtb"""
import numpy as np

import filter_ref as F

HEAD = F.HEAD


def workspace_words(J):
    return J + J * J


def replay(state, c, t, W, d, z, count=None):
    """ws (M, J + J^2): the (F, S) every taken row starts from, unpropagated (rows beyond count: NaN)."""
    M, J = W.shape
    count = M if count is None else count
    ws = np.full((M, workspace_words(J)), np.nan)
    st = state.copy()
    for m in range(count):
        ws[m] = st[HEAD:]
        st = F.absorb(st, c, t[m:m + 1], W[m:m + 1], d[m:m + 1], z[m:m + 1])
    return ws


def append_rev(state, c, t, U, W, d, z, flag, bstate, bd=None, bW=None, bz=None, count=None):
    """-> (bstate_in (SW,), bt (M,), bc (J,), ba (M,), bU (M, J), bV (M, J), by (M,), ws (M, J + J^2)) of one series."""
    M, J = U.shape
    count = M if count is None else min(max(int(count), 0), M)
    bd = np.zeros(M) if bd is None else bd
    bW = np.zeros((M, J)) if bW is None else bW
    bz = np.zeros(M) if bz is None else bz
    bt, ba, bU, bV, by = np.zeros(M), np.zeros(M), np.zeros((M, J)), np.zeros((M, J)), np.zeros(M)
    bc = np.zeros(J)
    if count == 0 or flag != 0:   # the forward call passed this series through
        return bstate.copy(), bt, bc, ba, bU, bV, by, np.full((M, workspace_words(J)), np.nan)
    ws = replay(state, c, t, W, d, z, count)
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
        u, w = U[m], W[m]
        g = St @ u
        Sw = Sb @ w
        db = bd[m] + lb / d[m] - qb * z[m] ** 2 / d[m] ** 2 + w @ Sw
        zb = bz[m] + 2 * qb * z[m] / d[m] + Fb @ w
        wb = bW[m] + z[m] * Fb + 2 * d[m] * Sw
        by[m] = zb
        ub = -zb * Ft
        Ftb = Fb - zb * u
        bV[m] = wb / d[m]
        gb = -wb / d[m]
        db -= (wb @ w) / d[m]
        ba[m] = db
        ub -= db * g
        gb -= db * u
        Stb = Sb + 0.5 * (np.outer(gb, u) + np.outer(u, gb))
        bU[m] = ub + St @ gb
        pb = 2 * (Stb * S0) @ p + Ftb * F0
        Sb = np.outer(p, p) * Stb
        Fb = p * Ftb
        if emp:
            Db = 0.0
        else:
            bc -= (t[m] - tp) * (p * pb)
            Db = -np.sum(c * p * pb)
        bt[m] = carry + Db
        carry = -Db
    bstate_in = np.concatenate([[carry + 0.0, bstate[1], lb, qb], Fb, Sb.ravel()])
    return bstate_in, bt, bc, ba, bU, bV, by, ws


def symmetrise(bstate, J):
    """A state cotangent with its S block replaced by the symmetric representative."""
    out = np.array(bstate, dtype=float)
    S = out[HEAD + J:].reshape(J, J)
    out[HEAD + J:] = (0.5 * (S + S.T)).ravel()
    return out


def torch_append(state, c, t, a, U, V, y):
    """filter_ref.append in torch float64 (no failure branch): -> (state_out (SW,), d (M,), W (M, J), z (M,)), for autograd.
    An entry state with n == 0 starts from p = 0 whatever its t_last."""
    import torch

    M, J = U.shape
    tl, n, ld, q = state[0], state[1], state[2], state[3]
    Fv, S = state[HEAD:HEAD + J], state[HEAD + J:].reshape(J, J)
    empty = float(n.detach()) == 0.0
    d, W, z = [], [], []
    for m in range(M):
        p = torch.zeros_like(c) if empty else torch.exp(-c * (t[m] - tl))
        S = torch.outer(p, p) * S
        Fv = p * Fv
        g = S @ U[m]
        dm = a[m] - g @ U[m]
        w = (V[m] - g) / dm
        zm = y[m] - U[m] @ Fv
        S = S + dm * torch.outer(w, w)
        Fv = Fv + w * zm
        tl, n, ld, q = t[m], n + 1.0, ld + torch.log(dm), q + zm * zm / dm
        empty = False
        d.append(dm)
        W.append(w)
        z.append(zm)
    out = torch.cat([torch.stack([tl, n, ld, q]), Fv, S.reshape(-1)])
    return out, torch.stack(d), torch.stack(W), torch.stack(z)
