# -*- coding: utf-8 -*-
"""The fit WITHOUT the trial column(s), shared by periodogram.finish and transit.finish: with Z0 = L^-1 [A0 | y - mean]
(B, N, Q0 = P0 + 1) and <a, b> = sum_n a_n b_n / d_n,

    S0 = Z0^T diag(1/d) Z0   ->  G00 = S0[:P0, :P0] = L0 L0^T,  g0y = S0[:P0, P0],  s_yy = S0[P0, P0]
    v = L0^-1 g0y,   chi2_0 = s_yy - v^T v,   X = L0^-1 G0t   (G0t: the trial columns' products with A0, read from T)

so that a trial's M = Gtt - X^T X and r = gty - X^T v.  Nothing here raises beyond the shape checks."""
import torch

from .autograd import _RANK_TOL


def null_products(Z0, d):
    """S0 (B, Q0, Q0) = Z0^T diag(1/d) Z0 for Z0 (B, N, Q0), d (B, N)."""
    return torch.matmul((Z0 / d[..., None]).transpose(1, 2), Z0)


def null_fit(S0, T, ok, layout, cross):
    """(S0, T, bad, chi2_0, v, X, L0) for S0 (B, Q0, Q0) and T (B, K, width); `layout` = (K's name, the width in words, the
    width), e.g. ("F", "3 + 2 Q0", 3 + 2 * Q0).  `ok` (B,) | None: series to take at all; S0, T come back with the others
    replaced by the identity and zeros, and `bad` (B,) holds them and the series whose G00 is rank-deficient (to _RANK_TOL of
    its own diagonal) or did not factor.  `cross`: the first columns of the slices T[..., i:i + P0] that hold the trial
    columns' products with A0; X (B, P0, K) -- for two slices (B, P0, 2 K), side by side -- is L0^-1 of them and v (B, P0) =
    L0^-1 g0y; L0 (B, P0, P0) the factor of G00, the identity in a bad series; all three None when P0 = 0."""
    B, Q0 = S0.shape[0], S0.shape[-1]
    if S0.dim() != 3 or S0.shape[1] != Q0 or Q0 < 1:
        raise ValueError("Invalid shape: S0 (must be (B, Q0, Q0), Q0 >= 1)")
    K, words, width = layout
    if T.dim() != 3 or T.shape[0] != B or T.shape[2] != width:
        raise ValueError("Invalid shape: T (must be (B, %s, %s) = (%d, %s, %d))" % (K, words, B, K, width))
    P0 = Q0 - 1
    if ok is not None:
        S0 = torch.where(ok[:, None, None], S0, torch.eye(Q0, dtype=S0.dtype, device=S0.device))
        T = torch.where(ok[:, None, None], T, torch.zeros((), dtype=T.dtype, device=T.device))
    bad = torch.zeros(B, dtype=torch.bool, device=S0.device) if ok is None else ~ok
    s_yy = S0[:, P0, P0]
    if not P0:
        return S0, T, bad, s_yy, None, None, None
    G00, g0y = S0[:, :P0, :P0], S0[:, :P0, P0]
    L0, info = torch.linalg.cholesky_ex(G00)
    bad = bad | (info != 0)
    bad = bad | ~((torch.diagonal(L0, dim1=-2, dim2=-1) ** 2 > _RANK_TOL * torch.diagonal(G00, dim1=-2, dim2=-1)).all(dim=-1))
    # (the solves below stay finite: a bad series is solved against the identity, then overwritten)
    L0 = torch.where(bad[:, None, None], torch.eye(P0, dtype=S0.dtype, device=S0.device), L0)
    v = torch.linalg.solve_triangular(L0, g0y[..., None], upper=False)[..., 0]                        # (B, P0)
    Gt0 = [T[..., i:i + P0] for i in cross]
    Gt0 = torch.cat(Gt0, dim=1) if len(Gt0) > 1 else Gt0[0]
    X = torch.linalg.solve_triangular(L0, Gt0.transpose(1, 2), upper=False)
    return S0, T, bad, s_yy - (v * v).sum(dim=-1), v, X, L0
