# -*- coding: utf-8 -*-
"""Batched, device-resident operator API over the C-ABI (include/celerite2_amd.h).

Same op names and argument meaning as the reference's backend-op layer
(python/celerite2/definitions.json; jax/ops.py:40-72; pymc/ops.py:38-159) with a
leading batch dimension B of independent series.  All tensors are float64,
contiguous, on one HIP device; t may be (B,N) or shared (N,), c (B,J) or (J,).
Launches go on torch's current stream.  torch is plumbing here (device memory,
streams); the arithmetic is in the gfx950 kernels.
"""
import collections
import ctypes
import re

import torch

from . import _lib

__all__ = [
    "factor", "solve_lower", "solve_upper", "matmul_lower", "matmul_upper", "general_matmul_lower",
    "general_matmul_upper", "factor_rev", "solve_lower_rev", "solve_upper_rev", "matmul_lower_rev",
    "matmul_upper_rev", "get_celerite_matrices", "kernel_values", "colsumsq_over_d", "loglik", "loglik_grad", "loglik_grad_workspace", "condition", "dot_tril",
    "inverse_diag", "inverse_diag_rev", "get_celerite_matrices_rev", "explained_variance", "explained_variance_rev", "prior_draw",
    "general_matmul_lower_rev", "general_matmul_upper_rev",
    "kron_loglik", "kron_loglik_grad", "loglik_terms", "loglik_terms_grad",
    "TermProgram", "TermExpr", "term_coefficients", "term_coefficients_rev", "noise_mean_apply", "noise_mean_rev",
    "noise_mean_shift_apply", "noise_mean_shift_rev",
    "loglik_kernel_workspace", "loglik_kernel_grad",
]
# (the ops of include/celerite2_amd.h; the public ops of the later headers stand with their headers in _lib.HEADERS)


def _p(x):
    return ctypes.c_void_p(0 if x is None else x.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(*xs):
    dev = None
    for x in xs:
        if x is None:
            continue
        if not (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()):
            raise ValueError("celerite2_amd ops need contiguous float64 tensors on the GPU")
        if dev is None:
            dev = x.device
        elif x.device != dev:
            raise ValueError("celerite2_amd ops need every tensor on the same device")


def _shape(name, x, *allowed):
    """The reference raises "Invalid shape: <name>" for every argument (driver.cpp:40-46,94-99); so does this layer,
    BEFORE any pointer reaches a kernel (the kernels compute their strides from (B, N, J, nrhs) alone)."""
    if x is None:
        return
    if tuple(x.shape) not in allowed:
        raise ValueError("Invalid shape: %s (got %s, expected %s)"
                         % (name, tuple(x.shape), " or ".join(str(a) for a in allowed)))


def _forms(dims, spec):
    """The shapes a spec allows: a letter names a dimension of `dims`, | separates the form shared by the batch from the
    per-series one -- "N|BN" -> ((N,), (B, N))."""
    return tuple(tuple(map(dims.__getitem__, form)) for form in spec.split("|"))


def _shapes(dims, entries):
    """_shape for every (name, tensor, spec) entry, in the listed order (a None tensor is skipped).  Reads shapes only."""
    forms = {}   # (a spec becomes shapes once per call, not once per entry)
    for name, x, spec in entries:
        if x is not None:
            if spec not in forms:
                forms[spec] = _forms(dims, spec)
            if x.shape not in forms[spec]:
                _shape(name, x, *forms[spec])


def _args(dims, ins, outs=()):
    """The checks of one op on its (name, tensor, spec) entries: dtype, device and contiguity of all of them, then their
    shapes in the listed order (`ins` before `outs`), then -- for an op that names its outputs -- _no_alias."""
    entries = list(ins) + list(outs)
    _chk(*(x for _, x, _ in entries))
    _shapes(dims, entries)
    if outs:
        _no_alias(outs, ins)


def _empty(dev, dims, *specs):
    """Fresh float64 tensors of the given specs (outputs are always per series: the last form of a spec)."""
    return tuple(torch.empty(_forms(dims, s)[-1], dtype=torch.float64, device=dev) for s in specs)


def _named(spec, tensors):
    """The (name, tensor, spec) entries of the tensors an output spec -- a dict name -> shape spec -- describes."""
    return [(name, x, s) for (name, s), x in zip(spec.items(), tensors)]


def _flag(B, dev):
    return torch.empty(B, dtype=torch.int32, device=dev)


def _bs(x, per):
    """(tensor, batch stride in elements): 0 when shared by the batch."""
    return 0 if x.dim() == 1 else per


def _dims(U):
    if U.dim() != 3:
        raise ValueError("U must be (B, N, J)")
    return U.shape


_T, _C = "N|BN", "J|BJ"   # t and c: shared by the batch or per series
_LOGLIK_IN = dict(t=_T, c=_C, a="BN", U="BNJ", V="BNJ", y="BN")
_LOGLIK_GRADS = dict(bt="BN", bc="BJ", ba="BN", bU="BNJ", bV="BNJ", by="BN")
_COEFS = ("BR", "BR", "BC", "BC", "BC", "BC")   # ar, cr (B, Jr); ac, bc, cc, dc (B, Jc)


def factor(t, c, a, U, V, d=None, W=None, S=None, *, workspace=False):
    """Batched core::factor.  Returns (d, W, flag) or (d, W, S, flag); d may alias a, W may alias V."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    d = torch.empty_like(a) if d is None else d
    W = torch.empty_like(V) if W is None else W
    if workspace and S is None:
        S, = _empty(U.device, dims, "BNJJ")
    flag = _flag(B, U.device)
    _args(dims, [("t", t, _T), ("c", c, _C), ("a", a, "BN"), ("U", U, "BNJ"), ("V", V, "BNJ"), ("d", d, "BN"), ("W", W, "BNJ"),
                 ("S", S, "BNJJ")])
    rc = _lib.load().c2_factor(B, N, J, t, _bs(t, N), c, _bs(c, J), a, U, V, d, W, S, flag, _stream())
    _lib.check(rc, "factor")
    return (d, W, S, flag) if S is not None else (d, W, flag)


def condition(t, c, a, U, V):
    """kappa[b] = max_n a_n / d_n per series (+inf where the factorisation fails), and the factor flag: whether north_star's
    1e-10 agreement with the reference is attainable in float64 for these inputs (include/celerite2_amd.h, c2_condition:
    any evaluation order carries ~0.4 eps kappa^2 of the largest gradient entry).  Returns (kappa, flag)."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    kappa, = _empty(U.device, dims, "B")
    flag = _flag(B, U.device)
    _args(dims, [("t", t, _T), ("c", c, _C), ("a", a, "BN"), ("U", U, "BNJ"), ("V", V, "BNJ")])
    rc = _lib.load().c2_condition(B, N, J, t, _bs(t, N), c, _bs(c, J), a, U, V, kappa, flag, _stream())
    _lib.check(rc, "condition")
    return kappa, flag


def _sweep(name, matmul):
    def op(t, c, U, W, Y, Z=None, F=None, *, workspace=False, zero_z=False):
        B, N, J = _dims(U)
        if Y.dim() != 3:
            raise ValueError("Invalid shape: Y (must be (B, N, nrhs))")
        nrhs = Y.shape[-1]
        dims = dict(B=B, N=N, J=J, K=nrhs)
        if Z is None:
            Z = torch.zeros_like(Y) if matmul else torch.empty_like(Y)
        if workspace and F is None:
            F, = _empty(U.device, dims, "BNJK")
        _args(dims, [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("Y", Y, "BNK"), ("Z", Z, "BNK"),
                     ("F", F, "BNJK")])
        flags = (bool(zero_z),) if matmul else ()
        rc = getattr(_lib.load(), "c2_" + name)(B, N, J, nrhs, t, _bs(t, N), c, _bs(c, J), U, W, Y, Z, F, *flags, _stream())
        _lib.check(rc, name)
        return (Z, F) if F is not None else Z
    op.__name__ = name
    return op


solve_lower = _sweep("solve_lower", False)
solve_upper = _sweep("solve_upper", False)
matmul_lower = _sweep("matmul_lower", True)
matmul_upper = _sweep("matmul_upper", True)


def _general_dims(U, V, Y):
    B, N, J = _dims(U)
    if V.dim() != 3 or Y.dim() != 3:
        raise ValueError("Invalid shape: V must be (B, M, J) and Y (B, M, nrhs)")
    return dict(B=B, N=N, M=V.shape[1], J=J, K=Y.shape[-1])


def _general(name):
    def op(t1, t2, c, U, V, Y, Z=None, F=None, *, workspace=False, zero_z=False):
        dims = _general_dims(U, V, Y)
        B, N, M, J, nrhs = dims.values()
        if Z is None:
            Z = torch.zeros((B, N, nrhs), dtype=torch.float64, device=U.device)
        if workspace and F is None:
            F = torch.zeros((B, M, J, nrhs), dtype=torch.float64, device=U.device)
        _args(dims, [("t1", t1, _T), ("t2", t2, "M|BM"), ("c", c, _C), ("U", U, "BNJ"), ("V", V, "BMJ"), ("Y", Y, "BMK"),
                     ("Z", Z, "BNK"), ("F", F, "BMJK")])
        rc = getattr(_lib.load(), "c2_" + name)(B, N, M, J, nrhs, t1, _bs(t1, N), t2, _bs(t2, M), c, _bs(c, J), U, V, Y, Z, F,
                                                bool(zero_z), _stream())
        _lib.check(rc, name)
        return (Z, F) if F is not None else Z
    op.__name__ = name
    return op


general_matmul_lower = _general("general_matmul_lower")
general_matmul_upper = _general("general_matmul_upper")


def factor_rev(t, c, a, U, V, d, W, S, bd, bW):
    """Batched core::factor_rev (reverse.hpp:10-85).  `S` is the workspace `factor(..., workspace=True)` returned.  The
    row-by-row kernel reads every C-th row of it and replays the rows in between from d, W; on small batches of series of
    512 rows and more the reverse pass runs parallel along time and replays ALL its states from d, W --
    `S` is then only read if the device-side verification of that pass fails and the row-by-row kernel recomputes the
    batch behind it.  Either way the result is that of the reference on the same (t, c, U, d, W, bd, bW)."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    bt, bc, ba, bU, bV = _empty(U.device, dims, "BN", "BJ", "BN", "BNJ", "BNJ")
    _args(dims, [("t", t, _T), ("c", c, _C), ("a", a, "BN"), ("U", U, "BNJ"), ("V", V, "BNJ"), ("d", d, "BN"), ("W", W, "BNJ"),
                 ("S", S, "BNJJ"), ("bd", bd, "BN"), ("bW", bW, "BNJ")])
    rc = _lib.load().c2_factor_rev(B, N, J, t, _bs(t, N), c, _bs(c, J), a, U, V, d, W, S, bd, bW, bt, bc, ba, bU, bV, _stream())
    _lib.check(rc, "factor_rev")
    return bt, bc, ba, bU, bV


def _sweep_rev(name):
    def op(t, c, U, W, Y, Z, F, bZ):
        B, N, J = _dims(U)
        if Y.dim() != 3:
            raise ValueError("Invalid shape: Y (must be (B, N, nrhs))")
        nrhs = Y.shape[-1]
        dims = dict(B=B, N=N, J=J, K=nrhs)
        bt, bc, bU, bW, bY = _empty(U.device, dims, "BN", "BJ", "BNJ", "BNJ", "BNK")
        _args(dims, [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("Y", Y, "BNK"), ("Z", Z, "BNK"),
                     ("F", F, "BNJK"), ("bZ", bZ, "BNK")])
        rc = getattr(_lib.load(), "c2_" + name)(B, N, J, nrhs, t, _bs(t, N), c, _bs(c, J), U, W, Y, Z, F, bZ, bt, bc, bU, bW,
                                                bY, _stream())
        _lib.check(rc, name)
        return bt, bc, bU, bW, bY
    op.__name__ = name
    return op


solve_lower_rev = _sweep_rev("solve_lower_rev")
solve_upper_rev = _sweep_rev("solve_upper_rev")
matmul_lower_rev = _sweep_rev("matmul_lower_rev")
matmul_upper_rev = _sweep_rev("matmul_upper_rev")


def get_celerite_matrices(ar, ac, bc, dc, x, diag):
    """Batched driver.get_celerite_matrices.  ar (Jr,)|(B,Jr); ac,bc,dc (Jc,)|(B,Jc); x (N,)|(B,N); diag (B,N)."""
    if diag.dim() != 2:
        raise ValueError("Invalid shape: diag (must be (B, N))")
    B, N = diag.shape
    Jr, Jc = ar.shape[-1], ac.shape[-1]
    J = Jr + 2 * Jc
    batched = ar.dim() == 2 or ac.dim() == 2
    if batched and (ar.dim() != 2 or ac.dim() != 2 or bc.dim() != 2 or dc.dim() != 2):
        raise ValueError("coefficients must be all shared or all per-series")
    dev = diag.device
    a = torch.empty((B, N), dtype=torch.float64, device=dev)
    U = torch.empty((B, N, J), dtype=torch.float64, device=dev)
    V = torch.empty((B, N, J), dtype=torch.float64, device=dev)
    _chk(ar, ac, bc, dc, x, diag)
    _shape("x", x, (N,), (B, N))
    _shape("ar", ar, (Jr,), (B, Jr))
    for nm, v in (("ac", ac), ("bc", bc), ("dc", dc)):
        _shape(nm, v, (Jc,), (B, Jc))
    rc = _lib.load().c2_get_celerite_matrices(B, N, Jr, Jc, ar if Jr else None, ac if Jc else None, bc if Jc else None,
                                              dc if Jc else None, batched, x, _bs(x, N), diag, a, U, V, _stream())
    _lib.check(rc, "get_celerite_matrices")
    return a, U, V


def kernel_values(ar, cr, ac, bc, cc, dc, t1, t2, B=None):
    """K[b, n, m] = k(t1[b, n] - t2[b, m]) (terms.py:58-79 on two grids): coefficients (Jr,)|(B,Jr) / (Jc,)|(B,Jc), t1 (N,)|(B,N),
    t2 (M,)|(B,M); B is taken from whichever argument carries it (or the keyword when everything is shared)."""
    Jr, Jc = ar.shape[-1], ac.shape[-1]
    batched = ar.dim() == 2 or ac.dim() == 2
    if batched and any(v.dim() != 2 for v in (ar, cr, ac, bc, cc, dc)):
        raise ValueError("coefficients must be all shared or all per-series")
    for v in (t1, t2, ar, ac):
        if v.dim() == 2:
            B = v.shape[0] if B is None else B
    if B is None:
        B = 1
    N, M = t1.shape[-1], t2.shape[-1]
    _chk(ar, cr, ac, bc, cc, dc, t1, t2)
    _shape("t1", t1, (N,), (B, N)); _shape("t2", t2, (M,), (B, M))
    for nm, v, w in (("ar", ar, Jr), ("cr", cr, Jr), ("ac", ac, Jc), ("bc", bc, Jc), ("cc", cc, Jc), ("dc", dc, Jc)):
        _shape(nm, v, (w,), (B, w))
    K = torch.empty((B, N, M), dtype=torch.float64, device=t1.device)
    rc = _lib.load().c2_kernel_values(B, N, M, Jr, Jc, *_coef_ptrs(ar, cr, ac, bc, cc, dc, Jr, Jc), batched, t1, _bs(t1, N), t2,
                                      _bs(t2, M), K, _stream())
    _lib.check(rc, "kernel_values")
    return K


def colsumsq_over_d(Z, d):
    """out[b, m] = sum_n Z[b, n, m]^2 / d[b, n]  (Z (B, N, M), d (B, N)): the quadratic form of the predictive variance from the
    lower solve alone (c2_colsumsq_over_d; core.py:134-140)."""
    if Z.dim() != 3:
        raise ValueError("Invalid shape: Z (must be (B, N, M))")
    B, N, M = Z.shape
    _chk(Z, d)
    _shape("d", d, (B, N))
    out = torch.empty((B, M), dtype=torch.float64, device=Z.device)
    rc = _lib.load().c2_colsumsq_over_d(B, N, M, Z, d, out, _stream())
    _lib.check(rc, "colsumsq_over_d")
    return out


def loglik(t, c, a, U, V, y):
    """Fused batched log-likelihood.  Returns (ll (B,), flag (B,) int32)."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    ll, = _empty(U.device, dims, "B")
    flag = _flag(B, U.device)
    _args(dims, _named(_LOGLIK_IN, (t, c, a, U, V, y)))
    rc = _lib.load().c2_loglik(B, N, J, t, _bs(t, N), c, _bs(c, J), a, U, V, y, ll, flag, _stream())
    _lib.check(rc, "loglik")
    return ll, flag


def loglik_grad_workspace(B, N, J, device):
    nbytes = _lib.load().c2_loglik_grad_workspace_bytes(B, N, J)
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def loglik_grad_buffers(t, c, a, U, V, y, *, candidates=3):
    """Workspace and gradient arrays for repeated `loglik_grad(..., work=, out=)` calls on one shape, PLACED by
    measurement.  A chip-filling step streams a dozen 2 - 16 GiB arrays at once, and WHERE in the 288 GB of HBM the
    workspace and the gradient arrays lie relative to the inputs moves its time by 6 - 10 % -- deterministically: the same
    process re-allocating the same arrays behind a spacer of a few tens of GiB switches between 28.2 and 31.5 ms for
    65536 x 4096 x 8, shifts of MiB change nothing, a plain copy between 16-GiB buffers does not care
    (profiles/r04_headline_spread.md).  So: time one
    step on the allocator's own placement, then on fresh allocations behind spacers of 24 and 48 GiB (more with
    `candidates`), and keep the fastest.  Returns (work, out, report) -- `report` lists every candidate's time."""
    B, N, J = _dims(U)
    dev = U.device

    def fresh():
        return loglik_grad_workspace(B, N, J, dev), _empty(dev, dict(B=B, N=N, J=J), *_LOGLIK_GRADS.values())

    def one_step_ms(w_, o_):
        for _ in range(2):
            loglik_grad(t, c, a, U, V, y, work=w_, out=o_)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loglik_grad(t, c, a, U, V, y, work=w_, out=o_)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    work, out = fresh()
    cand = [{"spacer_GiB": 0, "ms": one_step_ms(work, out)}]
    best_ms = cand[0]["ms"]
    # spacers scaled to the memory that is actually free (24 / 48 GiB on a 288-GB part holding the bench shape)
    free_gib = torch.cuda.mem_get_info(dev)[0] / 2**30
    need_gib = (work.numel() * 8 + sum(o.numel() for o in out) * 8) / 2**30
    room = max(0.0, free_gib - need_gib - 2.0)
    for gib in [g for g in (24, 48, 12, 72, 96) if g <= room][:max(0, candidates - 1)]:
        sp = w_ = o_ = None
        try:
            sp = torch.empty(gib * 2**30, dtype=torch.uint8, device=dev)
            w_, o_ = fresh()
        except RuntimeError:   # (not enough memory left for a second set behind this spacer)
            del sp, w_, o_
            torch.cuda.empty_cache()
            break
        del sp                 # (only the position of the arrays matters: the spacer itself goes back at once)
        ms_ = one_step_ms(w_, o_)
        cand.append({"spacer_GiB": gib, "ms": ms_})
        if ms_ < best_ms:
            best_ms, work, out = ms_, w_, o_
        del w_, o_
        torch.cuda.empty_cache()   # the next candidate must not simply get the loser's blocks back
    return work, out, {"candidates": cand, "chosen_ms": best_ms,
                       "note": "setup, untimed: one step per candidate placement of the workspace and the gradient arrays "
                               "(behind spacers of tens of GiB; profiles/r04_headline_spread.md)"}


def loglik_grad(t, c, a, U, V, y, *, work=None, out=None):
    """Fused batched log-likelihood + gradient.  Returns (ll, (bt, bc, ba, bU, bV, by), flag)."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    dev = U.device
    if work is None:
        work = loglik_grad_workspace(B, N, J, dev)
    if out is None:
        out = _empty(dev, dims, *_LOGLIK_GRADS.values())
    bt, bc, ba, bU, bV, by = out
    ll, = _empty(dev, dims, "B")
    flag = _flag(B, dev)
    _args(dims, _named(_LOGLIK_IN, (t, c, a, U, V, y)) + _named(_LOGLIK_GRADS, out))
    rc = _lib.load().c2_loglik_grad(B, N, J, t, _bs(t, N), c, _bs(c, J), a, U, V, y, ll, bt, bc, ba, bU, bV, by, flag, work,
                                    work.numel() * 8, _stream())
    _lib.check(rc, "loglik_grad")
    return ll, out, flag


def dot_tril(t, c, U, W, d, Y, Z=None):
    """Z = L sqrt(D) Y (numpy.py:100-102).  Y may be passed as Z for in-place use."""
    B, N, J = _dims(U)
    if Y.dim() != 3:
        raise ValueError("Invalid shape: Y (must be (B, N, nrhs))")
    nrhs = Y.shape[-1]
    Z = torch.empty_like(Y) if Z is None else Z
    _args(dict(B=B, N=N, J=J, K=nrhs), [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("d", d, "BN"),
                                        ("Y", Y, "BNK"), ("Z", Z, "BNK")])
    rc = _lib.load().c2_dot_tril(B, N, J, nrhs, t, _bs(t, N), c, _bs(c, J), U, W, d, Y, Z, _stream())
    _lib.check(rc, "dot_tril")
    return Z


def whitened_gram(t, c, U, W, d, A, y=None, S=None):
    """S (B, Q, Q) = [A | y]^T (K + D)^-1 [A | y] from the factors (d, W) of `factor`, in one forward sweep that keeps S in
    registers and never writes L^-1 [A | y] (c2_whitened_gram, csrc/c2_gram.hip).  A (N, P) shared by the batch or (B, N, P);
    y (B, N) or None: Q = P + 1 with y (its column last), P without.  Both triangles are stored and equal to the bit.
    Caller-owned `S` is accepted (nothing is allocated then: capturable in a HIP graph); it must not alias an input.
    J <= 32 and Q <= 32.  No atomics: two calls give identical bits."""
    B, N, J = _dims(U)
    if A.dim() not in (2, 3):
        raise ValueError("Invalid shape: A (must be (N, P) or (B, N, P))")
    P = A.shape[-1]
    dims = dict(B=B, N=N, J=J, P=P, Q=P + (y is not None))
    if S is None:
        S, = _empty(U.device, dims, "BQQ")
    _args(dims, [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("d", d, "BN"), ("A", A, "NP|BNP"), ("y", y, "BN")],
          [("S", S, "BQQ")])
    rc = _lib.load().c2_whitened_gram(B, N, J, P, t, _bs(t, N), c, _bs(c, J), U, W, d, A, 0 if A.dim() == 2 else N * P, y, S,
                                      _stream())
    _lib.check(rc, "whitened_gram")
    return S


# THE KINDS OF TRIAL: what the sweep (c2_whitened_*) and the projection (c2_trial_projections, c2_shape_projections) of each
# take.  code: C2_TRIAL_* of celerite2_amd_trials.h (None: the kind has entry points of its own); words: doubles per trial;
# columns: C; width: T's last axis as (constant, per column of Z0); draws: vectors per wavefront of the projection
# (C2_TRIAL_*_DRAWS, C2_SHAPE_DRAWS); bank: whether a shape bank goes with the trials.  tests/test_significance.py holds it
# to the headers.
_TrialKind = collections.namedtuple("_TrialKind", "code words columns width draws bank")
_TRIAL_TABLE = {"periodogram": _TrialKind(0, 1, 2, (3, 2), 64, False), "transit": _TrialKind(1, 4, 1, (1, 1), 32, False),
                "keplerian": _TrialKind(2, 3, 2, (3, 2), 128, False), "shape": _TrialKind(None, 4, 1, (1, 1), 32, True)}
# kind -> (C2_TRIAL_*, doubles per trial, columns per trial C, vectors per wavefront C2_TRIAL_*_DRAWS) of celerite2_amd_trials.h
TRIAL_KINDS = {k: (v.code, v.words, v.columns, v.draws) for k, v in _TRIAL_TABLE.items() if v.code is not None}
SHAPE_MAX_NODES, SHAPE_DRAWS = 1024, _TRIAL_TABLE["shape"].draws   # C2_SHAPE_MAX_NODES, C2_SHAPE_DRAWS of celerite2_amd_shapes.h


def _trial_grid(kd, trials, name="trials", k="K"):
    """(K, shape spec, batch stride) of the trials of kind `kd`: (K,) | (B, K) at one double per trial, (K, words) |
    (B, K, words) otherwise."""
    lead = 1 if kd.words == 1 else 2
    if trials.dim() not in (lead, lead + 1) or (lead == 2 and trials.shape[-1] != kd.words):
        raise ValueError("Invalid shape: %s (must be %s)" % (name, "(%s,) or (B, %s)" % (k, k) if lead == 1 else
                                                             "(K, %d) or (B, K, %d)" % (kd.words, kd.words)))
    K = trials.shape[-lead]
    return K, "K|BK" if lead == 1 else "KF|BKF", 0 if trials.dim() == lead else kd.words * K


def _bank(shapes, B):
    """(NS, S, batch stride) of a shape bank (NS, S) | (B, NS, S); its limits are checked here, from its shape."""
    if shapes.dim() not in (2, 3) or (shapes.dim() == 3 and shapes.shape[0] != B):
        raise ValueError("Invalid shape: shapes (must be (NS, S) or (B, NS, S) with B = %d)" % B)
    NS, S = shapes.shape[-2:]
    if NS < 1 or S < 2:
        raise ValueError("Invalid shape: shapes (NS >= 1 shapes of S >= 2 nodes; got NS = %d, S = %d)" % (NS, S))
    if NS * S > SHAPE_MAX_NODES:
        raise ValueError("Invalid shape: shapes (NS * S <= %d; got %d * %d = %d -- a larger bank takes several calls)"
                         % (SHAPE_MAX_NODES, NS, S, NS * S))
    return NS, S, 0 if shapes.dim() == 2 else NS * S


def _whitened(op, kind, t, c, U, W, d, Z0, trials, out, *, t_ref=None, shapes=None, name="trials", k="K", count=()):
    """The sweep c2_<op> of one kind of _TRIAL_TABLE (or a _TrialKind outside it): T (B, K, width).  `count`: integers that
    follow K in the call; `t_ref` goes before T, the bank after it."""
    kd = _TRIAL_TABLE[kind] if isinstance(kind, str) else kind
    B, N, J = _dims(U)
    if Z0.dim() != 3:
        raise ValueError("Invalid shape: Z0 (must be (B, N, Q0))")
    K, spec, tr_bs = _trial_grid(kd, trials, name, k)
    Q0 = Z0.shape[-1]
    dims = dict(B=B, N=N, J=J, Q=Q0, K=K, F=kd.words, R=kd.width[0] + kd.width[1] * Q0)
    ins = [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("d", d, "BN"), ("Z0", Z0, "BNQ"), (name, trials, spec)]
    bank = ()
    if kd.bank:
        NS, S, sh_bs = _bank(shapes, B)
        dims.update(H=NS, S=S)
        ins.append(("shapes", shapes, "HS|BHS"))
        bank = (shapes, sh_bs, NS, S)
    if out is None:
        out, = _empty(U.device, dims, "BKR")
    _args(dims, ins, [("out", out, "BKR")])
    rc = getattr(_lib.load(), "c2_" + op)(B, N, J, Q0, K, *count, t, _bs(t, N), c, _bs(c, J), U, W, d, Z0, trials, tr_bs,
                                          *(() if t_ref is None else (float(t_ref),)), out, *bank, _stream())
    _lib.check(rc, op)
    return out


def _projections(op, kind, t, alpha, trials, out, *, t_ref=0.0, shapes=None):
    """The projection of one kind of _TRIAL_TABLE: P (B, K, C, R)."""
    kd = _TRIAL_TABLE[kind]
    if alpha.dim() != 3:
        raise ValueError("Invalid shape: alpha (must be (B, N, R))")
    B, N, R = alpha.shape
    K, spec, tr_bs = _trial_grid(kd, trials)
    dims = dict(B=B, N=N, R=R, K=K, F=kd.words, C=kd.columns)
    ins = [("t", t, _T), ("alpha", alpha, "BNR"), ("trials", trials, spec)]
    if kd.bank:
        NS, S, sh_bs = _bank(shapes, B)
        dims.update(H=NS, S=S)
        ins.append(("shapes", shapes, "HS|BHS"))
    if out is None:
        out, = _empty(alpha.device, dims, "BKCR")
    _args(dims, ins, [("out", out, "BKCR")])
    if kd.bank:
        rc = _lib.load().c2_shape_projections(B, N, K, R, t, _bs(t, N), trials, tr_bs, alpha, out, shapes, sh_bs, NS, S, _stream())
    else:
        rc = _lib.load().c2_trial_projections(kd.code, B, N, K, R, t, _bs(t, N), trials, tr_bs, float(t_ref), alpha, out, _stream())
    _lib.check(rc, op)
    return out


def whitened_sinusoids(t, c, U, W, d, Z0, freq, *, t_ref=0.0, out=None):
    """T (B, F, 3 + 2 Q0): for every series and every ANGULAR trial frequency freq ((F,) shared by the batch or (B, F)), with
    z_c = L^-1 cos(w (t - t_ref)), z_s = L^-1 sin(w (t - t_ref)) and <a, b> = sum_n a_n b_n / d_n,

        T[b, f] = [<z_c, z_c>, <z_c, z_s>, <z_s, z_s>, <z_c, Z0[:, k]> for k < Q0, <z_s, Z0[:, k]> for k < Q0]

    from the factors (d, W) of `factor` and Z0 (B, N, Q0) = solve_lower of [A0 | y - mean], in one forward sweep that forms the
    two columns in registers, one lane per frequency (c2_whitened_sinusoids, csrc/c2_periodogram.hip; the header has the rule
    for the phase).  What the periodogram under correlated noise reads (celerite2_amd/periodogram.py).  Caller-owned `out` is
    accepted (nothing is allocated then: capturable in a HIP graph); it must not alias an input.  J <= 32 and 1 <= Q0 <= 8.
    No atomics: two calls give identical bits."""
    return _whitened("whitened_sinusoids", "periodogram", t, c, U, W, d, Z0, freq, out, t_ref=t_ref, name="freq", k="F")


# C2_HARMONICS_MAX of include/celerite2_amd_harmonics.h
HARMONICS_MAX = int(re.search(r"^#define\s+C2_HARMONICS_MAX\s+(\d+)", _lib.header_text("harmonics"), flags=re.M).group(1))


def whitened_harmonics(t, c, U, W, d, Z0, freq, nterms, *, t_ref=0.0, out=None):
    """T (B, F, H (2 H + 1) + 2 H Q0) for H = `nterms` harmonics of every ANGULAR trial frequency freq ((F,) shared by the batch
    or (B, F)): with the 2 H columns ordered (c_1, s_1, ..., c_H, s_H), c_h = cos x_h, s_h = sin x_h at the phase of
    `whitened_sinusoids` for the frequency fl(h w), z_i = L^-1 (column i) and <a, b> = sum_n a_n b_n / d_n,

        T[b, f] = [<z_i, z_j> for 0 <= i <= j < 2 H (row-major over the upper triangle), <z_i, Z0[:, k]> for i < 2 H, k < Q0]

    from the factors (d, W) of `factor` and Z0 (B, N, Q0) = solve_lower of [A0 | y - mean], in one forward sweep that forms
    the columns in registers, H neighbouring lanes per frequency (c2_whitened_harmonics, csrc/c2_harmonics.hip; the header has
    the column rule).  nterms = 1 is `whitened_sinusoids` to the bit, and what T holds about harmonic h alone is
    `whitened_sinusoids` at h * freq to the bit.  What the multi-harmonic periodogram reads (celerite2_amd/harmonics.py).
    Caller-owned `out` is accepted (nothing is allocated then: capturable in a HIP graph); it must not alias an input.
    1 <= nterms <= 4, J <= 32 and 1 <= Q0 <= 8.  No atomics: two calls give identical bits."""
    if isinstance(nterms, bool) or not isinstance(nterms, int) or not 1 <= nterms <= HARMONICS_MAX:
        raise ValueError("nterms must be an integer from 1 to %d (got %r)" % (HARMONICS_MAX, nterms))
    kind = _TrialKind(None, 1, 2 * nterms, (nterms * (2 * nterms + 1), 2 * nterms), None, False)
    return _whitened("whitened_harmonics", kind, t, c, U, W, d, Z0, freq, out, t_ref=t_ref, name="freq", k="F", count=(nterms,))


# H -> C2_HARMONIC_DRAWS_H of include/celerite2_amd_harmonic_trials.h: the draws a wavefront takes
HARMONIC_DRAWS = {int(h): int(v) for h, v in re.findall(r"^#define\s+C2_HARMONIC_DRAWS_(\d+)\s+(\d+)",
                                                         _lib.header_text("harmonic_trials"), flags=re.M)}
_HARMONIC_MAX_P0 = 7


def _harmonic_trials(t, alpha, freq, nterms):
    """(dims, the entries of t, alpha, freq, freq's batch stride) of the two ops of celerite2_amd_harmonic_trials.h."""
    if isinstance(nterms, bool) or not isinstance(nterms, int) or not 1 <= nterms <= HARMONICS_MAX:
        raise ValueError("nterms must be an integer from 1 to %d (got %r)" % (HARMONICS_MAX, nterms))
    if alpha.dim() != 3:
        raise ValueError("Invalid shape: alpha (must be (B, N, R))")
    B, N, R = alpha.shape
    K, spec, f_bs = _trial_grid(_TRIAL_TABLE["periodogram"], freq, "freq", "F")
    dims = dict(B=B, N=N, R=R, K=K, C=2 * nterms, L=nterms * (2 * nterms + 1))
    return dims, [("t", t, _T), ("alpha", alpha, "BNR"), ("freq", freq, spec)], f_bs


def harmonic_projections(t, alpha, freq, nterms, *, t_ref=0.0, out=None):
    """P (B, F, 2 H, R): P[b, f, i, r] = sum_n col_i(f; t[b, n]) alpha[b, n, r] for alpha (B, N, R), t (N,) shared by the
    batch or (B, N), the ANGULAR frequencies freq (F,) | (B, F) and H = `nterms` harmonics, the columns ordered
    (c_1, s_1, ..., c_H, s_H) as `whitened_harmonics` has them: `trial_projections("periodogram", ...)` at every h * freq in
    one pass over alpha (c2_harmonic_projections, csrc/c2_harmonic_trials.hip), and P[:, :, 2 h - 2:2 h] is that call's result
    to the bit.  Caller-owned `out` is accepted (nothing is allocated then: capturable in a HIP graph); it must not alias an
    input.  1 <= nterms <= 4.  No atomics: two calls give identical bits."""
    dims, ins, f_bs = _harmonic_trials(t, alpha, freq, nterms)
    if out is None:
        out, = _empty(alpha.device, dims, "BKCR")
    _args(dims, ins, [("out", out, "BKCR")])
    B, N, R, F = dims["B"], dims["N"], dims["R"], dims["K"]
    rc = _lib.load().c2_harmonic_projections(B, N, F, nterms, R, t, _bs(t, N), freq, f_bs, float(t_ref), alpha, out, _stream())
    _lib.check(rc, "harmonic_projections")
    return out


def harmonic_null_chi2(t, alpha, freq, nterms, Lm, Xt=None, V=None, *, t_ref=0.0, out=None):
    """D (B, F, R): the multi-harmonic dchi2 of R series at every frequency, finished in registers from the projections of
    `harmonic_projections` without writing them (c2_harmonic_null_chi2, csrc/c2_harmonic_trials.hip; the header has the
    rule line by line).  alpha (B, N, R), t, freq, nterms as there; Lm (B, F, H (2 H + 1)), Xt (B, F, 2 H, P0) and V (B, P0, R)
    as harmonics.null_factors and harmonics.null_draws give them (Xt and V None when P0 = 0; P0 <= 7).  NaN in Lm at a
    frequency gives NaN at every draw of that frequency and nowhere else.  What gp.search_significance(..., nterms=H) reads.
    Caller-owned `out` is accepted (nothing is allocated then: capturable in a HIP graph); it must not alias an input.  No
    atomics: two calls give identical bits."""
    dims, ins, f_bs = _harmonic_trials(t, alpha, freq, nterms)
    if (Xt is None) != (V is None):
        raise ValueError("Invalid shape: Xt, V (both None when P0 = 0, else (B, F, 2 H, P0) and (B, P0, R))")
    P0 = 0 if V is None else (V.shape[1] if V.dim() == 3 else -1)
    if not 0 <= P0 <= _HARMONIC_MAX_P0:
        raise ValueError("Invalid shape: V (must be (B, P0, R) with P0 <= %d)" % _HARMONIC_MAX_P0)
    dims["P"] = P0
    ins += [("Lm", Lm, "BKL"), ("Xt", Xt, "BKCP"), ("V", V, "BPR")]
    if out is None:
        out, = _empty(alpha.device, dims, "BKR")
    _args(dims, ins, [("out", out, "BKR")])
    B, N, R, F = dims["B"], dims["N"], dims["R"], dims["K"]
    rc = _lib.load().c2_harmonic_null_chi2(B, N, F, nterms, R, P0, t, _bs(t, N), freq, f_bs, float(t_ref), alpha, Lm, Xt, V, out,
                                           _stream())
    _lib.check(rc, "harmonic_null_chi2")
    return out


def whitened_transits(t, c, U, W, d, Z0, trials, *, out=None):
    """T (B, K, 1 + Q0): for every series and every trial (period P, epoch t0, duration w, ingress tau) of `trials` ((K, 4)
    shared by the batch or (B, K, 4)), with z = L^-1 b_k(t) and <a, b> = sum_n a_n b_n / d_n,

        T[b, k] = [<z, z>, <z, Z0[:, j]> for j < Q0]

    from the factors (d, W) of `factor` and Z0 (B, N, Q0) = solve_lower of [A0 | y - mean], in one forward sweep that forms
    the box (tau = 0) or trapezoid template b_k in registers, one lane per trial (c2_whitened_transits, csrc/c2_transit.hip;
    the header has the rule for the template; P = 0 is a single event, P > 0 folds).  What the transit search under
    correlated noise reads (celerite2_amd/transit.py).  Caller-owned `out` is accepted (nothing is allocated then: capturable
    in a HIP graph); it must not alias an input.  J <= 32 and 1 <= Q0 <= 8.  No atomics: two calls give identical bits."""
    return _whitened("whitened_transits", "transit", t, c, U, W, d, Z0, trials, out)


def whitened_keplerians(t, c, U, W, d, Z0, trials, *, out=None):
    """T (B, K, 3 + 2 Q0): for every series and every trial (angular frequency w, eccentricity e, time of periastron tp) of
    `trials` ((K, 3) shared by the batch or (B, K, 3)), with nu(t) the true anomaly of that orbit, z_c = L^-1 cos nu,
    z_s = L^-1 sin nu and <a, b> = sum_n a_n b_n / d_n,

        T[b, k] = [<z_c, z_c>, <z_c, z_s>, <z_s, z_s>, <z_c, Z0[:, j]> for j < Q0, <z_s, Z0[:, j]> for j < Q0]

    (the layout of `whitened_sinusoids`) from the factors (d, W) of `factor` and Z0 (B, N, Q0) = solve_lower of
    [A0 | y - mean], in one forward sweep that solves Kepler's equation and forms the two columns in registers, one lane per
    trial (c2_whitened_keplerians, csrc/c2_kepler.hip; the header has the rule for the columns and the solver).  What the
    Keplerian search under correlated noise reads (celerite2_amd/kepler.py).  Every trial is evaluated as written; the
    domain w > 0, 0 <= e <= 0.99 is the caller's to mask.  Caller-owned `out` is accepted (nothing is allocated then:
    capturable in a HIP graph); it must not alias an input.  J <= 32 and 1 <= Q0 <= 8.  No atomics: two calls give identical
    bits."""
    return _whitened("whitened_keplerians", "keplerian", t, c, U, W, d, Z0, trials, out)


def whitened_shapes(t, c, U, W, d, Z0, trials, shapes, *, out=None):
    """T (B, K, 1 + Q0): for every series and every trial (period P, epoch t0, width w, shape index s) of `trials` ((K, 4)
    shared by the batch or (B, K, 4)) and the bank `shapes` ((NS, S) shared or (B, NS, S): NS event profiles tabulated on S
    uniform nodes from the leading to the trailing edge; NS * S <= 1024), with z = L^-1 b_k(t) and
    <a, b> = sum_n a_n b_n / d_n,

        T[b, k] = [<z, z>, <z, Z0[:, j]> for j < Q0]

    (the layout of `whitened_transits`) from the factors (d, W) of `factor` and Z0 (B, N, Q0) = solve_lower of
    [A0 | y - mean], in one forward sweep that interpolates the shape in registers, one lane per trial (c2_whitened_shapes,
    csrc/c2_shapes.hip; include/celerite2_amd_shapes.h has the rule; P = 0 is a single event, P > 0 folds).  What the shape
    search under correlated noise reads (celerite2_amd/shapes.py).  Every trial is evaluated as written and none can read
    outside the bank (the index is clamped); the domain is the caller's to mask.  Caller-owned `out` is accepted (nothing
    is allocated then: capturable in a HIP graph); it must not alias an input.  J <= 32 and 1 <= Q0 <= 8.  No atomics: two
    calls give identical bits."""
    return _whitened("whitened_shapes", "shape", t, c, U, W, d, Z0, trials, out, shapes=shapes)


def trial_projections(kind, t, alpha, trials, *, t_ref=0.0, out=None):
    """P (B, K, C, R): P[b, k, c, r] = sum_n col_c(trial k; t[b, n]) alpha[b, n, r] for alpha (B, N, R), t (N,) shared by the
    batch or (B, N), and the trials of `kind`: "periodogram" (ANGULAR frequencies (K,) | (B, K); columns cos, sin of
    w (t - t_ref); C = 2), "transit" ((K, 4) | (B, K, 4) = (P, t0, w, tau); the template; C = 1) or "keplerian" ((K, 3) |
    (B, K, 3) = (w, e, tp); columns cos nu, sin nu; C = 2).  The columns are formed in registers, bit for bit the ones
    `whitened_sinusoids` / `whitened_transits` / `whitened_keplerians` whiten, and contracted with alpha on the matrix cores
    (c2_trial_projections, csrc/c2_trial_project.hip): with alpha = (K + D)^-1 (y_r - mean), P is the one entry of those ops'
    T that depends on y, for R series y_r at once.  What gp.search_significance reads.  Caller-owned `out` is accepted
    (nothing is allocated then: capturable in a HIP graph); it must not alias an input.  No atomics: two calls give
    identical bits."""
    if kind not in TRIAL_KINDS:
        raise ValueError("kind must be one of %s" % (tuple(TRIAL_KINDS),))
    return _projections("trial_projections", kind, t, alpha, trials, out, t_ref=t_ref)


def shape_projections(t, alpha, trials, shapes, *, out=None):
    """P (B, K, 1, R): P[b, k, 0, r] = sum_n b_k(t[b, n]) alpha[b, n, r] for alpha (B, N, R), t (N,) shared by the batch or
    (B, N), the trials (K, 4) | (B, K, 4) = (P, t0, w, s) and the bank `shapes` (NS, S) | (B, NS, S) of `whitened_shapes`:
    `trial_projections` for the tabulated shape, in the layout significance.null_statistics takes for a one-column kind.
    The column is formed in registers, bit for bit the one `whitened_shapes` whitens, and contracted with alpha on the
    matrix cores (c2_shape_projections, csrc/c2_trial_project.hip).  What gp.shape_search_significance reads.  Caller-owned
    `out` is accepted (nothing is allocated then: capturable in a HIP graph); it must not alias an input.  No atomics: two
    calls give identical bits."""
    return _projections("shape_projections", "shape", t, alpha, trials, out, shapes=shapes)


_KRON_METHODS = {"collapsed": 0, "interleaved": 1}


def _no_alias(outs, ins):
    """No output may share its first byte with an input or another output ("<name> must not alias <name>"); entries are
    (name, tensor, ...)."""
    seen = [(e[0], e[1].data_ptr()) for e in ins if e[1] is not None and e[1].numel()]
    for nm, x, *_ in outs:
        if x is None or not x.numel():
            continue
        for other, ptr in seen:
            if x.data_ptr() == ptr:
                raise ValueError("Invalid argument: %s must not alias %s" % (nm, other))
        seen.append((nm, x.data_ptr()))


def inverse_diag(t, c, U, W, d, z=None, q=None, alpha=None, *, workspace=False, ws=None):
    """q (B, N), the diagonal of the inverse of the factored matrix K + D = L diag(d) L^T, in one backward sweep over
    d, W (c2_inverse_diag).  With z (B, N) -- solve_lower of a residual -- the same pass also returns
    alpha = L^-T (z / d) = (K + D)^-1 (y - mean): (q, alpha); `alpha` may be `z` itself (the only aliasing allowed).  Caller-owned outputs `q`,
    `alpha` are accepted (nothing is allocated then: capturable in a HIP graph).

    `workspace=True` (c2_inverse_diag_fwd): the same q and alpha, bit for bit, and the states inverse_diag_rev reads --
    returns (q, ws) or (q, alpha, ws) with ws = (Mws (B, N, J, J), Fws (B, N, J) | None without z): 8 B N J (J + 1) bytes,
    2.4 MB per series at N = 4096, J = 8; callers with large batches chunk the batch.  Caller-owned `ws` is accepted.
    J <= 32, and no output may alias an input or another output (alpha == z included)."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    q = torch.empty_like(d) if q is None else q
    if z is None:
        if alpha is not None:
            raise ValueError("Invalid shape: alpha (given without z)")
    elif alpha is None:
        alpha = torch.empty_like(z)
    ins = [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("d", d, "BN"), ("z", z, "BN")]
    outs = [("q", q, "BN"), ("alpha", alpha, "BN")]
    _args(dims, ins + outs)
    if workspace or ws is not None:
        if ws is None:
            ws = _empty(U.device, dims, "BNJJ") + (_empty(U.device, dims, "BNJ") if z is not None else (None,))
        Mws, Fws = ws
        if (Fws is None) != (z is None):
            raise ValueError("Invalid shape: Fws (given exactly when z is)")
        states = [("Mws", Mws, "BNJJ"), ("Fws", Fws, "BNJ")]
        _args(dims, states)
        _no_alias(outs + states, ins)
        rc = _lib.load().c2_inverse_diag_fwd(B, N, J, t, _bs(t, N), c, _bs(c, J), U, W, d, z, q, alpha, Mws, Fws, _stream())
        _lib.check(rc, "inverse_diag")
        return (q, (Mws, Fws)) if z is None else (q, alpha, (Mws, Fws))
    # the only aliasing the sweep allows is alpha == z (a row's z is read before its alpha is stored)
    if q.data_ptr() == d.data_ptr():
        raise ValueError("Invalid argument: q must not alias d")
    if z is not None and q.data_ptr() in (z.data_ptr(), alpha.data_ptr()):
        raise ValueError("Invalid argument: q must not alias z or alpha")
    if alpha is not None and alpha.data_ptr() == d.data_ptr():
        raise ValueError("Invalid argument: alpha must not alias d")
    rc = _lib.load().c2_inverse_diag(B, N, J, t, _bs(t, N), c, _bs(c, J), U, W, d, z, q, alpha, _stream())
    _lib.check(rc, "inverse_diag")
    return q if z is None else (q, alpha)


def inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, balpha, *, out=None):
    """The reverse of inverse_diag (c2_inverse_diag_rev): cotangents bq (B, N) of q and balpha (B, N) of alpha ->
    (bt (B, N), bc (B, J), bU, bW (B, N, J), bd (B, N), bz (B, N)), per series also when t or c is shared (the caller
    sums).  q, alpha, ws: what inverse_diag(..., workspace=True) returned for the same inputs -- ws holds
    8 B N J (J + 1) bytes, 2.4 MB per series at N = 4096, J = 8.  z, alpha, balpha and ws[1] are None together (bz is then
    None).  `out`: the six tensors of a previous call to write into (nothing is allocated then: capturable).  J <= 32; no
    output may alias an input or another output.  No atomics: two calls give identical bits."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    Mws, Fws = ws
    grads = dict(bt="BN", bc="BJ", bU="BNJ", bW="BNJ", bd="BN", **({} if z is None else dict(bz="BN")))
    if out is None:
        out = _empty(U.device, dims, *grads.values()) + ((None,) if z is None else ())
    bt, bc, bU, bW, bd, bz = out
    hz = z is not None
    for nm, v in (("alpha", alpha), ("Fws", Fws), ("balpha", balpha), ("bz", bz)):
        if (v is not None) != hz:
            raise ValueError("Invalid shape: %s (given exactly when z is)" % nm)
    _args(dims, [("t", t, _T), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("d", d, "BN"), ("z", z, "BN"), ("q", q, "BN"),
                 ("alpha", alpha, "BN"), ("Mws", Mws, "BNJJ"), ("Fws", Fws, "BNJ"), ("bq", bq, "BN"), ("balpha", balpha, "BN")],
          _named(grads, out))
    rc = _lib.load().c2_inverse_diag_rev(B, N, J, t, _bs(t, N), c, _bs(c, J), U, W, d, z, q, alpha, Mws, Fws, bq, balpha, bt, bc,
                                         bU, bW, bd, bz, _stream())
    _lib.check(rc, "inverse_diag_rev")
    return bt, bc, bU, bW, bd, bz


def get_celerite_matrices_rev(ac, bc, dc, x, V, bt, bcv, ba, bU, bV, Jr, *, work=None):
    """The reverse of get_celerite_matrices (c2_get_celerite_matrices_rev): cotangents bt (B, N), bcv (B, J), ba (B, N),
    bU, bV (B, N, J) of (t, c, a, U, V), J = Jr + 2 Jc, and the V the forward call returned ->
    (bar, bcr (B, Jr), bac, bbc, bcc, bdc (B, Jc), bx (B, N), bdiag (B, N)), per series also for shared coefficients.
    ac, bc, dc (Jc,) | (B, Jc); x (N,) | (B, N).  No output aliases an input; fixed summation order."""
    B, N, J = _dims(V)
    Jc = ac.shape[-1]
    if Jr + 2 * Jc != J:
        raise ValueError("Invalid shape: V (got width %d, expected Jr + 2 Jc = %d)" % (J, Jr + 2 * Jc))
    dims = dict(B=B, N=N, J=J, R=Jr, C=Jc)
    batched = ac.dim() == 2
    coef = "BC" if batched else "C"
    _args(dims, [("x", x, _T), ("ac", ac, coef), ("bc", bc, coef), ("dc", dc, coef), ("V", V, "BNJ"), ("bt", bt, "BN"),
                 ("bc", bcv, "BJ"), ("ba", ba, "BN"), ("bU", bU, "BNJ"), ("bV", bV, "BNJ")])
    outs = _empty(V.device, dims, *_COEFS, "BN", "BN")
    lib = _lib.load()
    nbytes = lib.c2_get_celerite_matrices_rev_workspace_bytes(B, N, Jr, Jc)
    if nbytes and (work is None or work.numel() * 8 < nbytes):
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=V.device)
    rc = lib.c2_get_celerite_matrices_rev(
        B, N, Jr, Jc, ac if Jc else None, bc if Jc else None, dc if Jc else None, batched, x, _bs(x, N), V, bt, bcv, ba, bU, bV,
        *_coef_ptrs(*outs[:6], Jr, Jc), *outs[6:], work, 0 if work is None else work.numel() * 8, _stream())
    _lib.check(rc, "get_celerite_matrices_rev")
    return outs


def _general_rev(name):
    def op(t1, t2, c, U, V, Y, F, bZ, *, out=None):
        dims = _general_dims(U, V, Y)
        B, N, M, J, nrhs = dims.values()
        grads = dict(bt1="BN", bt2="BM", bc="BJ", bU="BNJ", bV="BMJ", bY="BMK")
        if out is None:
            out = _empty(U.device, dims, *grads.values())
        bt1, bt2, bc, bU, bV, bY = out
        _args(dims, [("t1", t1, _T), ("t2", t2, "M|BM"), ("c", c, _C), ("U", U, "BNJ"), ("V", V, "BMJ"), ("Y", Y, "BMK"),
                     ("F", F, "BMJK"), ("bZ", bZ, "BNK")], _named(grads, out))
        rc = getattr(_lib.load(), "c2_" + name)(B, N, M, J, nrhs, t1, _bs(t1, N), t2, _bs(t2, M), c, _bs(c, J), U, V, Y, F, bZ,
                                                bt1, bt2, bc, bU, bV, bY, _stream())
        _lib.check(rc, name)
        return bt1, bt2, bc, bU, bV, bY
    op.__name__ = name
    op.__doc__ = (
        "The reverse of %s (c2_%s, csrc/c2_general_rev.hip): the cotangent bZ (B, N, nrhs) of the product ->\n"
        "(bt1 (B, N), bt2 (B, M), bc (B, J), bU (B, N, J), bV (B, M, J), bY (B, M, nrhs)), per series also when t1, t2 or c is\n"
        "shared (the caller sums); every element is overwritten.  F (B, M, J, nrhs): the workspace the forward call wrote for\n"
        "the same arguments (`workspace=True`); it is read, never re-derived, and only at rows the forward absorbed.  `out`:\n"
        "the six tensors of a previous call to write into (nothing is allocated then: capturable).  One sweep over the merge\n"
        "of the two grids per right-hand side, O((N + M) J) each.  J <= 32; no output may alias an input or another output.\n"
        "No atomics: two calls give identical bits." % (name[:-4], name))
    return op


general_matmul_lower_rev = _general_rev("general_matmul_lower_rev")
general_matmul_upper_rev = _general_rev("general_matmul_upper_rev")


def _merged_dims(U, Us):
    B, N, J = _dims(U)
    if Us.dim() != 3:
        raise ValueError("Invalid shape: Us (must be (B, M, J))")
    return dict(B=B, N=N, M=Us.shape[1], J=J)


def _explained_variance_in(t, ts, c, U, W, d, Us, Vs):
    return [("t", t, _T), ("ts", ts, "M|BM"), ("c", c, _C), ("U", U, "BNJ"), ("W", W, "BNJ"), ("d", d, "BN"), ("Us", Us, "BMJ"),
            ("Vs", Vs, "BMJ")]


def explained_variance(t, ts, c, U, W, d, Us, Vs, *, out=None, work=None, workspace=False, ws=None):
    """r (B, M) = diag(K*^T (K + D)^-1 K*) at the M sorted query times `ts` ((M,) shared or (B, M)) against the factored
    matrix K + D = L diag(d) L^T on the data times `t`: the predictive variance at `ts` is k(0) - r.  Two sweeps over the
    merge of the two grids (c2_explained_variance), O((N + M) J^2) per series, no N x M array.  Us, Vs (B, M, J): the
    kernel's U and V rows at the queries.  Caller-owned `out` (B, M) and `work` (B, M, J) are accepted (nothing is
    allocated then: capturable in a HIP graph); neither may alias an input or the other.  J <= 32.

    `workspace=True` (c2_explained_variance_fwd): the same r and work, bit for bit, and the states explained_variance_rev
    reads -- returns (r, ws) with ws = (Sws, Rws), both (B, N, J, J), the forward and the backward state after every data
    row: 16 B N J^2 bytes, 4.2 MB per series at N = 4096, J = 8; callers with large batches chunk the batch.  A caller-owned
    `ws` is accepted.  The reverse also reads `work`: pass it in to keep it."""
    dims = _merged_dims(U, Us)
    B, N, M, J = dims.values()
    dev = U.device
    out = _empty(dev, dims, "BM")[0] if out is None else out
    with_ws = workspace or ws is not None
    if ws is not None:
        Sws, Rws = ws
    elif with_ws:
        Sws, Rws = _empty(dev, dims, "BNJJ", "BNJJ")
    else:
        Sws = Rws = None
    work = _empty(dev, dims, "BMJ")[0] if work is None else work
    ins = _explained_variance_in(t, ts, c, U, W, d, Us, Vs)
    outs = [("out", out, "BM"), ("work", work, "BMJ"), ("Sws", Sws, "BNJJ"), ("Rws", Rws, "BNJJ")]
    _args(dims, ins + outs)
    if with_ws:
        _no_alias(outs, ins)
        rc = _lib.load().c2_explained_variance_fwd(B, N, M, J, t, _bs(t, N), ts, _bs(ts, M), c, _bs(c, J), U, W, d, Us, Vs, out,
                                                   work, Sws, Rws, _stream())
        _lib.check(rc, "explained_variance")
        return out, (Sws, Rws)
    inputs = [x.data_ptr() for x in (t, ts, c, U, W, d, Us, Vs)]
    if out.data_ptr() in inputs or out.data_ptr() == work.data_ptr():
        raise ValueError("Invalid argument: out must not alias an input or work")
    if work.data_ptr() in inputs:
        raise ValueError("Invalid argument: work must not alias an input")
    rc = _lib.load().c2_explained_variance(B, N, M, J, t, _bs(t, N), ts, _bs(ts, M), c, _bs(c, J), U, W, d, Us, Vs, out, work,
                                           _stream())
    _lib.check(rc, "explained_variance")
    return out


def explained_variance_rev(t, ts, c, U, W, d, Us, Vs, work, ws, br, *, out=None):
    """The reverse of explained_variance (c2_explained_variance_rev, csrc/c2_predvar_rev.hip): the cotangent br (B, M) of r ->
    (bt (B, N), bts (B, M), bc (B, J), bU, bW (B, N, J), bd (B, N), bUs, bVs (B, M, J)), per series also when t, ts or c is
    shared (the caller sums); every element is overwritten.  work (B, M, J) and ws = (Sws, Rws) (B, N, J, J): what
    explained_variance(..., work=work, workspace=True) wrote and returned for the same inputs --
    16 B N J^2 bytes, 4.2 MB per series at N = 4096, J = 8; the states are read, never re-derived.  `out`: the eight tensors
    of a previous call to write into (nothing is allocated then: capturable).  Two sweeps over the merge of the two grids,
    O((N + M) J^2) per series.  J <= 32; no output may alias an input or another output.  No atomics: two calls give
    identical bits."""
    dims = _merged_dims(U, Us)
    B, N, M, J = dims.values()
    Sws, Rws = ws
    grads = dict(bt="BN", bts="BM", bc="BJ", bU="BNJ", bW="BNJ", bd="BN", bUs="BMJ", bVs="BMJ")
    if out is None:
        out = _empty(U.device, dims, *grads.values())
    bt, bts, bc, bU, bW, bd, bUs, bVs = out
    _args(dims, _explained_variance_in(t, ts, c, U, W, d, Us, Vs) + [("work", work, "BMJ"), ("Sws", Sws, "BNJJ"),
                                                                     ("Rws", Rws, "BNJJ"), ("br", br, "BM")],
          _named(grads, out))
    rc = _lib.load().c2_explained_variance_rev(B, N, M, J, t, _bs(t, N), ts, _bs(ts, M), c, _bs(c, J), U, W, d, Us, Vs, work, Sws,
                                               Rws, br, bt, bts, bc, bU, bW, bd, bUs, bVs, _stream())
    _lib.check(rc, "explained_variance_rev")
    return bt, bts, bc, bU, bW, bd, bUs, bVs


def prior_draw(t, ts, c, U, V, Us, Vs, nt, ns, *, ft=None, fs=None):
    """(ft (B, N, K), fs (B, M, K)): K joint draws of the NOISE-FREE prior process at the sorted data times `t` ((N,)
    shared or (B, N)) and the sorted query times `ts` ((M,) or (B, M)) -- the Cholesky factor of the zero-noise kernel
    matrix on the merged grid applied to the standard normals nt (B, N, K), ns (B, M, K), in one forward sweep
    (c2_prior_draw), O((N + M) (J^2 + J K)) per series, nothing stored per row.  U, V (B, N, J) and Us, Vs (B, M, J): the
    kernel's rows on the two grids.  A point that coincides with an earlier one takes that point's value and consumes no
    normal.  Caller-owned `ft`, `fs` are accepted (nothing is allocated then: capturable in a HIP graph); `ft` may be `nt`
    and `fs` may be `ns` (a row's normals are read before its draw is stored), any other aliasing is refused.  J <= 32."""
    dims = _merged_dims(U, Us)
    if nt.dim() != 3:
        raise ValueError("Invalid shape: nt (must be (B, N, K))")
    dims["K"] = nt.shape[2]
    B, N, M, J, K = dims.values()
    ft = _empty(U.device, dims, "BNK")[0] if ft is None else ft
    fs = _empty(U.device, dims, "BMK")[0] if fs is None else fs
    _args(dims, [("t", t, _T), ("ts", ts, "M|BM"), ("c", c, _C), ("U", U, "BNJ"), ("V", V, "BNJ"), ("Us", Us, "BMJ"),
                 ("Vs", Vs, "BMJ"), ("nt", nt, "BNK"), ("ns", ns, "BMK"), ("ft", ft, "BNK"), ("fs", fs, "BMK")])
    # the only aliasing the sweep allows is ft == nt and fs == ns
    inputs = {name: x.data_ptr() for name, x in (("t", t), ("ts", ts), ("c", c), ("U", U), ("V", V), ("Us", Us), ("Vs", Vs),
                                                   ("nt", nt), ("ns", ns))}
    if ft.data_ptr() in [p for name, p in inputs.items() if name != "nt"] or ft.data_ptr() == fs.data_ptr():
        raise ValueError("Invalid argument: ft must not alias an input other than nt, or fs")
    if fs.data_ptr() in [p for name, p in inputs.items() if name != "ns"]:
        raise ValueError("Invalid argument: fs must not alias an input other than ns")
    rc = _lib.load().c2_prior_draw(B, N, M, J, K, t, _bs(t, N), ts, _bs(ts, M), c, _bs(c, J), U, V, Us, Vs, nt, ns, ft, fs,
                                   _stream())
    _lib.check(rc, "prior_draw")
    return ft, fs


def _kron_args(t, c, a, U, V, alpha, diag, y, method):
    B, N, J = _dims(U)
    if diag.dim() != 3:
        raise ValueError("Invalid shape: diag (must be (B, N, M))")
    M = diag.shape[-1]
    if method not in _KRON_METHODS:
        raise ValueError("method must be 'collapsed' or 'interleaved'")
    dims = dict(B=B, N=N, M=M, J=J)
    _args(dims, [("t", t, _T), ("c", c, _C), ("a", a, "BN"), ("U", U, "BNJ"), ("V", V, "BNJ"), ("alpha", alpha, "M|BM"),
                 ("diag", diag, "BNM"), ("y", y, "BNM")])
    return dims, _KRON_METHODS[method]


def kron_loglik(t, c, a, U, V, alpha, diag, y, *, method="collapsed", work=None):
    """2-D (multi-band) log-likelihood, rank-1 band covariance K = T (x) alpha alpha^T + diag (extension; the
    reference has no 2-D code).  (t, c, a, U, V): celerite matrices of the EPOCH grid built with zero white noise
    (a = k(0)); alpha (M,)|(B,M); diag, y (B,N,M).  Returns (ll (B,), flag (B,) int32)."""
    dims, meth = _kron_args(t, c, a, U, V, alpha, diag, y, method)
    B, N, M, J = dims.values()
    lib = _lib.load()
    nbytes = lib.c2_kron_loglik_workspace_bytes(B, N, M, J, meth, 0)
    if work is None or work.numel() * 8 < nbytes:
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=U.device)
    ll, = _empty(U.device, dims, "B")
    flag = _flag(B, U.device)
    rc = lib.c2_kron_loglik(B, N, M, J, t, _bs(t, N), c, _bs(c, J), a, U, V, alpha, _bs(alpha, M), diag, y, ll, flag, meth, work,
                            work.numel() * 8, _stream())
    _lib.check(rc, "kron_loglik")
    return ll, flag


def kron_loglik_grad(t, c, a, U, V, alpha, diag, y, *, method="collapsed", work=None):
    """kron_loglik + reverse-mode gradient.  Returns (ll, (bt, bc, ba, bU, bV, balpha, bdiag, by), flag); balpha is
    per series (B, M) also for a shared alpha.  (ba, bU, bV) are the partials of the method's own parametrisation
    ("collapsed": T_nn = a_n, the literal Kronecker definition; "interleaved": same-epoch cross-band terms through
    U_n.V_n); the total derivatives bU + ba V, bV + ba U along a = U.V agree."""
    dims, meth = _kron_args(t, c, a, U, V, alpha, diag, y, method)
    B, N, M, J = dims.values()
    lib = _lib.load()
    dev = U.device
    nbytes = lib.c2_kron_loglik_workspace_bytes(B, N, M, J, meth, 1)
    if work is None or work.numel() * 8 < nbytes:
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    ll, bt, bc, ba, bU, bV, balpha, bdiag, by = _empty(dev, dims, "B", "BN", "BJ", "BN", "BNJ", "BNJ", "BM", "BNM", "BNM")
    flag = _flag(B, dev)
    rc = lib.c2_kron_loglik_grad(B, N, M, J, t, _bs(t, N), c, _bs(c, J), a, U, V, alpha, _bs(alpha, M), diag, y, ll, bt, bc, ba,
                                 bU, bV, balpha, bdiag, by, flag, meth, work, work.numel() * 8, _stream())
    _lib.check(rc, "kron_loglik_grad")
    return ll, (bt, bc, ba, bU, bV, balpha, bdiag, by), flag


def _terms_args(ar, cr, ac, bc, cc, dc, x, diag, y):
    if diag.dim() != 2:
        raise ValueError("Invalid shape: diag (must be (B, N))")
    B, N = diag.shape
    Jr, Jc = ar.shape[-1], ac.shape[-1]
    batched = any(v.dim() == 2 for v in (ar, cr, ac, bc, cc, dc))
    if batched and not all(v.dim() == 2 for v in (ar, cr, ac, bc, cc, dc)):
        raise ValueError("coefficients must be all shared or all per-series")
    _chk(ar, cr, ac, bc, cc, dc, x, diag, y)
    _shape("x", x, (N,), (B, N)); _shape("y", y, (B, N))
    for nm, v, w in (("ar", ar, Jr), ("cr", cr, Jr), ("ac", ac, Jc), ("bc", bc, Jc), ("cc", cc, Jc), ("dc", dc, Jc)):
        _shape(nm, v, (w,), (B, w))
    return B, N, Jr, Jc, batched


def _coef_ptrs(ar, cr, ac, bc, cc, dc, Jr, Jc):
    """The six coefficient arrays as arguments: a zero-width one is passed as NULL."""
    return [ar if Jr else None, cr if Jr else None, ac if Jc else None, bc if Jc else None, cc if Jc else None,
            dc if Jc else None]


def loglik_terms(ar, cr, ac, bc, cc, dc, x, diag, y, *, work=None):
    """Batched log-likelihood straight from the celerite coefficients (terms.py:117-177 + numpy.py:84-109).
    ar, cr (Jr,)|(B,Jr); ac, bc, cc, dc (Jc,)|(B,Jc); x (N,)|(B,N); diag, y (B,N).  Returns (ll, flag)."""
    B, N, Jr, Jc, batched = _terms_args(ar, cr, ac, bc, cc, dc, x, diag, y)
    lib = _lib.load()
    nbytes = lib.c2_loglik_terms_workspace_bytes(B, N, Jr, Jc, 0)
    if work is None or work.numel() * 8 < nbytes:
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=diag.device)
    ll = torch.empty(B, dtype=torch.float64, device=diag.device)
    flag = _flag(B, diag.device)
    rc = lib.c2_loglik_terms(B, N, Jr, Jc, *_coef_ptrs(ar, cr, ac, bc, cc, dc, Jr, Jc), batched, x, _bs(x, N), diag, y, ll, flag,
                             work, work.numel() * 8, _stream())
    _lib.check(rc, "loglik_terms")
    return ll, flag


def loglik_terms_workspace(B, N, Jr, Jc, device, grad=True):
    """Scratch for loglik_terms[_grad] (reusable across calls of the same shape)."""
    lib = _lib.load()
    return torch.empty(lib.c2_loglik_terms_workspace_bytes(B, N, Jr, Jc, 1 if grad else 0) // 8, dtype=torch.float64,
                       device=device)


def loglik_terms_grad(ar, cr, ac, bc, cc, dc, x, diag, y, *, work=None, out=None):
    """loglik_terms + reverse-mode gradient w.r.t. every input: returns
    (ll, (bar, bcr, bac, bbc, bcc, bdc, bx, bdiag, by), flag); coefficient gradients are per series (B, Jr|Jc) also when
    the coefficients are shared by the batch.  `out`: a previous call's nine gradient tensors to write into."""
    B, N, Jr, Jc, batched = _terms_args(ar, cr, ac, bc, cc, dc, x, diag, y)
    lib = _lib.load()
    dev = diag.device
    dims = dict(B=B, N=N, R=Jr, C=Jc)
    nbytes = lib.c2_loglik_terms_workspace_bytes(B, N, Jr, Jc, 1)
    if work is None or work.numel() * 8 < nbytes:
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    spec = _COEFS + ("BN", "BN", "BN")
    if out is not None:
        outs = list(out)
        if len(outs) != 9 or any(tuple(o.shape) != _forms(dims, s)[0] or o.dtype != torch.float64 or o.device != dev
                                 or not o.is_contiguous() for o, s in zip(outs, spec)):
            raise ValueError("Invalid shape: out (nine contiguous float64 tensors as returned by loglik_terms_grad)")
    else:
        outs = list(_empty(dev, dims, *spec))
    ll, = _empty(dev, dims, "B")
    flag = _flag(B, dev)
    rc = lib.c2_loglik_terms_grad(B, N, Jr, Jc, *_coef_ptrs(ar, cr, ac, bc, cc, dc, Jr, Jc), batched, x, _bs(x, N), diag, y, ll,
                                  *_coef_ptrs(*outs[:6], Jr, Jc), *outs[6:], flag, work, work.numel() * 8, _stream())
    _lib.check(rc, "loglik_terms_grad")
    return ll, tuple(outs), flag


def _loglik_grad_composite(t, c, a, U, V, y):
    """Internal cross-check: the literal op chain (factor_fwd -> solve_lower_fwd -> seeds -> solve_lower_rev ->
    factor_rev) with S/F workspaces materialised in HBM, as the reference's autodiff frontends run it."""
    B, N, J = _dims(U)
    dims = dict(B=B, N=N, J=J)
    dev = U.device
    lib = _lib.load()
    # (not in the public header: declared here, next to their only user)
    lib.c2_loglik_grad_composite_workspace_bytes.restype = ctypes.c_size_t
    lib.c2_loglik_grad_composite_workspace_bytes.argtypes = [ctypes.c_int64] * 3
    lib.c2_loglik_grad_composite.argtypes = lib.c2_loglik_grad.argtypes
    work = torch.empty(lib.c2_loglik_grad_composite_workspace_bytes(B, N, J) // 8, dtype=torch.float64, device=dev)
    out = _empty(dev, dims, *_LOGLIK_GRADS.values())
    bt, bc, ba, bU, bV, by = out
    ll, = _empty(dev, dims, "B")
    flag = _flag(B, dev)
    rc = lib.c2_loglik_grad_composite(B, N, J, t, _bs(t, N), c, _bs(c, J), a, U, V, y, ll, bt, bc, ba, bU, bV, by, flag, work,
                                      work.numel() * 8, _stream())
    _lib.check(rc, "loglik_grad_composite")
    return ll, out, flag


# ---- term hyper-parameters on the device (csrc/c2_term_params.hip) --------------------------------------------------------
class _TermRec(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("par", ctypes.c_int32), ("regime", ctypes.c_int32), ("jr", ctypes.c_int32),
                ("jc", ctypes.c_int32), ("col", ctypes.c_int32 * 5), ("eps", ctypes.c_double)]


class _TermProgram(ctypes.Structure):
    _fields_ = [("nterms", ctypes.c_int32), ("np", ctypes.c_int32), ("Jr", ctypes.c_int32), ("Jc", ctypes.c_int32),
                ("term", _TermRec * 16)]


_KINDS = {"real": (0, 2, 1, 0), "complex": (1, 4, 0, 1), "sho": (2, 3, None, None), "matern32": (3, 2, 0, 1),
          "rotation": (4, 5, 0, 2)}   # name -> (C2_TERM_*, parameters, real slots, complex slots)
_REGIMES = {"under": (0, 0, 1), "over": (1, 2, 0), "mixed": (2, 2, 1)}   # name -> (C2_SHO_*, real slots, complex slots)
SHO_SIGMA, SHO_RHO, SHO_TAU = 1, 2, 4


def _fill_program(records, NP):
    """records -> (copies with jr / jc / eps / par filled in, NP, the c2_term_program)."""
    if not 1 <= len(records) <= 16:
        raise ValueError("a term program holds 1 .. 16 terms (got %d)" % len(records))
    records = [dict(r) for r in records]
    NP = int(NP)
    c = _TermProgram()
    jr = jc = 0
    for i, r in enumerate(records):
        if r["kind"] not in _KINDS:
            raise ValueError("unknown term kind %r" % (r["kind"],))
        kind, npar, wr, wc = _KINDS[r["kind"]]
        regime = 0
        if r["kind"] == "sho":
            if r.get("regime") not in _REGIMES:
                raise ValueError("SHO regime must be 'under', 'over' or 'mixed'")
            regime, wr, wc = _REGIMES[r["regime"]]
        cols = [int(k) for k in r["cols"]]
        if len(cols) != npar or any(not 0 <= k < NP for k in cols):
            raise ValueError("term %d (%s): needs %d parameter columns in [0, %d)" % (i, r["kind"], npar, NP))
        t = c.term[i]
        t.kind, t.par, t.regime, t.jr, t.jc = kind, int(r.get("par") or 0), regime, jr, jc
        for k, v in enumerate(cols):
            t.col[k] = v
        eps = r.get("eps")
        t.eps = float((0.01 if r["kind"] == "matern32" else 1e-5) if eps is None else eps)
        r.update(jr=jr, jc=jc, eps=t.eps, par=t.par)
        jr += wr
        jc += wc
    c.nterms, c.np, c.Jr, c.Jc = len(records), NP, jr, jc
    return records, NP, c


def record_widths(record):
    """(real slots, complex slots) of one leaf record."""
    if record["kind"] == "sho":
        return _REGIMES[record["regime"]][1:]
    return _KINDS[record["kind"]][2:]


class TermProgram:
    """The flattened sum of terms the kernels walk (c2_term_program, celerite2_amd.h): built ONCE from a list of records
    `dict(kind=, cols=, par=0, regime=None, eps=)` and passed to the kernels by value.  `kind` is "real" (cols a, c),
    "complex" (a, b, c, d), "sho" (S0|sigma, w0|rho, Q|tau; `par` = OR of SHO_SIGMA / SHO_RHO / SHO_TAU; `regime` "under" |
    "over" | "mixed"), "matern32" (sigma, rho) or "rotation" (sigma, period, Q0, dQ, f); `cols` index the parameter matrix
    P (B, NP) | (NP,).  Coefficient slots follow program order, reals and complex terms each concatenated
    (TermSum.get_coefficients).  Jr + 2 Jc <= 32."""

    def __init__(self, records, NP):
        self.records, self.NP, self._c = _fill_program(records, NP)
        self.Jr, self.Jc = self._c.Jr, self._c.Jc
        if self.Jr + 2 * self.Jc > 32:
            raise ValueError("term program: width %d not supported (the coefficient-level entry points take J <= 32)" % (self.Jr + 2 * self.Jc))

    @property
    def width(self):
        return self.Jr + 2 * self.Jc


class _TermRange(ctypes.Structure):
    _fields_ = [("r0", ctypes.c_int32), ("nr", ctypes.c_int32), ("c0", ctypes.c_int32), ("nc", ctypes.c_int32)]


class _TermOp(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("col", ctypes.c_int32), ("a", _TermRange), ("b", _TermRange), ("out", _TermRange)]


class _TermExpr(ctypes.Structure):
    _fields_ = [("leaves", _TermProgram), ("nops", ctypes.c_int32), ("NR", ctypes.c_int32), ("NC", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("op", _TermOp * 16)]


_OPS = {"sum": 0, "product": 1, "diff": 2, "convolve": 3}


class TermExpr:
    """Term ALGEBRA the kernels walk (c2_term_expr, celerite2_amd.h): the leaf records of a TermProgram (`records`, same
    dicts, but their total width is not limited to 32) followed by `operations` in post-order, each
    `dict(op="sum" | "product" | "diff" | "convolve", a=, b=, col=)`.  An operand is an int i (the result of operation i) or a
    4-tuple (r0, nr, c0, nc) of leaf registers: real registers [r0, r0 + nr) and complex registers [c0, c0 + nc), numbered
    as the leaves' jr / jc.  "diff" and "convolve" take `a` only; "convolve" must be the last operation and `col` names the
    column of P that holds the boxcar width delta.  Results get fresh registers in order (filled in as `out`); the result
    of the last operation is the kernel: Jr, Jc, width <= 32."""

    def __init__(self, records, operations, NP):
        self.records, self.NP, leaves = _fill_program(records, NP)
        if not 1 <= len(operations) <= 16:
            raise ValueError("a term expression holds 1 .. 16 operations (got %d)" % len(operations))
        c = _TermExpr()
        c.leaves = leaves
        nr, nc = leaves.Jr, leaves.Jc
        self.operations = []
        for i, o in enumerate(operations):
            o = dict(o)
            if o["op"] not in _OPS:
                raise ValueError("unknown operation %r" % (o["op"],))
            binary = o["op"] in ("sum", "product")
            rng = []
            for key in ("a", "b") if binary else ("a",):
                v = o[key]
                if isinstance(v, int):
                    if not 0 <= v < i:
                        raise ValueError("operation %d: operand %r is not an earlier operation" % (i, v))
                    v = self.operations[v]["out"]
                v = tuple(int(k) for k in v)
                if len(v) != 4 or min(v) < 0 or v[0] + v[1] > nr or v[2] + v[3] > nc:
                    raise ValueError("operation %d: operand range %r outside the registers written so far" % (i, v))
                rng.append(v)
            a = rng[0]
            b = rng[1] if binary else (0, 0, 0, 0)
            if o["op"] == "sum":
                wr, wc = a[1] + b[1], a[3] + b[3]
            elif o["op"] == "product":
                wr, wc = a[1] * b[1], a[1] * b[3] + b[1] * a[3] + 2 * a[3] * b[3]
            else:
                wr, wc = a[1], a[3]
            col = -1
            if o["op"] == "convolve":
                col = int(o["col"])
                if i != len(operations) - 1 or not 0 <= col < self.NP:
                    raise ValueError("a convolution is the last operation and reads a column of P")
            out = (nr, wr, nc, wc)
            if wr + 2 * wc > 32 or nr + wr > 256 or nc + wc > 256:
                raise ValueError("term expression: width %d not supported (the coefficient-level entry points take J <= 32)" % (wr + 2 * wc))
            t = c.op[i]
            t.op, t.col = _OPS[o["op"]], col
            for dst, src in ((t.a, a), (t.b, b), (t.out, out)):
                dst.r0, dst.nr, dst.c0, dst.nc = src
            nr, nc = nr + wr, nc + wc
            self.operations.append(dict(op=o["op"], a=a, b=b, out=out, col=col))
        c.nops, c.NR, c.NC = len(operations), nr, nc
        self.Jr, self.Jc = self.operations[-1]["out"][1], self.operations[-1]["out"][3]
        self.has_shift = self.operations[-1]["op"] == "convolve"
        self._c = c

    @property
    def width(self):
        return self.Jr + 2 * self.Jc

    def workspace(self, B, device):
        """The register buffer of term_coefficients[_rev] for B series (values + cotangents)."""
        nbytes = _lib.load().c2_term_expr_workspace_bytes(ctypes.byref(self._c), B)
        return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)


def _program_P(program, P):
    if P.dim() not in (1, 2):
        raise ValueError("Invalid shape: P (must be (NP,) or (B, NP))")
    _chk(P)
    if P.shape[-1] != program.NP:
        raise ValueError("Invalid shape: P (got %s, expected (%d,) or (B, %d))" % (tuple(P.shape), program.NP, program.NP))


def term_coefficients(program, P, B=None, *, out=None, flag=None, shift=None, work=None):
    """P (B, NP) | shared (NP,) (then `B` says how many series) -> ((ar, cr, ac, bc, cc, dc), flag): the coefficients in the
    layout loglik_terms takes, (B, Jr) / (B, Jc), and flag (B,) int32 (nonzero: an SHO series on the wrong side of its regime).
    For a TermExpr (products, derivatives, the exposure-time convolution) a third value is returned, `shift` (B,): what the
    convolution adds to the diagonal (0 without one); `work` = program.workspace(B, device), reusable."""
    _program_P(program, P)
    B = P.shape[0] if P.dim() == 2 else B
    if B is None:
        raise ValueError("term_coefficients: a shared P needs the batch size B")
    _shape("P", P, (program.NP,), (B, program.NP))
    dev = P.device
    Jr, Jc = program.Jr, program.Jc
    dims = dict(B=B, R=Jr, C=Jc)
    if out is None:
        out = list(_empty(dev, dims, *_COEFS))
    else:
        _args(dims, zip(("ar", "cr", "ac", "bc", "cc", "dc"), out, _COEFS))
    flag = _flag(B, dev) if flag is None else flag
    if isinstance(program, TermExpr):
        shift = _empty(dev, dims, "B")[0] if shift is None else shift
        work = program.workspace(B, dev) if work is None else work
        _chk(shift, work)
        _shape("shift", shift, (B,))
        rc = _lib.load().c2_term_expr_coefficients(ctypes.byref(program._c), B, P, _bs(P, program.NP), *_coef_ptrs(*out, Jr, Jc),
                                                   shift, flag, work, work.numel() * 8, _stream())
        _lib.check(rc, "term_expr_coefficients")
        return tuple(out), flag, shift
    rc = _lib.load().c2_term_coefficients(ctypes.byref(program._c), B, P, _bs(P, program.NP), *_coef_ptrs(*out, Jr, Jc), flag,
                                          _stream())
    _lib.check(rc, "term_coefficients")
    return tuple(out), flag


def term_coefficients_rev(program, P, cotangents, *, B=None, tflag=None, lflag=None, ll=None, out=None, bshift=None, work=None):
    """The reverse of term_coefficients: cotangents (bar, bcr, bac, bbc, bcc, bdc), (B, Jr) / (B, Jc), -> bP (B, NP), per series
    also for a shared P.  `tflag` (term_coefficients' flag), `lflag` (loglik_terms_grad's flag) and `ll`, when given, are
    settled on the device: a wrong-regime series gets a zero row, ll = -inf and lflag = -2; a failed factorisation a zero row.
    For a TermExpr: `bshift` (B,), the cotangent of the diagonal shift (None = 0), and `work` as in term_coefficients."""
    _program_P(program, P)
    Jr, Jc = program.Jr, program.Jc
    cot = list(cotangents)
    if len(cot) != 6:
        raise ValueError("Invalid shape: cotangents (six tensors)")
    B = cot[0].shape[0] if Jr else cot[2].shape[0]
    _shape("P", P, (program.NP,), (B, program.NP))
    dims = dict(B=B, R=Jr, C=Jc, P=program.NP)
    _args(dims, zip(("bar", "bcr", "bac", "bbc", "bcc", "bdc"), cot, _COEFS))
    bP = _empty(P.device, dims, "BP")[0] if out is None else out
    _chk(bP)
    _shape("bP", bP, (B, program.NP))
    for nm, f in (("tflag", tflag), ("lflag", lflag)):
        if f is not None and (f.dtype != torch.int32 or tuple(f.shape) != (B,) or not f.is_contiguous()):
            raise ValueError("Invalid shape: %s (must be (B,) int32)" % nm)
    _shape("ll", ll, (B,))
    if isinstance(program, TermExpr):
        work = program.workspace(B, P.device) if work is None else work
        _chk(bshift, work)
        _shape("bshift", bshift, (B,))
        rc = _lib.load().c2_term_expr_coefficients_rev(ctypes.byref(program._c), B, P, _bs(P, program.NP),
                                                       *_coef_ptrs(*cot, Jr, Jc), bshift, tflag, lflag, ll, bP, work,
                                                       work.numel() * 8, _stream())
        _lib.check(rc, "term_expr_coefficients_rev")
        return bP
    rc = _lib.load().c2_term_coefficients_rev(ctypes.byref(program._c), B, P, _bs(P, program.NP),
                                              *_coef_ptrs(*cot, Jr, Jc), tflag, lflag, ll, bP, _stream())
    _lib.check(rc, "term_coefficients_rev")
    return bP


def noise_mean_apply(yerr, jitter, mean, y, *, yerr_is_sigma=True, out=None):
    """diag = yerr^2 + jitter^2 (`yerr_is_sigma=False`: yerr is already a variance, diag = yerr + jitter^2) and r = y - mean in
    one pass.  yerr, y (B, N); jitter, mean (B,) or None (= 0).  Returns (diag, r); `out` = two (B, N) tensors to write into."""
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B, N = y.shape
    diag, r = (torch.empty_like(y), torch.empty_like(y)) if out is None else out
    _args(dict(B=B, N=N), [("yerr", yerr, "BN"), ("jitter", jitter, "B"), ("mean", mean, "B"), ("y", y, "BN"), ("diag", diag, "BN"),
                           ("r", r, "BN")])
    rc = _lib.load().c2_noise_mean_apply(B, N, yerr, bool(yerr_is_sigma), jitter, mean, y, diag, r, _stream())
    _lib.check(rc, "noise_mean_apply")
    return diag, r


def noise_mean_rev(jitter, bdiag, by, *, flag=None, out=None):
    """bjitter = 2 jitter sum_n bdiag, bmean = -sum_n by, (B,) each, in one pass over bdiag and by (B, N) with a fixed
    summation order (two runs give identical bits).  jitter (B,) or None (bjitter = 0); a series with flag != 0 gets zeros."""
    if by.dim() != 2:
        raise ValueError("Invalid shape: by (must be (B, N))")
    B, N = by.shape
    dims = dict(B=B, N=N)
    bj, bm = _empty(by.device, dims, "B", "B") if out is None else out
    _args(dims, [("jitter", jitter, "B"), ("bdiag", bdiag, "BN"), ("by", by, "BN"), ("bjitter", bj, "B"), ("bmean", bm, "B")])
    if flag is not None and (flag.dtype != torch.int32 or tuple(flag.shape) != (B,)):
        raise ValueError("Invalid shape: flag (must be (B,) int32)")
    rc = _lib.load().c2_noise_mean_rev(B, N, jitter, bdiag, by, flag, bj, bm, _stream())
    _lib.check(rc, "noise_mean_rev")
    return bj, bm


def noise_mean_shift_apply(yerr, jitter, mean, shift, y, *, yerr_is_sigma=True, out=None):
    """noise_mean_apply with one more per-series term: diag = yerr^2 (or yerr) + jitter^2 + shift[b] -- the (negative) diagonal
    shift of an exposure-time convolution (term_coefficients of a TermExpr).  shift (B,) or None (then noise_mean_apply's bits)."""
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B, N = y.shape
    diag, r = (torch.empty_like(y), torch.empty_like(y)) if out is None else out
    _args(dict(B=B, N=N), [("yerr", yerr, "BN"), ("jitter", jitter, "B"), ("mean", mean, "B"), ("shift", shift, "B"), ("y", y, "BN"),
                           ("diag", diag, "BN"), ("r", r, "BN")])
    rc = _lib.load().c2_noise_mean_shift_apply(B, N, yerr, bool(yerr_is_sigma), jitter, mean, shift, y, diag, r, _stream())
    _lib.check(rc, "noise_mean_shift_apply")
    return diag, r


def noise_mean_shift_rev(jitter, bdiag, by, *, flag=None, tflag=None, out=None):
    """noise_mean_rev plus bshift = sum_n bdiag, the cotangent of noise_mean_shift_apply's shift: (bjitter, bmean, bshift), (B,)
    each, one pass, the same fixed summation order.  A series with flag != 0 or tflag != 0 gets zeros."""
    if by.dim() != 2:
        raise ValueError("Invalid shape: by (must be (B, N))")
    B, N = by.shape
    dims = dict(B=B, N=N)
    bj, bm, bs = _empty(by.device, dims, "B", "B", "B") if out is None else out
    _args(dims, [("jitter", jitter, "B"), ("bdiag", bdiag, "BN"), ("by", by, "BN"), ("bjitter", bj, "B"), ("bmean", bm, "B"),
                 ("bshift", bs, "B")])
    for f in (flag, tflag):
        if f is not None and (f.dtype != torch.int32 or tuple(f.shape) != (B,)):
            raise ValueError("Invalid shape: flag (must be (B,) int32)")
    rc = _lib.load().c2_noise_mean_shift_rev(B, N, jitter, bdiag, by, flag, tflag, bj, bm, bs, _stream())
    _lib.check(rc, "noise_mean_shift_rev")
    return bj, bm, bs


def loglik_kernel_workspace(program, B, N, device):
    """Caller-owned buffers of loglik_kernel_grad, reusable across calls of the same shape (and required for graph capture):
    a dict with the scratch of loglik_terms_grad, the six coefficient arrays and their cotangents, diag, r and the term flag;
    for a TermExpr also the diagonal shift, its cotangent and the register buffer of the coefficient kernels."""
    Jr, Jc = program.Jr, program.Jc
    dims = dict(B=B, N=N, R=Jr, C=Jc)
    diag, r = _empty(device, dims, "BN", "BN")
    work = {"terms": loglik_terms_workspace(B, N, Jr, Jc, device), "coefs": list(_empty(device, dims, *_COEFS)),
            "cots": list(_empty(device, dims, *_COEFS)), "diag": diag, "r": r, "tflag": _flag(B, device)}
    if isinstance(program, TermExpr):
        shift, bshift = _empty(device, dims, "B", "B")
        work.update(shift=shift, bshift=bshift, expr=program.workspace(B, device))
    return work


def loglik_kernel_grad(program, P, x, yerr, jitter, mean, y, *, yerr_is_sigma=True, work=None, out=None):
    """Hyper-parameters to log-likelihood and gradient in one stream-ordered chain, no host traffic (graph-capturable with
    caller-owned `work` = loglik_kernel_workspace(...) and `out` = a previous call's six gradient tensors):
    noise_mean_apply -> term_coefficients -> loglik_terms_grad -> term_coefficients_rev / noise_mean_rev.
    With a TermExpr the coefficient stage comes first, because diag needs its shift:
    term_coefficients -> noise_mean_shift_apply -> loglik_terms_grad -> noise_mean_shift_rev -> term_coefficients_rev.
    P (B, NP) | (NP,); x (N,) | (B, N); yerr, y (B, N); jitter, mean (B,) or None.
    Returns (ll, (bP, bjitter, bmean, bx, bdiag, by), flag): bP (B, NP), bjitter, bmean (B,) per series; bdiag is the
    cotangent of diag = yerr^2 + jitter^2 (byerr = 2 yerr bdiag is the caller's).  flag: 0, the first failing row of the
    factorisation, or -2 for an SHO series on the wrong side of its regime; a flagged series has ll = -inf and ZERO bP,
    bjitter, bmean (its rows of bx, bdiag, by are what loglik_terms_grad left there)."""
    if y.dim() != 2:
        raise ValueError("Invalid shape: y (must be (B, N))")
    B, N = y.shape
    dev = y.device
    if work is None:
        work = loglik_kernel_workspace(program, B, N, dev)
    if out is None:
        out = _empty(dev, dict(B=B, N=N, P=program.NP), "BP", "B", "B", "BN", "BN", "BN")
    bP, bj, bm, bx, bdiag, by = out
    if isinstance(program, TermExpr):
        coefs, tflag, shift = term_coefficients(program, P, B, out=work["coefs"], flag=work["tflag"], shift=work["shift"],
                                                work=work["expr"])
        diag, r = noise_mean_shift_apply(yerr, jitter, mean, shift, y, yerr_is_sigma=yerr_is_sigma, out=(work["diag"], work["r"]))
        ll, _, flag = loglik_terms_grad(*coefs, x, diag, r, work=work["terms"], out=tuple(work["cots"]) + (bx, bdiag, by))
        noise_mean_shift_rev(jitter, bdiag, by, flag=flag, tflag=tflag, out=(bj, bm, work["bshift"]))
        term_coefficients_rev(program, P, work["cots"], tflag=tflag, lflag=flag, ll=ll, out=bP, bshift=work["bshift"],
                              work=work["expr"])
        return ll, (bP, bj, bm, bx, bdiag, by), flag
    diag, r = noise_mean_apply(yerr, jitter, mean, y, yerr_is_sigma=yerr_is_sigma, out=(work["diag"], work["r"]))
    coefs, tflag = term_coefficients(program, P, B, out=work["coefs"], flag=work["tflag"])
    ll, _, flag = loglik_terms_grad(*coefs, x, diag, r, work=work["terms"], out=tuple(work["cots"]) + (bx, bdiag, by))
    term_coefficients_rev(program, P, work["cots"], tflag=tflag, lflag=flag, ll=ll, out=bP)
    noise_mean_rev(jitter, bdiag, by, flag=flag, out=(bj, bm))
    return ll, (bP, bj, bm, bx, bdiag, by), flag


# ---- streaming updates (include/celerite2_amd_filter.h, csrc/c2_filter.hip; _lib.HEADERS["filter"]) ------------------------
_FILTER_ROWS = dict(t="M|BM", c=_C)   # the new rows' times and the rates; everything else of a row is per series


def filter_state_words(J):
    """Doubles per series of a filter state, 4 + J + J^2 (t_last, n, sum log d, sum z^2 / d, F, S); 0 beyond J = 32."""
    return int(_lib.load().c2_filter_state_words(int(J)))


def filter_init(B, J, device):
    """The empty state of B series of width J: zeros (B, SW), n = 0."""
    SW = filter_state_words(J)
    if SW == 0:
        raise ValueError("celerite2_amd.filter_init: width not supported (1 <= J <= %d)" % _lib.C2_FAST_WIDTH)
    return torch.zeros((int(B), SW), dtype=torch.float64, device=device)


def _filter_dims(X, name):
    if X.dim() != 3:
        raise ValueError("Invalid shape: %s (must be (B, M, J))" % name)
    B, M, J = X.shape
    return dict(B=B, M=M, J=J, S=4 + J + J * J)


def _filter_count(count, dims, dev):
    if count is None:
        return
    if not (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.device == dev):
        raise ValueError("celerite2_amd filter ops need `count` as a contiguous int32 tensor on the same device")
    if tuple(count.shape) != (dims["B"],):
        raise ValueError("Invalid shape: count (got %s, expected %s)" % (tuple(count.shape), (dims["B"],)))


def _filter_out(state, out):
    """The output state: `state` itself (in place), or a tensor of its own."""
    if out is None:
        return torch.empty_like(state)
    if out is not state and out.data_ptr() == state.data_ptr():
        raise ValueError("Invalid argument: out must be state itself or must not overlap it")
    return out


def filter_append(state, t, c, a, U, V, y, *, count=None, out=None, d=None, W=None, z=None):
    """Append up to M rows per series to a filter state in O(M J^2) (c2_filter_append): t (M,) | (B, M), c (J,) | (B, J),
    a, y (B, M), U, V (B, M, J) -> (state, d, W, z, flag) with the d, W, z rows that `factor` and `solve_lower` of the whole
    series would give -- d the one-step-ahead predictive variance, z the innovation.  `count` (B,) int32: rows m >= count[b]
    are not read and their outputs are not written; a series with count 0 keeps its state bit for bit.  flag (B,) int32:
    the 1-based row of this call whose d <= 0 (the rows before it are written, the series' state stays as on entry), else 0.
    `out` may be `state` (in place); caller-owned `d`, `W`, `z` are accepted and must not alias an input.  J <= 32.
    The times must be sorted and not before the state's t_last: not checked here (celerite2_amd.stream.Filter does)."""
    dims = _filter_dims(U, "U")
    B, M, J = dims["B"], dims["M"], dims["J"]
    out = _filter_out(state, out)
    d = torch.empty_like(a) if d is None else d
    W = torch.empty_like(V) if W is None else W
    z = torch.empty_like(y) if z is None else z
    ins = [("state", state, "BS"), ("out", out, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("a", a, "BM"), ("U", U, "BMJ"),
           ("V", V, "BMJ"), ("y", y, "BM")]
    _args(dims, ins, [("d", d, "BM"), ("W", W, "BMJ"), ("z", z, "BM")])
    _filter_count(count, dims, U.device)
    flag = _flag(B, U.device)
    rc = _lib.load().c2_filter_append(B, M, J, state, out, t, _bs(t, M), c, _bs(c, J), a, U, V, y, count, d, W, z, flag, _stream())
    _lib.check(rc, "filter_append")
    return out, d, W, z, flag


def filter_absorb(state, t, c, W, d, z, *, count=None, out=None):
    """Absorb rows of an existing factorisation -- W (B, M, J), d (B, M) of `factor`, z (B, M) of `solve_lower` -- into a
    filter state without refactoring (c2_filter_absorb): only the decay and the update of the state are applied.  Returns the
    new state; `out` may be `state`; `count` as in filter_append."""
    dims = _filter_dims(W, "W")
    B, M, J = dims["B"], dims["M"], dims["J"]
    out = _filter_out(state, out)
    _args(dims, [("state", state, "BS"), ("out", out, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("W", W, "BMJ"),
                 ("d", d, "BM"), ("z", z, "BM")])
    _filter_count(count, dims, W.device)
    rc = _lib.load().c2_filter_absorb(B, M, J, state, out, t, _bs(t, M), c, _bs(c, J), W, d, z, count, _stream())
    _lib.check(rc, "filter_absorb")
    return out


def filter_forecast(state, t, c, a, U, *, count=None, mu=None, var=None):
    """(mu, var) (B, M) at M query rows per series, each independently from the same unchanged state (c2_filter_forecast):
    mu = u^T (p o F), var = a - u^T ((p p^T) o S) u, p = exp(-c (t - t_last)).  For t >= t_last this is the full conditional
    given all absorbed rows (earlier times are not checked and give no conditional).  Rows m >= count[b] are not read and
    not written."""
    dims = _filter_dims(U, "U")
    B, M, J = dims["B"], dims["M"], dims["J"]
    mu = torch.empty_like(a) if mu is None else mu
    var = torch.empty_like(a) if var is None else var
    _args(dims, [("state", state, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("a", a, "BM"), ("U", U, "BMJ")],
          [("mu", mu, "BM"), ("var", var, "BM")])
    _filter_count(count, dims, U.device)
    rc = _lib.load().c2_filter_forecast(B, M, J, state, t, _bs(t, M), c, _bs(c, J), a, U, count, mu, var, _stream())
    _lib.check(rc, "filter_forecast")
    return mu, var


# ---- reverse of the append (include/celerite2_amd_filter_rev.h, csrc/c2_filter_rev.hip; _lib.HEADERS["filter_rev"]) --------
_FILTER_REV_OUT = dict(bstate_in="BS", bt="BM", bc="BJ", ba="BM", bU="BMJ", bV="BMJ", by="BM")   # bt, bc: per series always


def filter_rev_workspace_words(J):
    """Doubles of scratch per row of filter_append_rev, J + J^2 (the F and S the row starts from); 0 beyond J = 32."""
    return int(_lib.load().c2_filter_rev_workspace_words(int(J)))


def filter_append_rev(state, t, c, U, W, d, z, flag, bstate, bd=None, bW=None, bz=None, *, count=None, ws=None, out=None):
    """Reverse of filter_append (c2_filter_append_rev): `state` (B, SW) the state the forward call STARTED from, t, c, U,
    count as given to it, W, d, z, flag as it returned them; cotangents bstate (B, SW) of the state it left and bd, bz (B, M),
    bW (B, M, J) of its rows (None = 0) -> (bstate_in (B, SW), bt (B, M), bc (B, J), ba (B, M), bU, bV (B, M, J), by (B, M)).
    bt and bc come out PER SERIES also when t or c are shared.  The S block of a state cotangent is the symmetric
    representative: the incoming one is replaced by (B + B^T) / 2.  Word [0] of bstate is added to bt of the last taken row;
    rows m >= count[b] get zeros; a series with count 0 or flag != 0 gets bstate_in = bstate and zeros.  `ws`
    (B, M, J + J^2): scratch of this call (allocated when None); `out`: the seven outputs, caller-owned (they may be
    uninitialised, and must not alias an input).  J <= 32."""
    dims = _filter_dims(U, "U")
    B, M, J = dims["B"], dims["M"], dims["J"]
    dims["X"] = J + J * J
    ws = _empty(U.device, dims, "BMX")[0] if ws is None else ws
    out = _empty(U.device, dims, *_FILTER_REV_OUT.values()) if out is None else tuple(out)
    if len(out) != len(_FILTER_REV_OUT):
        raise ValueError("Invalid argument: out must be (bstate_in, bt, bc, ba, bU, bV, by)")
    ins = [("state", state, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("U", U, "BMJ"), ("W", W, "BMJ"), ("d", d, "BM"),
           ("z", z, "BM"), ("bstate", bstate, "BS"), ("bd", bd, "BM"), ("bW", bW, "BMJ"), ("bz", bz, "BM")]
    _args(dims, ins, [("ws", ws, "BMX")] + _named(_FILTER_REV_OUT, out))
    _filter_count(count, dims, U.device)
    _filter_count(flag, dims, U.device)
    rc = _lib.load().c2_filter_append_rev(B, M, J, state, t, _bs(t, M), c, _bs(c, J), U, W, d, z, count, flag, bstate, bd, bW, bz,
                                          ws, *out, _stream())
    _lib.check(rc, "filter_append_rev")
    return out


# ---- reverse of forecast and absorb (include/celerite2_amd_filter_stream_rev.h, csrc/c2_filter_stream_rev.hip;
# _lib.HEADERS["filter_stream_rev"]) ----------------------------------------------------------------------------------------
_FILTER_FORECAST_REV_OUT = dict(bstate="BS", bt="BM", bc="BJ", ba="BM", bU="BMJ")                       # bt, bc: per series always
_FILTER_ABSORB_REV_OUT = dict(bstate_in="BS", bt="BM", bc="BJ", bW="BMJ", bd="BM", bz="BM")


def filter_forecast_rev(state, t, c, U, bmu, bvar, *, count=None, out=None):
    """Reverse of filter_forecast (c2_filter_forecast_rev): state, t, c, U, count as given to it, cotangents bmu, bvar (B, M)
    -> (bstate (B, SW), bt (B, M), bc (B, J), ba (B, M), bU (B, M, J)).  The forecast reads the state and leaves it, so
    bstate is a cotangent to ADD to whatever else the state feeds: word [0] = -sum_m bt_m, words [1..3] zero, the S block
    symmetric to the bit.  bt and bc come out PER SERIES also when t or c are shared.  Rows m >= count[b] get zeros, a series
    with count 0 or an empty state (n == 0) zeros everywhere but ba = bvar in the rows it took.  `out`: the five outputs,
    caller-owned (they may be uninitialised, and must not alias an input).  J <= 32."""
    dims = _filter_dims(U, "U")
    B, M, J = dims["B"], dims["M"], dims["J"]
    out = _empty(U.device, dims, *_FILTER_FORECAST_REV_OUT.values()) if out is None else tuple(out)
    if len(out) != len(_FILTER_FORECAST_REV_OUT):
        raise ValueError("Invalid argument: out must be (bstate, bt, bc, ba, bU)")
    ins = [("state", state, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("U", U, "BMJ"), ("bmu", bmu, "BM"),
           ("bvar", bvar, "BM")]
    _args(dims, ins, _named(_FILTER_FORECAST_REV_OUT, out))
    _filter_count(count, dims, U.device)
    rc = _lib.load().c2_filter_forecast_rev(B, M, J, state, t, _bs(t, M), c, _bs(c, J), U, count, bmu, bvar, *out, _stream())
    _lib.check(rc, "filter_forecast_rev")
    return out


def filter_absorb_rev(state, t, c, W, d, z, bstate, *, count=None, ws=None, out=None):
    """Reverse of filter_absorb (c2_filter_absorb_rev): `state` (B, SW) the state the forward call STARTED from, t, c, W, d,
    z, count as given to it, bstate (B, SW) the cotangent of the state it left -> (bstate_in (B, SW), bt (B, M), bc (B, J),
    bW (B, M, J), bd (B, M), bz (B, M)).  The conventions of filter_append_rev: the S block of a state cotangent is the
    symmetric representative (the incoming one is replaced by (B + B^T) / 2), word [0] of bstate is added to bt of the last
    taken row, words [1..3] pass through, bt and bc come out PER SERIES; rows m >= count[b] get zeros, a series with count 0
    gets bstate_in = bstate and zeros.  `ws` (B, M, J + J^2), filter_rev_workspace_words(J) doubles per row: scratch of this
    call (allocated when None); `out`: the six outputs, caller-owned.  J <= 32."""
    dims = _filter_dims(W, "W")
    B, M, J = dims["B"], dims["M"], dims["J"]
    dims["X"] = J + J * J
    ws = _empty(W.device, dims, "BMX")[0] if ws is None else ws
    out = _empty(W.device, dims, *_FILTER_ABSORB_REV_OUT.values()) if out is None else tuple(out)
    if len(out) != len(_FILTER_ABSORB_REV_OUT):
        raise ValueError("Invalid argument: out must be (bstate_in, bt, bc, bW, bd, bz)")
    ins = [("state", state, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("W", W, "BMJ"), ("d", d, "BM"), ("z", z, "BM"),
           ("bstate", bstate, "BS")]
    _args(dims, ins, [("ws", ws, "BMX")] + _named(_FILTER_ABSORB_REV_OUT, out))
    _filter_count(count, dims, W.device)
    rc = _lib.load().c2_filter_absorb_rev(B, M, J, state, t, _bs(t, M), c, _bs(c, J), W, d, z, count, bstate, ws, *out, _stream())
    _lib.check(rc, "filter_absorb_rev")
    return out


# ---- forecast sample paths (include/celerite2_amd_filter_draw.h, csrc/c2_filter_draw.hip; _lib.HEADERS["filter_draw"]) -----
def filter_draw_chunk(J):
    """Draws one pass of the draw kernel carries at width J (further draws go to further blocks, each repeating the O(J^2)
    part of a row); 0 beyond J = 32."""
    return int(_lib.load().c2_filter_draw_chunk(int(J)))


def filter_draw(state, t, c, a, U, V, eps, *, count=None, paths=None, d=None):
    """K joint draws at M query rows per series from a filter state, in O(M (J^2 + J K)) (c2_filter_draw): state (B, SW),
    t (M,) | (B, M), c (J,) | (B, J), a (B, M), U, V (B, M, J) the celerite matrices of the query rows, eps (B, M, K) standard
    normals, draw-fastest -> (paths (B, M, K), d (B, M), flag (B,) int32).  Row by row, the append run backwards in y:
    z_k = sqrt(d) eps_k, y_k = u^T F_k + z_k, F_k <- F_k + w z_k, with the S, d and w of the append shared by the draws -- so
    paths = mu_c + chol(Sigma_c) eps for the dense conditional mean and covariance of the M rows given every absorbed row,
    and d, flag have filter_append's bits.  a = k(0) + diag: draws of would-be observations; a = k(0): of the latent process.
    The state is read and not written.  `count` (B,) int32: rows m >= count[b] are neither read nor written.  flag: the
    1-based row with d <= 0 (the rows before it are written, the failing row's d, nothing behind it), else 0.  Caller-owned
    `paths`, `d` are accepted and must not alias an input.  J <= 32.  The times must be sorted and not before the state's
    t_last: not checked here (celerite2_amd.stream.Filter.sample_forecast does)."""
    dims = _filter_dims(U, "U")
    B, M, J = dims["B"], dims["M"], dims["J"]
    if eps.dim() != 3:
        raise ValueError("Invalid shape: eps (must be (B, M, K))")
    dims["K"] = K = eps.shape[2]
    paths = torch.empty_like(eps) if paths is None else paths
    d = torch.empty_like(a) if d is None else d
    ins = [("state", state, "BS"), ("t", t, _FILTER_ROWS["t"]), ("c", c, _C), ("a", a, "BM"), ("U", U, "BMJ"), ("V", V, "BMJ"),
           ("eps", eps, "BMK")]
    _args(dims, ins, [("paths", paths, "BMK"), ("d", d, "BM")])
    _filter_count(count, dims, U.device)
    flag = _flag(B, U.device)
    rc = _lib.load().c2_filter_draw(B, M, J, K, state, t, _bs(t, M), c, _bs(c, J), a, U, V, eps, count, paths, d, flag, _stream())
    _lib.check(rc, "filter_draw")
    return paths, d, flag
