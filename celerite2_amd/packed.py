# -*- coding: utf-8 -*-
"""Ragged batches: the exact log-likelihood, and its gradient, of B series of DIFFERENT lengths stored as catalogues store
them -- row-packed with offsets -- in memory that grows like rows x J (csrc/c2_packed.hip).

    pk = Packed.from_list([t_0, t_1, ...])                   # or Packed(t, lengths), t (R,) with R = sum(lengths)
    ll, flag = loglik(pk, c, a, U, V, y)                      # a, y (R,), U, V (R, J), c (J,) | (B, J)
    ll, (bt, bc, ba, bU, bV, by), flag = loglik_grad(pk, c, a, U, V, y)
    ll = log_likelihood(pk, c, a, U, V, y)                    # differentiable (torch.autograd)
    ll = log_likelihood_kernel(kernel, pk, y, yerr=yerr)      # ... in the hyper-parameters of a terms.* kernel

A PROVISIONAL interface: the three C entry points are declared in csrc/c2_packed_api.h, not under include/, and this module
binds them itself -- from that header, with the parser and the type table of _lib, typed exactly as _lib.load() types the
public ones.  Nothing here is in ops.__all__ or _lib.HEADERS (INTEGRATION.md says what promotion takes).

As everywhere in this package there is no fallback: without the library or a device the ops raise.  `Packed` and
`celerite_rows` are plain torch and also take CPU tensors.
"""
import ctypes
import math
import os
import re

import numpy as np
import torch

from . import _lib, ops

__all__ = ["Packed", "loglik", "loglik_grad", "workspace", "checkpoint_interval", "log_likelihood", "celerite_rows",
           "log_likelihood_kernel"]

HEADER = os.path.join(_lib._HERE, "csrc", "c2_packed_api.h")
# the C symbols the header declares, in its order (hand-written: the pin the header is compared against, as _lib.HEADERS)
SYMBOLS = ["c2_packed_loglik_grad_workspace_bytes", "c2_packed_loglik", "c2_packed_loglik_grad"]

_fns = None


def header_text():
    """csrc/c2_packed_api.h without its comments."""
    if not os.path.exists(HEADER):
        raise _lib.BackendError("celerite2_amd: %s not found -- celerite2_amd.packed takes its prototypes from it" % HEADER)
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def _load():
    """name -> typed function of the provisional header, bound on the library _lib.load() loaded."""
    global _fns
    if _fns is None:
        lib = _lib.load()
        protos = _lib._prototypes(header_text())
        if list(protos) != SYMBOLS:
            raise _lib.BackendError("celerite2_amd.packed: %s declares %s, expected %s" % (HEADER, list(protos), SYMBOLS))
        _fns = {name: ctypes.CFUNCTYPE(restype, *argtypes)((name, lib), ((1,),) * len(argtypes))
                for name, (restype, argtypes) in protos.items()}
    return _fns


def checkpoint_interval(n_max):
    """C = max(1, ceil(sqrt(n_max))): the rows between two checkpoints of the gradient call (c2_packed_api.h)."""
    n_max = int(n_max)
    return 1 if n_max <= 1 else math.isqrt(n_max - 1) + 1


class Packed:
    """The row layout of a ragged batch: series b owns rows offsets[b] .. offsets[b+1]-1 of every (R, ...) array.

    Fields: t (R,) float64; lengths (host, numpy int64 (B,)); offsets (B+1,) int64 on t's device; n_max; order (B,) int32 on
    the device, the series by descending length (stable: ties keep their order); seg (R,) int64, the series of each row
    (built on first use); B, R."""

    def __init__(self, t, lengths, *, check_sorted=True):
        if not torch.is_tensor(t) or t.dtype != torch.float64:
            raise ValueError("Packed: t must be a float64 tensor")
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("Packed: t must be a contiguous (R,) tensor")
        if torch.is_tensor(lengths):
            lengths = lengths.detach().cpu().numpy()
        lengths = np.asarray(lengths)
        if lengths.ndim != 1 or lengths.size < 1 or lengths.dtype.kind not in "iu":
            raise ValueError("Packed: lengths must be a (B,) array of integers, B >= 1")
        lengths = lengths.astype(np.int64)
        if (lengths < 0).any():
            raise ValueError("Packed: negative length")
        if int(lengths.sum()) != t.shape[0]:
            raise ValueError("Packed: sum(lengths) = %d, but t has %d rows" % (int(lengths.sum()), t.shape[0]))
        self.t, self.lengths = t, lengths
        self.B, self.R = int(lengths.size), int(t.shape[0])
        self.n_max = int(lengths.max())
        off = np.zeros(self.B + 1, dtype=np.int64)
        np.cumsum(lengths, out=off[1:])
        self._off = off
        self.offsets = torch.from_numpy(off).to(t.device)
        self.order = torch.from_numpy(np.argsort(-lengths, kind="stable").astype(np.int32)).to(t.device)
        self._seg = self._pos = None
        if check_sorted and self.R > 1:
            inner = torch.ones(self.R - 1, dtype=torch.bool, device=t.device)   # row pairs inside one series
            cut = off[1:-1]
            cut = cut[(cut > 0) & (cut < self.R)]
            if cut.size:
                inner[torch.from_numpy(cut - 1).to(t.device)] = False
            td = t.detach()
            if bool(((td[1:] < td[:-1]) & inner).any()):
                raise ValueError("Packed: times decrease within a series")

    @classmethod
    def from_list(cls, ts, *, check_sorted=True):
        ts = list(ts)
        if not ts:
            raise ValueError("Packed.from_list: no series")
        for x in ts:
            if not torch.is_tensor(x) or x.dim() != 1:
                raise ValueError("Packed.from_list: every series must be a (N_b,) tensor")
        return cls(torch.cat(ts).contiguous(), [int(x.shape[0]) for x in ts], check_sorted=check_sorted)

    @property
    def seg(self):
        if self._seg is None:
            dev = self.t.device
            self._seg = torch.repeat_interleave(torch.arange(self.B, device=dev), torch.from_numpy(self.lengths).to(dev),
                                                output_size=self.R)
        return self._seg

    @property
    def pos(self):
        """(R,) int64: the row's index within its series."""
        if self._pos is None:
            self._pos = torch.arange(self.R, device=self.t.device) - self.offsets[self.seg]
        return self._pos

    def _rows(self, x, name):
        if x.shape[:1] != (self.R,):
            raise ValueError("Invalid shape: %s (got %s, expected (%d, ...))" % (name, tuple(x.shape), self.R))

    def unpack(self, x):
        """The B views x[offsets[b] : offsets[b+1]] of an (R, ...) array."""
        self._rows(x, "x")
        return [x[self._off[b]:self._off[b + 1]] for b in range(self.B)]

    def to_padded(self, x, fill=0.0):
        """(R, ...) -> (B, n_max, ...), `fill` behind the rows of a series."""
        self._rows(x, "x")
        out = torch.full((self.B, self.n_max) + tuple(x.shape[1:]), fill, dtype=x.dtype, device=x.device)
        out[self.seg, self.pos] = x
        return out

    def from_padded(self, X):
        """(B, n_max, ...) -> (R, ...): the rows of every series, the padding dropped."""
        if tuple(X.shape[:2]) != (self.B, self.n_max):
            raise ValueError("Invalid shape: X (got %s, expected (%d, %d, ...))" % (tuple(X.shape), self.B, self.n_max))
        return X[self.seg, self.pos]


_IN = (("c", "J|BJ"), ("a", "R"), ("U", "RJ"), ("V", "RJ"), ("y", "R"))
_GRADS = (("bt", "R"), ("bc", "BJ"), ("ba", "R"), ("bU", "RJ"), ("bV", "RJ"), ("by", "R"))
_SORTED, _AUTO = "sorted", "auto"


def _prepare(pk, c, a, U, V, y, outs=()):
    """The checks of one op, before any pointer reaches a kernel: dtype, device, contiguity and shapes."""
    if not isinstance(pk, Packed):
        raise TypeError("celerite2_amd.packed: pk must be a Packed")
    if U.dim() != 2:
        raise ValueError("Invalid shape: U (must be (R, J))")
    dims = dict(B=pk.B, R=pk.R, J=U.shape[1])
    entries = [("t", pk.t, "R")] + [(n, x, s) for (n, s), x in zip(_IN, (c, a, U, V, y))] + list(outs)
    ops._chk(*(x for _, x, _ in entries))
    if pk.offsets.device != U.device:
        raise ValueError("celerite2_amd ops need every tensor on the same device")
    ops._shapes(dims, entries)
    return dims


def _order(pk, order, J):
    if order is None:
        return None
    if isinstance(order, str):
        if order == _AUTO:
            return _auto_order(pk, J)
        if order != _SORTED:
            raise ValueError("order: 'auto', 'sorted', None or a (B,) int32 permutation")
        return pk.order
    if not (torch.is_tensor(order) and order.dtype == torch.int32 and tuple(order.shape) == (pk.B,) and order.is_contiguous()
            and order.device == pk.offsets.device):
        raise ValueError("order: 'auto', 'sorted', None or a contiguous (B,) int32 permutation on the device")
    return order


_cus = {}


def _auto_order(pk, J):
    """The order the ops take by default: pk.order where the grid has more wavefronts than the device holds at once, else
    none.  Series of similar length in one wavefront save its idle trips, and that pays once wavefronts queue for a place:
    the call then lasts as long as all of them together.  While every wavefront is resident at once the call lasts as long as
    its longest wavefront, which no order shortens -- and, measured, wavefronts full of long series run slower than mixed ones
    (profiles/packed.md: 8192 ragged series, J = 2, 13.2 ms sorted against 8.5 ms as stored; the rule is drawn from the four
    ragged shapes there).  A wavefront holds 64 / G series; 16 per compute unit stands for what is resident."""
    if int(pk.lengths.min()) == pk.n_max:
        return None
    dev = pk.offsets.device
    if dev not in _cus:
        _cus[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    G = 1
    while G < J:
        G *= 2
    return pk.order if (pk.B * G + 63) // 64 > 16 * _cus[dev] else None


def _nz(x):
    """An empty tensor has no address (R == 0: every series empty); the kernels then touch no row of what stands in."""
    return x if x is None or x.numel() else x.new_empty(1)


def workspace(pk, J):
    """The `work` of loglik_grad for this layout at width J (float64, uninitialised: nothing depends on what it holds)."""
    nbytes = _load()["c2_packed_loglik_grad_workspace_bytes"](pk.B, pk.R, pk.n_max, int(J))
    if nbytes == 0:
        raise ValueError("celerite2_amd.packed.workspace: width not supported (1 <= J <= %d)" % _lib.C2_FAST_WIDTH)
    return torch.empty(nbytes // 8, dtype=torch.float64, device=pk.offsets.device)


def loglik(pk, c, a, U, V, y, *, factor=False, order=_AUTO):
    """The log-likelihood of every series -> (ll (B,), flag (B,) int32); with factor=True also d (R,), W (R, J), z (R,): the
    packed factor + solve_lower.  flag[b] is the 1-based row within the series of the first d <= 0 (ll = -inf), or 0.
    `order`: which series share a wavefront -- 'auto' (pk.order on grids larger than the device, else as stored), 'sorted'
    (pk.order), None (as stored) or a (B,) int32 permutation; no result depends on it by a bit."""
    dims = _prepare(pk, c, a, U, V, y)
    dev = U.device
    ll = torch.empty(pk.B, dtype=torch.float64, device=dev)
    flag = torch.empty(pk.B, dtype=torch.int32, device=dev)
    d = W = z = None
    if factor:
        d, W, z = torch.empty_like(a), torch.empty_like(U), torch.empty_like(a)
    rc = _load()["c2_packed_loglik"](pk.B, pk.R, dims["J"], pk.offsets, _order(pk, order, dims["J"]), _nz(pk.t), c, ops._bs(c, dims["J"]),
                                     _nz(a), _nz(U), _nz(V), _nz(y), ll, flag, _nz(d), _nz(W), _nz(z), ops._stream())
    _lib.check(rc, "packed.loglik")
    return (ll, flag, d, W, z) if factor else (ll, flag)


def loglik_grad(pk, c, a, U, V, y, *, work=None, out=None, order=_AUTO):
    """The log-likelihood and its gradient -> (ll, (bt, bc, ba, bU, bV, by), flag): bt, ba, by (R,), bU, bV (R, J), bc (B, J)
    per series also for a shared c.  A failed series has ll = -inf and NaN gradients.  With caller-owned `work`
    (workspace(pk, J)) and `out` only ll and flag are allocated."""
    J = U.shape[1] if U.dim() == 2 else 0
    if out is None and U.dim() == 2:
        dev, f = U.device, dict(R=pk.R, B=pk.B, J=J)
        out = tuple(torch.empty(tuple(f[k] for k in s), dtype=torch.float64, device=dev) for _, s in _GRADS)
    dims = _prepare(pk, c, a, U, V, y, [(n, x, s) for (n, s), x in zip(_GRADS, out or ())])
    if work is None:
        work = workspace(pk, J)
    ops._chk(work)
    bt, bc, ba, bU, bV, by = out
    dev = U.device
    ll = torch.empty(pk.B, dtype=torch.float64, device=dev)
    flag = torch.empty(pk.B, dtype=torch.int32, device=dev)
    rc = _load()["c2_packed_loglik_grad"](pk.B, pk.R, pk.n_max, J, pk.offsets, _order(pk, order, J), _nz(pk.t), c, ops._bs(c, J),
                                          _nz(a), _nz(U), _nz(V), _nz(y), ll, _nz(bt), bc, _nz(ba), _nz(bU), _nz(bV), _nz(by),
                                          flag, work, work.numel() * 8, ops._stream())
    _lib.check(rc, "packed.loglik_grad")
    return ll, tuple(out), flag


class _PackedLogLik(torch.autograd.Function):
    """As autograd._LogLik: the gradients come out of the forward call, backward scales them by the incoming cotangent."""

    @staticmethod
    def forward(ctx, pk, t, c, a, U, V, y):
        tens = (t, c, a, U, V, y)
        cd, ad, Ud, Vd, yd = [x.detach().contiguous() for x in tens[1:]]
        if not any(x.requires_grad for x in tens):
            ll, flag = loglik(pk, cd, ad, Ud, Vd, yd)
            return ll
        ll, grads, flag = loglik_grad(pk, cd, ad, Ud, Vd, yd)
        ctx.pk, ctx.shared_c = pk, c.dim() == 1
        ctx.save_for_backward(flag, *grads)
        return ll

    @staticmethod
    def backward(ctx, g):
        # A failed series (ll = -inf, NaN gradients) and a series with a ZERO cotangent contribute exactly zero
        # (autograd._LogLikKernel.backward), so the batch sum of a shared c stays finite.
        flag, bt, bc, ba, bU, bV, by = ctx.saved_tensors
        zero = torch.zeros((), dtype=g.dtype, device=g.device)
        dead = (g == 0) | (flag != 0)
        seg = ctx.pk.seg
        gr, dr = g[seg], dead[seg]
        r1 = lambda v: torch.where(dr, zero, v * gr)
        r2 = lambda v: torch.where(dr[:, None], zero, v * gr[:, None])
        gc = torch.where(dead[:, None], zero, bc * g[:, None])
        return None, r1(bt), gc.sum(0) if ctx.shared_c else gc, r1(ba), r2(bU), r2(bV), r1(by)


def log_likelihood(pk, c, a, U, V, y):
    """The log-likelihood (B,) of a ragged batch, differentiable in pk.t, c, a, U, V, y through torch.autograd.  A series
    whose factorisation fails has ll = -inf and contributes zero gradient; a shared c (J,) receives the batch sum."""
    return _PackedLogLik.apply(pk, pk.t, c, a, U, V, y)


def celerite_rows(coefs, pk, diag):
    """(c (B, J), a (R,), U (R, J), V (R, J)) of packed rows from per-series coefficients (ar, cr, ac, bc, cc, dc), each
    (B, Jr) / (B, Jc) as autograd.term_coefficients returns them (a (Jr,) / (Jc,) one is shared by the batch), the times
    pk.t and the diagonal `diag` (R,): get_celerite_matrices (terms.py:117-177 of the reference) with every row taking the
    coefficients of its series, the columns of a complex term interleaved.  Plain torch: autograd differentiates it, and it
    runs on CPU tensors too."""
    ar, cr, ac, bc, cc, dc = [v if v.dim() == 2 else v[None].expand(pk.B, -1) for v in coefs]
    if ar.shape[0] != pk.B or ac.shape[0] != pk.B:
        raise ValueError("Invalid shape: coefficients (must be (B, Jr) / (B, Jc) with B = %d)" % pk.B)
    if tuple(diag.shape) != (pk.R,):
        raise ValueError("Invalid shape: diag (must be (R,) = (%d,))" % pk.R)
    seg, t = pk.seg, pk.t
    a = diag + (ar.sum(1) + ac.sum(1))[seg]
    arg = dc[seg] * t[:, None]
    cs, sn = torch.cos(arg), torch.sin(arg)
    acr, bcr = ac[seg], bc[seg]
    Uc = torch.stack([acr * cs + bcr * sn, acr * sn - bcr * cs], dim=2).reshape(pk.R, -1)
    Vc = torch.stack([cs, sn], dim=2).reshape(pk.R, -1)
    arr = ar[seg]
    U = torch.cat([arr, Uc], dim=1)
    V = torch.cat([torch.ones_like(arr), Vc], dim=1)
    c = torch.cat([cr, cc.repeat_interleave(2, dim=1)], dim=1)   # (terms.py:171-173)
    return c, a, U, V


def log_likelihood_kernel(kernel, pk, y, *, yerr=None, diag=None, jitter=None, mean=None):
    """The log-likelihood (B,) of a ragged batch as a differentiable function of the HYPER-PARAMETERS, with
    autograd.log_likelihood_kernel's conventions: the tensor parameters of `kernel` (0-d or (B,)), `jitter` (added in
    quadrature) and `mean` (subtracted), floats, 0-d or (B,); y and yerr | diag are (R,).  The chain term_coefficients ->
    celerite_rows -> log_likelihood; a TermExpr's diagonal shift is added to the diagonal.  A kernel with a TermConvolution
    anywhere in it is refused."""
    from . import autograd

    if (yerr is None) == (diag is None):
        raise ValueError("exactly one of 'yerr' and 'diag' (R,) is required")
    if not isinstance(pk, Packed):
        raise TypeError("celerite2_amd.packed: pk must be a Packed")
    if tuple(y.shape) != (pk.R,):
        raise ValueError("Invalid shape: y (must be (R,) = (%d,))" % pk.R)
    if autograd._has_convolution(kernel):
        raise ValueError("packed.log_likelihood_kernel does not take a kernel with a TermConvolution in it (not semiseparable "
                         "inside the exposure window): use predict(y, t, return_var=True)")
    if not kernel._has_tensors():
        raise TypeError("packed.log_likelihood_kernel: the kernel has no tensor parameter (give its parameters as device tensors)")
    B, seg = pk.B, pk.seg
    *coefs, shift = autograd.term_coefficients(kernel.program, kernel.parameter_matrix(B), B, with_shift=True)
    D = (yerr * yerr if diag is None else diag) + shift[seg]
    jitter, mean = autograd._per_series(jitter, B, y), autograd._per_series(mean, B, y)
    if jitter is not None:
        D = D + (jitter * jitter)[seg]
    r = y if mean is None else y - mean[seg]
    c, a, U, V = celerite_rows(coefs, pk, D)
    return log_likelihood(pk, c, a, U, V, r)
