# -*- coding: utf-8 -*-
"""Device arrays that start 8 bytes off a 16-byte boundary (plain helpers, no tests).

The C ABI promises 8-byte alignment of every double* (include/celerite2_amd.h); the torch allocator hands out blocks
aligned to 256 bytes and more, so the suite's own tensors never show a kernel anything else.  `off16` / `empty_off16`
place an array at element 1 of a 16-byte aligned buffer of numel + 2 doubles -- what `y[1:]` of a batch with an odd number
of rows looks like -- and fill the two doubles that flank it with SENTINEL, which `flanks_intact` checks afterwards."""
import numpy as np

SENTINEL = -1.2345678e300   # (finite: compared with ==)


def _buffer(numel):
    import torch
    buf = torch.full((numel + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf


def _view(buf, shape):
    numel = buf.numel() - 2
    v = buf[1:1 + numel].view(tuple(shape))
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    v.guard_buffer = buf   # (the view keeps the buffer alive anyway; this names it for flanks_intact)
    return v


def off16(x):
    """A contiguous float64 device copy of `x` (numpy array or tensor) whose first byte is 8 past a 16-byte boundary."""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) if isinstance(x, np.ndarray) else x
    buf = _buffer(src.numel())
    buf[1:1 + src.numel()].copy_(src.reshape(-1))
    return _view(buf, src.shape)


def empty_off16(shape, fill=float("nan")):
    """The same for an output: `shape` doubles filled with `fill` (NaN: an element the op leaves out shows)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    buf = _buffer(int(np.prod(shape, dtype=np.int64)))
    buf[1:-1] = fill
    return _view(buf, shape)


def flanks_intact(v):
    """The two doubles around an off16 / empty_off16 array still hold the sentinel."""
    buf = v.guard_buffer
    return float(buf[0]) == SENTINEL and float(buf[-1]) == SENTINEL
