# -*- coding: utf-8 -*-
"""Streaming updates of a factored GP: the torch part (kernel: csrc/c2_filter.hip, ops.filter_*).

A `Filter` holds, per series, the state behind its last row -- t_last, n, sum log d, sum z^2 / d, and the F and S of the
reference's solve_lower and factor -- and appends rows in O(M J^2) without the old ones.  The d and z of an appended row are
its one-step-ahead predictive variance and its innovation: z / sqrt(d) is the anomaly score of an alert stream.

    flt = gp.filter(y)                        # after gp.compute: one solve_lower and one absorb, nothing is refactored
    flt = Filter.empty(kernel, B, device=dev) # or from nothing
    upd = flt.append(t_new, y_new, yerr=e_new, count=count)   # Update(innovation, variance, score, flag)
    mu, var = flt.forecast(t_query)
    flt.log_likelihood                        # (B,), that of every row absorbed so far

No gradients, and no kernels with tensor hyper-parameters: both are out of scope here."""
import collections
import math

import torch

from . import ops

Update = collections.namedtuple("Update", "innovation variance score flag")


class Filter:
    def __init__(self, kernel, state, *, mean=0.0):
        from .terms import TermConvolution

        if isinstance(kernel, TermConvolution):
            raise ValueError("a Filter does not take a TermConvolution kernel (not semiseparable inside the exposure window)")
        if kernel._has_tensors():
            raise ValueError("a Filter does not take a kernel with tensor hyper-parameters")
        if state.dim() != 2 or state.shape[1] != ops.filter_state_words(kernel.width):
            raise ValueError("Invalid shape: state %s, expected (B, %d)" % (tuple(state.shape), ops.filter_state_words(kernel.width)))
        self.kernel = kernel
        self.mean = mean if torch.is_tensor(mean) else float(mean)
        self.state = state

    @classmethod
    def empty(cls, kernel, B, *, mean=0.0, device="cuda"):
        """A filter of B series that has seen nothing."""
        return cls(kernel, ops.filter_init(B, kernel.width, device), mean=mean)

    # -- what the state holds ------------------------------------------------------------------------------------------
    @property
    def n(self):
        """Rows absorbed per series, (B,) int64."""
        return self.state[:, 1].to(torch.int64)

    @property
    def t_last(self):
        """Time of the last absorbed row per series, (B,) (meaningless where n == 0)."""
        return self.state[:, 0]

    @property
    def log_likelihood(self):
        """(B,) = -(1/2) (sum z^2 / d + sum log d + n log 2 pi) of every row absorbed so far."""
        return -0.5 * (self.state[:, 3] + self.state[:, 2] + self.state[:, 1] * math.log(2 * math.pi))

    def clone(self):
        return Filter(self.kernel, self.state.clone(), mean=self.mean)

    def _rows(self, t, diag, name):
        B = self.state.shape[0]
        if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != B):
            raise ValueError("Invalid shape: %s %s, expected (M,) or (%d, M)" % (name, tuple(t.shape), B))
        if tuple(diag.shape) != (B, t.shape[-1]):
            raise ValueError("Invalid shape: diag %s, expected %s" % (tuple(diag.shape), (B, t.shape[-1])))
        return self.kernel.get_celerite_matrices(t.contiguous(), diag.contiguous())

    # -- append ----------------------------------------------------------------------------------------------------------
    def append(self, t_new, y_new, *, yerr=None, diag=None, count=None, check_sorted=True):
        """Append the rows (t_new (M,) | (B, M), y_new (B, M)) with white noise `yerr` or `diag` (B, M); `count` (B,) int32
        says how many of the M rows each series takes (rows beyond it are not read, a series with 0 keeps its state).
        The state advances in place.  Returns Update(innovation z, variance d, score z / sqrt(d), flag): (B, M) each, NaN
        in the rows that were not taken, and flag (B,) int32 -- the 1-based row whose predictive variance came out <= 0
        (the rows before it are returned, the series' state is left as it was), else 0."""
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        if yerr is not None:
            diag = yerr**2
        if diag is None:
            raise ValueError("'diag' or 'yerr' (B, M) is required")
        B, M = self.state.shape[0], t_new.shape[-1]
        if tuple(y_new.shape) != (B, M):
            raise ValueError("Invalid shape: y_new %s, expected %s" % (tuple(y_new.shape), (B, M)))
        if check_sorted:
            self._check_sorted(t_new, count)
        c, a, U, V = self._rows(t_new, diag, "t_new")
        r = (y_new - self.mean).contiguous()
        d, z = (torch.full((B, M), math.nan, dtype=torch.float64, device=self.state.device) for _ in range(2))
        W = torch.full((B, M, U.shape[-1]), math.nan, dtype=torch.float64, device=self.state.device)
        _, d, W, z, flag = ops.filter_append(self.state, t_new.contiguous(), c, a, U, V, r, count=count, out=self.state,
                                             d=d, W=W, z=z)
        return Update(z, d, z / torch.sqrt(d), flag)

    def _check_sorted(self, t_new, count):
        """The rows a series takes are non-decreasing in time and not before its t_last (the kernel does not check)."""
        B, M = self.state.shape[0], t_new.shape[-1]
        t = t_new if t_new.dim() == 2 else t_new[None, :].expand(B, M)
        if count is None:
            taken = torch.ones((B, M), dtype=torch.bool, device=t.device)
        else:
            taken = torch.arange(M, device=t.device)[None, :] < count[:, None]
        bad = ((t[:, 1:] < t[:, :-1]) & taken[:, 1:]).any()
        bad = bad | ((t[:, 0] < self.t_last) & taken[:, 0] & (self.state[:, 1] > 0)).any()
        if bool(bad):
            raise ValueError("The new coordinates must be sorted and not before the last absorbed time")

    # -- forecast --------------------------------------------------------------------------------------------------------
    def forecast(self, t, *, diag=None, include_mean=True):
        """(mu, var) (B, M) at the times t (M,) | (B, M), each row independently from the present state; `diag` (B, M) is
        added to the variance (white noise of the would-be observation).  For times at or after t_last this is the full
        conditional given every absorbed row; an earlier time is refused (use gp.predict_at for those)."""
        B = self.state.shape[0]
        if diag is None:
            diag = torch.zeros((B, t.shape[-1]), dtype=torch.float64, device=self.state.device)
        tq = t if t.dim() == 2 else t[None, :]
        if bool(((tq < self.t_last[:, None]) & (self.state[:, 1:2] > 0)).any()):
            raise ValueError("The forecast coordinates must not be before the last absorbed time")
        c, a, U, _ = self._rows(t, diag, "t")
        mu, var = ops.filter_forecast(self.state, t.contiguous(), c, a, U)
        return (mu + self.mean if include_mean else mu), var
