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

A kernel with TENSOR hyper-parameters (and a tensor `mean`, a `jitter`) makes the filter differentiable: `append` then goes
through autograd.filter_append_kernel (reverse: csrc/c2_filter_rev.hip) and REBINDS `flt.state` instead of writing it in
place, the Update it returns and `flt.log_likelihood` carry a graph, and the gradient flows back through as many appends as
the graph holds -- `flt.detach()` cuts it at the present state, for truncated back-propagation night by night:

    flt = Filter.empty(kernel, B, mean=mean, jitter=jitter)   # kernel = terms.SHOTerm(S0=S0, ...) with device tensors
    for t_new, y_new, e_new in nights:
        before = flt.log_likelihood
        flt.append(t_new, y_new, yerr=e_new)
        (before - flt.log_likelihood).sum().backward()        # minus tonight's predictive log density
        optimiser.step(); optimiser.zero_grad(); flt.detach()

`forecast` works on such a filter but returns detached values; `forecast_kernel` is the forecast that carries the graph
(autograd.filter_forecast_kernel, reverse: csrc/c2_filter_stream_rev.hip), and `forecast_log_density` the log density of
what arrived at the forecast times -- forecast skill h nights ahead as a training objective:

    skill = flt.forecast_log_density(t_later, y_later, yerr=e_later)   # (B,), before those rows are appended
    (-skill.sum()).backward()

The future of a correlated process is a path: `sample_forecast` draws the M query times JOINTLY from the state (kernel:
csrc/c2_filter_draw.hip, ops.filter_draw -- the append run backwards in y, the S, d and w of a row shared by all draws), and
`forecast_joint_log_density` is the log density of M arrived rows taken together (an append that does not advance the filter):

    paths = flt.sample_forecast(t_next, size=256)              # (B, 256, M): latent paths; with yerr=...: would-be observations
    share = (paths > threshold).any(dim=2).double().mean(dim=1)   # in what share of futures does a source cross it?
    joint = flt.forecast_joint_log_density(t_later, y_later, yerr=e_later)   # (B,), carries the graph on a differentiable filter

`gp.filter_kernel(y)` builds a differentiable filter from a computed GP (autograd.filter_absorb_kernel): what is appended or
forecast behind it sends its gradient back through the absorbed series.  A filter on a plain kernel behaves as before: in
place, no graph."""
import collections
import math

import torch

from . import ops

Update = collections.namedtuple("Update", "innovation variance score flag")


class Filter:
    def __init__(self, kernel, state, *, mean=0.0, jitter=None):
        from .autograd import _has_convolution
        from .terms import TermConvolution

        if isinstance(kernel, TermConvolution):
            raise ValueError("a Filter does not take a TermConvolution kernel (not semiseparable inside the exposure window)")
        self.differentiable = kernel._has_tensors()
        if self.differentiable and _has_convolution(kernel):
            raise ValueError("a Filter does not take a kernel with a TermConvolution in it (not semiseparable inside the "
                             "exposure window)")
        if jitter is not None and not self.differentiable:
            raise ValueError("'jitter' goes with a kernel of tensor hyper-parameters (else add it to yerr)")
        if state.dim() != 2 or state.shape[1] != ops.filter_state_words(kernel.width):
            raise ValueError("Invalid shape: state %s, expected (B, %d)" % (tuple(state.shape), ops.filter_state_words(kernel.width)))
        self.kernel = kernel
        self.mean = mean if torch.is_tensor(mean) else float(mean)
        self.jitter = jitter
        self.state = state

    @classmethod
    def empty(cls, kernel, B, *, mean=0.0, jitter=None, device="cuda"):
        """A filter of B series that has seen nothing."""
        return cls(kernel, ops.filter_init(B, kernel.width, device), mean=mean, jitter=jitter)

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
        return Filter(self.kernel, self.state.clone(), mean=self.mean, jitter=self.jitter)

    def detach(self):
        """Cut the graph at the present state: later appends send no gradient into the earlier ones.  Returns self."""
        self.state = self.state.detach()
        return self

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
        The state advances in place -- under a kernel with tensor hyper-parameters `self.state` is rebound to a new tensor
        instead, and everything returned is differentiable in the hyper-parameters, jitter, mean, t_new, y_new, the noise
        and the state before.  Returns Update(innovation z, variance d, score z / sqrt(d), flag): (B, M) each, NaN
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
        if self.differentiable:
            return self._append_graph(t_new, y_new, diag, count)
        c, a, U, V = self._rows(t_new, diag, "t_new")
        r = (y_new - self.mean).contiguous()
        d, z = (torch.full((B, M), math.nan, dtype=torch.float64, device=self.state.device) for _ in range(2))
        W = torch.full((B, M, U.shape[-1]), math.nan, dtype=torch.float64, device=self.state.device)
        _, d, W, z, flag = ops.filter_append(self.state, t_new.contiguous(), c, a, U, V, r, count=count, out=self.state,
                                             d=d, W=W, z=z)
        return Update(z, d, z / torch.sqrt(d), flag)

    def _append_graph(self, t_new, y_new, diag, count):
        from . import autograd

        B, M = y_new.shape
        if t_new.dim() not in (1, 2) or (t_new.dim() == 2 and t_new.shape[0] != B):
            raise ValueError("Invalid shape: t_new %s, expected (M,) or (%d, M)" % (tuple(t_new.shape), B))
        if tuple(diag.shape) != (B, M):
            raise ValueError("Invalid shape: diag %s, expected %s" % (tuple(diag.shape), (B, M)))
        mean = self.mean if torch.is_tensor(self.mean) or self.mean != 0.0 else None
        self.state, d, _, z, flag = autograd.filter_append_kernel(self.kernel, self.state, t_new, y_new, diag=diag,
                                                                  jitter=self.jitter, mean=mean, count=count)
        # the rows that were not taken: NaN, as in place (of a failed series: every row from the failing one on)
        taken = torch.arange(M, device=d.device)[None, :] < (torch.full_like(flag, M) if count is None else count)[:, None]
        at = torch.arange(1, M + 1, device=d.device)[None, :]
        nan = torch.full_like(d, math.nan)
        d = torch.where(taken & ((flag[:, None] == 0) | (at <= flag[:, None])), d, nan)
        z = torch.where(taken & ((flag[:, None] == 0) | (at < flag[:, None])), z, nan)
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
        state, mean = self.state, self.mean
        if self.differentiable:   # detached values: the reverse of forecast is not written
            t, diag, state = t.detach(), diag.detach(), state.detach()
            if torch.is_tensor(mean):
                mean = mean.detach()[:, None] if mean.dim() == 1 else mean.detach()
        c, a, U, _ = self._rows(t, diag, "t")
        mu, var = ops.filter_forecast(state, t.contiguous(), c, a, U)
        return (mu + mean if include_mean else mu), var

    def _check_forecast(self, t, count=None):
        tq = t if t.dim() == 2 else t[None, :]
        early = (tq < self.t_last[:, None]) & (self.state[:, 1:2] > 0)
        if count is not None:
            early = early & (torch.arange(tq.shape[-1], device=tq.device)[None, :] < count[:, None])
        if bool(early.any()):
            raise ValueError("The forecast coordinates must not be before the last absorbed time")

    def forecast_kernel(self, t, *, yerr=None, diag=None, include_mean=True, count=None):
        """`forecast` with its graph, on a filter whose kernel has tensor hyper-parameters: (mu, var) (B, M) at the times t
        (M,) | (B, M), differentiable in the hyper-parameters, the mean, the jitter, the times, the noise and the state --
        and through the state in every append (or gp.filter_kernel) the graph still holds.  Without noise `var` is the
        latent variance; with `yerr` or `diag` (B, M) it is the variance of a would-be observation, jitter^2 included.
        `count` (B,) int32: rows m >= count[b] are not read, their mu and var are 0.  Times before t_last are refused."""
        from . import autograd

        if not self.differentiable:
            raise TypeError("forecast_kernel: the kernel has no tensor parameter (use forecast)")
        self._check_forecast(t, count)
        mean = self.mean if include_mean and (torch.is_tensor(self.mean) or self.mean != 0.0) else None
        return autograd.filter_forecast_kernel(self.kernel, self.state, t, yerr=yerr, diag=diag, jitter=self.jitter, mean=mean,
                                               count=count)

    def forecast_log_density(self, t, y, *, yerr=None, diag=None, count=None):
        """(B,) = sum over the taken rows of log N(y_m | mean + mu_m, var_m): the log density, under the forecast from the
        present state, of the values y (B, M) that arrived at the times t (M,) | (B, M) -- each row on its own (the marginal
        densities; forecast_joint_log_density is that of the rows taken together, and equals this one for M = 1).  The
        noise `yerr` or `diag` (B, M) of those values is required; the filter's jitter
        is added in quadrature.  On a filter with tensor hyper-parameters the result carries the graph (forecast_kernel);
        on a plain one it goes through ops.filter_forecast.  `count` (B,) int32: how many of the M rows each series takes
        (0: that series gives 0).  Times before t_last are refused."""
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        if yerr is None and diag is None:
            raise ValueError("'diag' or 'yerr' (B, M) is required")
        B, M = self.state.shape[0], t.shape[-1]
        if tuple(y.shape) != (B, M):
            raise ValueError("Invalid shape: y %s, expected %s" % (tuple(y.shape), (B, M)))
        if self.differentiable:
            mu, var = self.forecast_kernel(t, yerr=yerr, diag=diag, count=count)
        else:
            self._check_forecast(t, count)
            c, a, U, _ = self._rows(t, yerr**2 if diag is None else diag, "t")
            mu, var = ops.filter_forecast(self.state, t.contiguous(), c, a, U, count=count)
            mu = mu + (self.mean[:, None] if torch.is_tensor(self.mean) and self.mean.dim() == 1 else self.mean)
        if count is not None:   # the rows not taken: a unit normal at its mean, then dropped from the sum
            taken = torch.arange(M, device=y.device)[None, :] < count[:, None]
            mu, var = torch.where(taken, mu, y.detach()), torch.where(taken, var, torch.ones_like(var))
        dens = -0.5 * ((y - mu) ** 2 / var + torch.log(var) + math.log(2.0 * math.pi))
        return (dens if count is None else torch.where(taken, dens, torch.zeros_like(dens))).sum(dim=1)

    def forecast_joint_log_density(self, t, y, *, yerr=None, diag=None, count=None):
        """(B,) = log N(y | mean + mu_c, Sigma_c): the log density, under the forecast from the present state, of the values
        y (B, M) at the times t (M,) | (B, M) TAKEN TOGETHER -- mu_c and Sigma_c the conditional mean and covariance of the
        M rows given every absorbed row.  It is -(1/2) sum (z^2 / d + log d + log 2 pi) over the taken rows of an append
        that does not advance the filter (formed from that append's d and z, not from the states' running sums, which lose
        digits behind thousands of absorbed rows); the filter is left bit for bit as it was.  The noise `yerr` or `diag`
        (B, M) is required, the filter's jitter is added in quadrature.  On a filter with tensor hyper-parameters the
        result carries the graph (autograd.filter_append_kernel); on a plain one it goes through ops.filter_append.
        `count` (B,) int32: how many of the M rows each series takes (0: that series gives 0).  The times must be sorted
        and not before t_last.  NaN where a row's predictive variance came out <= 0."""
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        if yerr is None and diag is None:
            raise ValueError("'diag' or 'yerr' (B, M) is required")
        B, M = self.state.shape[0], t.shape[-1]
        if tuple(y.shape) != (B, M):
            raise ValueError("Invalid shape: y %s, expected %s" % (tuple(y.shape), (B, M)))
        self._check_sorted(t, count)
        if self.differentiable:
            from . import autograd

            mean = self.mean if torch.is_tensor(self.mean) or self.mean != 0.0 else None
            _, d, _, z, flag = autograd.filter_append_kernel(self.kernel, self.state, t, y, yerr=yerr, diag=diag,
                                                             jitter=self.jitter, mean=mean, count=count)
        else:
            c, a, U, V = self._rows(t, yerr**2 if diag is None else diag, "t")
            mean = self.mean[:, None] if torch.is_tensor(self.mean) and self.mean.dim() == 1 else self.mean
            _, d, _, z, flag = ops.filter_append(self.state, t.contiguous(), c, a, U, V, (y - mean).contiguous(), count=count)
        # the rows not taken, and every row of a failed series: a unit normal at its mean, then dropped from the sum
        taken = (flag == 0)[:, None].expand(B, M)
        if count is not None:
            taken = taken & (torch.arange(M, device=y.device)[None, :] < count[:, None])
        d, z = torch.where(taken, d, torch.ones_like(d)), torch.where(taken, z, torch.zeros_like(z))
        dens = torch.where(taken, -0.5 * (z * z / d + torch.log(d) + math.log(2.0 * math.pi)), torch.zeros_like(d)).sum(dim=1)
        return torch.where(flag == 0, dens, torch.full_like(dens, math.nan))

    # -- sample paths ----------------------------------------------------------------------------------------------------
    def sample_forecast(self, t, *, size=None, yerr=None, diag=None, include_mean=True, count=None, generator=None,
                        normals=None, check_sorted=True):
        """Joint draws (B, M) -- (B, size, M) when `size` is given, gp.sample_at's convention -- of the future at the sorted
        times t (M,) | (B, M), none before t_last, given every absorbed row: sample PATHS, where `forecast` gives a mean and
        a variance per time.  One kernel call (ops.filter_draw), O(M (J^2 + J size)) a series, without the old rows: the
        append run backwards in y, y_m = u^T F + sqrt(d_m) eps_m followed by the append of y_m, the S, d and w of a row
        shared by the draws.  The draws equal mu_c + chol(Sigma_c) eps for the conditional mean and covariance of the M rows.

        Without noise arguments the draws are of the LATENT process; with `yerr` or `diag` (B, M) they are of would-be
        observations, the filter's jitter added in quadrature where there is one.  A latent draw at a repeated query time
        (or at t_last itself) has d = 0 there: the row is flagged and the series comes back as NaN (where rounding leaves
        d a few ulps of k(0) above zero instead, the row repeats the value before it) -- give such rows a noise, or
        drop the repeat.  `normals` (B, M, K), K = size (1 for None): the standard normals, for reproducibility;
        otherwise torch.randn(..., generator=generator).  `count` (B,) int32: how many of the M rows each series takes.
        NaN in every row of a series whose predictive variance came out <= 0 somewhere and in the rows beyond `count`.
        The filter is not changed.  On a filter with tensor hyper-parameters the values are detached, as forecast's."""
        if yerr is not None and diag is not None:
            raise ValueError("only one of 'diag' and 'yerr' can be provided")
        B, M, dev = self.state.shape[0], t.shape[-1], self.state.device
        K = 1 if size is None else int(size)
        if K < 1:
            raise ValueError("'size' must be at least 1")
        if normals is not None and tuple(normals.shape) != (B, M, K):
            raise ValueError("Invalid shape: normals %s, expected %s" % (tuple(normals.shape), (B, M, K)))
        noise = diag if yerr is None else yerr**2
        state, mean = self.state, self.mean
        if self.differentiable:   # detached values: the reverse of the draw is not written
            t, state = t.detach(), state.detach()
            if torch.is_tensor(mean):
                mean = mean.detach()
            if noise is not None:
                noise = noise.detach()
                if self.jitter is not None:
                    jit = torch.as_tensor(self.jitter, dtype=torch.float64, device=dev).detach()
                    noise = noise + (jit * jit if jit.dim() == 0 else (jit * jit)[:, None])
        if noise is None:
            noise = torch.zeros((B, M), dtype=torch.float64, device=dev)
        c, a, U, V = (x.detach().contiguous() for x in self._rows(t, noise, "t"))   # (refuses a t or a noise of another shape)
        self._check_forecast(t, count)
        if check_sorted:
            self._check_sorted(t, count)
        if normals is None:
            normals = torch.randn((B, M, K), dtype=torch.float64, device=dev, generator=generator)
        paths = torch.full((B, M, K), math.nan, dtype=torch.float64, device=dev)
        paths, _, flag = ops.filter_draw(state, t.contiguous(), c, a, U, V, normals.contiguous(), count=count, paths=paths)
        out = paths.transpose(1, 2)   # (B, K, M)
        if include_mean:
            out = out + (mean[:, None, None] if torch.is_tensor(mean) and mean.dim() == 1 else mean)
        out = torch.where((flag != 0)[:, None, None], torch.full_like(out, math.nan), out)
        return out[:, 0] if size is None else out
