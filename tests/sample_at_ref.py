# -*- coding: utf-8 -*-
"""numpy restatement of the joint prior draw on the merge of two sorted grids (celerite2_amd/csrc/c2_priordraw.hip) and of
what it is checked against: the dense zero-noise kernel matrix on [t, ts], and the dense conditional mean and covariance
that the Matheron chain built on the draw must reproduce.  Test infrastructure only -- nothing here is imported by the
package.

Walk the merge of t and ts upwards, data first on a tie (predict_at_ref's ties="data_first").  An event at time s has
rows u, v and a vector z of K standard normals: U[n], V[n], nt[n] for a data event, Us[m], Vs[m], ns[m] for a query.
With S = 0 (J x J) and F = 0 (J x K) in front of the first event:

    p = exp(-c (s - s_prev));  S <- (p p^T) o S;  F <- p o F          (not at the first event)
    h = S u;  w^ = v - h;  d = u^T w^;  a = u^T v;  f = u^T F          (a = k(0) for every term but a convolution)
    if d > TAU a:   f += sqrt(d) z;   S += w^ w^^T / d;   F += w^ z^T / sqrt(d)      else: nothing more (determined)
    store f (K values) to ft[n] or fs[m]

This is the Cholesky factor of the zero-noise kernel matrix on the merged grid applied to the normals; w^ = d w is the
unnormalised row of W, so a pivot that is zero never divides.  A point is determined when it coincides with an earlier
one: its d is rounding noise of order J eps k(0), and skipping it loses at most TAU k(0) of variance.
"""
import numpy as np

from predict_at_ref import cross, dense, draw, draw_with_queries, err, queries  # noqa: F401  (re-exported for the tests)

TAU = 2.0 ** -44
KINDS = ["mixed", "before", "after", "equal", "dups", "cluster"]


def make_queries(kind, t, M, rng):
    """M sorted query times relative to the data grid t (the six kinds of tests/test_gpu_predict_at.py, copied)."""
    N = len(t)
    if kind == "before":
        return np.sort(t[0] - rng.uniform(1e-3, 3.0, M))
    if kind == "after":
        return np.sort(t[-1] + rng.uniform(1e-3, 3.0, M))
    if kind == "equal":     # data times only (repeats as soon as M > N)
        return np.sort(t[rng.integers(0, N, M)])
    if kind == "cluster":   # every query in ONE gap: all the other gaps are empty
        if N == 1:
            return np.sort(t[0] + rng.uniform(0.0, 0.5, M))
        k = N // 2 - 1 if N > 1 else 0
        return np.sort(t[k] + (t[k + 1] - t[k]) * rng.uniform(0.0, 1.0, M))
    ts = queries(t, rng, M)
    if kind == "dups":
        ts[1::2] = ts[:-1:2][:len(ts[1::2])]
    return np.sort(ts)


def prior_draw(t, ts, c, U, V, Us, Vs, nt, ns, *, dtype=np.float64, report=False):
    """ft (N, K), fs (M, K): the joint draw, computed in `dtype` (np.longdouble: the same recurrence in extended
    precision).  With `report` also a list with one tuple per event, (kind "d" | "q", row index, skipped, d / a)."""
    cast = lambda x: np.asarray(x, dtype=dtype)
    t, ts, c, U, V, Us, Vs, nt, ns = map(cast, (t, ts, c, U, V, Us, Vs, nt, ns))
    N, J = U.shape
    M, K = ns.shape
    tau = dtype(TAU)
    ft, fs = np.empty((N, K), dtype=dtype), np.empty((M, K), dtype=dtype)
    S, F = np.zeros((J, J), dtype=dtype), np.zeros((J, K), dtype=dtype)
    events = []
    n = m = 0
    s_prev = None
    while n < N or m < M:
        data = n < N and (m >= M or t[n] <= ts[m])
        s, u, v, z = (t[n], U[n], V[n], nt[n]) if data else (ts[m], Us[m], Vs[m], ns[m])
        if s_prev is not None:
            p = np.exp(-c * (s - s_prev))
            S = np.outer(p, p) * S
            F = p[:, None] * F
        h = S @ u
        w = v - h
        d, a = u @ w, u @ v
        f = u @ F
        take = bool(d > tau * a)
        if take:
            r = np.sqrt(d)
            f = f + r * z
            S = S + np.outer(w, w) / d
            F = F + np.outer(w, z) / r
        events.append(("d" if data else "q", n if data else m, not take, float(d / a)))
        if data:
            ft[n] = f
            n += 1
        else:
            fs[m] = f
            m += 1
        s_prev = s
    return (ft, fs, events) if report else (ft, fs)


def dense_prior(t, ts, c, k0, U, V, Us, Vs):
    """The zero-noise kernel matrix on the concatenation [t, ts] (N + M square): inverse_diag_ref.dense with a = k(0) on
    the time-sorted rows, put back in the order given."""
    tt = np.concatenate([t, ts])
    UU, VV = np.concatenate([U, Us]), np.concatenate([V, Vs])
    o = np.argsort(tt, kind="stable")
    Ks = dense(tt[o], c, np.full(len(tt), k0), UU[o], VV[o])
    K = np.empty_like(Ks)
    K[np.ix_(o, o)] = Ks
    return K


def dense_conditional(case):
    """(mu (M,), cov (M, M)): the conditional mean (zero prior mean) and covariance at case["ts"] given case["y"] at
    case["t"] with the white noise case["diag"], from dense algebra."""
    N = len(case["t"])
    Kall = dense_prior(case["t"], case["ts"], case["c"], case["k0"], case["U"], case["V"], case["Us"], case["Vs"])
    Kd = Kall[:N, :N] + np.diag(case["diag"])
    Ks, Kss = Kall[:N, N:], Kall[N:, N:]
    sol = np.linalg.solve(Kd, np.concatenate([case["y"][:, None], Ks], axis=1))
    return Ks.T @ sol[:, 0], Kss - Ks.T @ sol[:, 1:]


def matheron(case, nt, ns, ne):
    """fs + K* ^T (K + D)^-1 (y - ft - sqrt(D) ne), (M, K): the chain gp.sample_at runs, with the prior draw from the
    restatement and everything behind it in dense numpy."""
    N = len(case["t"])
    ft, fs = prior_draw(case["t"], case["ts"], case["c"], case["U"], case["V"], case["Us"], case["Vs"], nt, ns)
    Kd = dense(case["t"], case["c"], case["a"], case["U"], case["V"])
    Ks = cross(case["t"], case["ts"], case["c"], case["U"], case["V"], case["Us"], case["Vs"])
    resid = case["y"][:, None] - ft - np.sqrt(case["diag"])[:, None] * ne
    return fs + Ks.T @ np.linalg.solve(Kd, resid)
