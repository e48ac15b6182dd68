# -*- coding: utf-8 -*-
"""CPU checks of posterior draws at new times: the numpy restatement of the joint prior draw on the merge of the data and
the query grid (tests/sample_at_ref.py, what the GPU tests compare c2_prior_draw with) against dense algebra.

Fed identity normals -- one draw per unit vector -- the recurrence IS a linear map, so a distribution is checked
deterministically: A A^T must be the covariance.  Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 floor.
These tests pin the recurrence; they do not touch the device."""
import numpy as np
import pytest

import sample_at_ref as R

WIDTHS = [1, 2, 3, 5, 8, 16, 32]
SIZES = [(1, 1), (2, 15), (17, 15), (33, 16)]
KINDS, make_queries = R.KINDS, R.make_queries


def cases(J):
    for N, M in SIZES:
        for i, kind in enumerate(KINDS):
            seed = 10000 * J + 100 * N + i
            t = R.draw(seed, N, J)["t"]
            ts = make_queries(kind, t, M, np.random.default_rng(seed + 1))
            yield (N, M, kind), R.draw_with_queries(seed, N, J, t=t, ts=ts)


@pytest.mark.parametrize("J", WIDTHS)
def test_prior_draw_has_the_prior_covariance(J):
    """Identity normals: ft, fs stacked are the linear map A0 with A0 A0^T = the dense zero-noise kernel matrix on
    [t, ts]; u^T v = k(0) on every row (what the threshold is relative to)."""
    worst = 0.0
    for what, case in cases(J):
        t, ts, c, U, V, Us, Vs, k0 = (case[k] for k in ("t", "ts", "c", "U", "V", "Us", "Vs", "k0"))
        N, M = len(t), len(ts)
        for rows_u, rows_v in ((U, V), (Us, Vs)):
            a = np.einsum("nj,nj->n", rows_u, rows_v)
            assert np.all(np.abs(a - k0) <= (J + 2) * np.finfo(float).eps * k0), what   # J products and J - 1 sums of terms that add to k(0)
        eye = np.eye(N + M)
        ft, fs = R.prior_draw(t, ts, c, U, V, Us, Vs, eye[:N], eye[N:])
        A0 = np.concatenate([ft, fs])
        e = R.err(A0 @ A0.T, R.dense_prior(t, ts, c, k0, U, V, Us, Vs), floor=k0)
        worst = max(worst, e)
        assert e <= 1.0, (what, e)
    print("J=%d worst prior covariance error / criterion: %.3g" % (J, worst))


@pytest.mark.parametrize("J", WIDTHS)
def test_matheron_draw_has_the_conditional_mean_and_covariance(J):
    """The chain of gp.sample_at in dense numpy around the restatement, identity normals for (nt, ns, ne) plus one all-zero
    draw: the zero draw is the dense conditional mean, and the other draws minus it are A with A A^T = the dense
    conditional covariance."""
    worst = [0.0, 0.0]
    for what, case in cases(J):
        N, M = len(case["t"]), len(case["ts"])
        Z = np.concatenate([np.eye(2 * N + M), np.zeros((2 * N + M, 1))], axis=1)
        out = R.matheron(case, Z[:N], Z[N:N + M], Z[N + M:])
        mu_o, cov_o = R.dense_conditional(case)
        e_mu = R.err(out[:, -1], mu_o)
        A = out[:, :-1] - out[:, -1:]
        e_cov = R.err(A @ A.T, cov_o, floor=case["k0"])
        worst = [max(worst[0], e_mu), max(worst[1], e_cov)]
        assert e_mu <= 1.0, (what, "mean", e_mu)
        assert e_cov <= 1.0, (what, "covariance", e_cov)
    print("J=%d worst conditional mean, covariance error / criterion: %.3g, %.3g" % (J, worst[0], worst[1]))


@pytest.mark.parametrize("J", WIDTHS)
def test_float64_against_long_double(J):
    """The same function in long double: individual float64 draws sit inside the standing criterion with floor max |f_o|
    (the margin the device's other rounding order has against this restatement)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is double on this platform")
    worst = 0.0
    for i, (N, M, kind) in enumerate([(17, 15, "mixed"), (33, 16, "equal"), (150, 150, "mixed"), (150, 150, "dups"), (150, 40, "cluster")]):
        seed = 20000 * J + i
        t = R.draw(seed, N, J, gap=(i == 2))["t"]
        ts = make_queries(kind, t, M, np.random.default_rng(seed + 1))
        case = R.draw_with_queries(seed, N, J, t=t, ts=ts)
        rng = np.random.default_rng(seed + 2)
        nt, ns = rng.standard_normal((N, 3)), rng.standard_normal((M, 3))
        args = [case[k] for k in ("t", "ts", "c", "U", "V", "Us", "Vs")] + [nt, ns]
        f = np.concatenate(R.prior_draw(*args))
        fo = np.concatenate(R.prior_draw(*args, dtype=np.longdouble)).astype(np.float64)
        e = R.err(f, fo)
        worst = max(worst, e)
        assert e <= 1.0, (N, M, kind, e)
    print("J=%d worst float64 - long double / criterion: %.3g" % (J, worst))


@pytest.mark.parametrize("J", [1, 3, 8, 32])
def test_skip_report(J):
    """The per-event report: one entry per event in merge order (data first on a tie); an event is skipped exactly when
    its time equals the time of the event in front of it; skipped events have |d / a| <= TAU / 16 and every other event
    d / a >= 16 TAU -- far from the threshold on both sides."""
    for i, kind in enumerate(KINDS):
        N, M = 33, 16
        seed = 30000 * J + i
        t = R.draw(seed, N, J)["t"]
        if kind == "dups":
            t[5] = t[4]   # repeated data times too
        ts = make_queries(kind, t, M, np.random.default_rng(seed + 1))
        case = R.draw_with_queries(seed, N, J, t=t, ts=ts)
        z = np.zeros((N + M, 1))
        _, _, events = R.prior_draw(*[case[k] for k in ("t", "ts", "c", "U", "V", "Us", "Vs")], z[:N], z[N:], report=True)
        assert len(events) == N + M
        assert [e[1] for e in events if e[0] == "d"] == list(range(N)) and [e[1] for e in events if e[0] == "q"] == list(range(M))
        times = np.array([t[e[1]] if e[0] == "d" else ts[e[1]] for e in events])
        assert np.all(np.diff(times) >= 0)
        for a, b in zip(events[:-1], events[1:]):
            if (t[a[1]] if a[0] == "d" else ts[a[1]]) == (t[b[1]] if b[0] == "d" else ts[b[1]]):
                assert not (a[0] == "q" and b[0] == "d"), kind   # data first on a tie
        expect = np.concatenate([[False], np.diff(times) == 0])
        assert [e[2] for e in events] == expect.tolist(), kind
        if kind in ("equal", "dups"):
            assert expect.any()
        for kind_e, row, skipped, ratio in events:
            assert (abs(ratio) <= R.TAU / 16) if skipped else (ratio >= 16 * R.TAU), (kind, kind_e, row, skipped, ratio)
