# -*- coding: utf-8 -*-
"""CPU checks of the variance at new times: the numpy restatement of the two-state recurrence (tests/predict_at_ref.py,
what the GPU tests compare c2_explained_variance with) against k(0) - diag(K*^T (K + D)^-1 K*) from dense algebra.

Criterion: the standing one, |x - x_o| <= 1e-10 |x_o| + 1e-12 k(0), on the variance.  Every draw has a condition
number <= 1e6, asserted per draw.  These tests pin the recurrence; they do not touch the device."""
import numpy as np
import pytest

import predict_at_ref as P

WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32, 40, 128]
SIZES = [1, 2, 33, 150]


@pytest.mark.parametrize("gap", [False, True], ids=["even", "gap"])
@pytest.mark.parametrize("J", WIDTHS)
def test_recurrence_vs_dense(J, gap):
    worst = 0.0
    for N in SIZES:
        case = P.draw_with_queries(1000 * J + N, N, J, 2 * N + 5, gap=gap)
        t, ts, c, a, U, V, Us, Vs, k0 = (case[k] for k in ("t", "ts", "c", "a", "U", "V", "Us", "Vs", "k0"))
        cond = np.linalg.cond(P.dense(t, c, a, U, V))
        assert cond <= 1e6, (N, J, cond)   # a bad draw fails here instead of loosening anything below
        assert np.all(np.diff(ts) >= 0) and len(ts) == 2 * N + 5
        for x in (t[0], t[-1], t[N // 2]):
            assert x in ts
        assert ts[0] < t[0] and ts[-1] > t[-1]
        if N > 2:
            k = int(np.argmax(np.diff(t)))
            assert np.sum((ts > t[k]) & (ts < t[k + 1])) >= 3   # several queries in one gap
            assert (np.max(np.diff(t)) > 50.0) == gap
        d, W = P.factor(t, c, a, U, V)
        var_o = k0 - P.dense_explained(t, ts, c, a, U, V, Us, Vs)
        assert np.all(var_o > 0) and np.all(var_o <= k0 * (1 + 1e-12))
        for ties in ("data_first", "query_first"):   # a query at a data time: the same value from either side
            var = k0 - P.explained_variance(t, ts, c, U, W, d, Us, Vs, ties=ties)
            e = P.err(var, var_o, floor=k0)
            worst = max(worst, e)
            assert e <= 1.0, (N, J, gap, ties, e)
    print("J=%d gap=%s worst variance error / criterion: %.3g" % (J, gap, worst))


def test_cross_covariance_matches_the_data_rows():
    """K* built from U, V, U*, V* at queries equal to the data times is the kernel part of the dense matrix."""
    case = P.draw_with_queries(5, 33, 5, ts=P.draw(5, 33, 5)["t"])
    K = P.dense(case["t"], case["c"], case["a"], case["U"], case["V"]) - np.diag(case["diag"])
    Ks = P.cross(case["t"], case["ts"], case["c"], case["U"], case["V"], case["Us"], case["Vs"])
    assert P.err(Ks, K) <= 1.0
