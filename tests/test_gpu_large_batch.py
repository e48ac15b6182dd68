# -*- coding: utf-8 -*-
"""Every public op on EVERY series of a batch beyond 65535 (gridDim.y and gridDim.z stop there): B = 70000 series, seven
distinct ones repeated -- 70000 is no multiple of 64, and 65535 mod 7 = 1, 65536 mod 7 = 2, so a series index that wraps at
either limit lands on another series and shows as a mismatch.

Per row of tests/large_batch_cases.py: the references of the seven come from the oracle / restatement call of the op's own test
file, are uploaded and compared with all 70000 outputs on the device under that file's own criterion (one torch expression;
large_batch_cases.worst_ratio); caller outputs are pre-filled with NaN, so a series that is never written shows; a `fail` row
gives one of the seven a non-positive pivot and wants flag != 0 exactly at its repeats, every other series still inside its
criterion.  Bit equality with the repeat is asserted only where row.bits says why it holds.  Where a planning hook exists
(c2_internal_loglik_grad_plan, c2_internal_loglik_terms_plan, c2_internal_general_chunks_plan) the mapping it reports for the call is
recorded and must be the one the row names (row.plan: one lane per series, a group of lanes, the composed chain; no chunks along
time) -- none of the forms the launchers keep below 65536 series.  At these small shapes those forms would be declined at any
batch size (four rows are too few for the time-parallel form, three right-hand sides too few for chunks), so the assertion pins
the kernel family a row runs, not the B <= 65535 clause itself.

What this file found when it was written: c2_colsumsq_over_d (and with it gp.predict(..., return_var=True)), c2_kron_loglik and
c2_kron_loglik_grad refused B > 65535 -- their kernels now stride over the batch; every other row passed on the code as it was.
Measured then, worst |err| / bound per family: the core ops and their reverses <= 5e-5, the coefficient-level log-likelihoods
<= 3e-4 (loglik_kernel_grad at width 8: 1.3e-3), kernel_values 1e-3, kron interleaved 2e-3 (collapsed 5e-5), the searches, projections and filter ops <= 3e-5,
noise_mean_apply 0.42 of its 4 * 2^-53, noise_mean_rev 0.02 of its 1e-14; test_worst_case_report prints them per row."""
import numpy as np
import pytest

import large_batch_cases as L

pytestmark = pytest.mark.gpu
WORST = {}
MAPPINGS = {}


@pytest.fixture(scope="module")
def ops():
    import torch
    from celerite2_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def raw():
    return L.plan_hooks()


@pytest.mark.parametrize("row", L.ROWS, ids=[r.id for r in L.ROWS])
def test_every_series_of_seventy_thousand(ops, oracle, raw, row):
    import torch

    inp = row.build()
    want = row.ref(oracle, inp)
    T = {k: (v if k.startswith("_") else L.expand(torch, v)) for k, v in inp.items()}
    if row.plan:
        MAPPINGS[row.id] = L.mapping_of(raw, row, inp)
        assert MAPPINGS[row.id] == row.plan[1], (row.id, MAPPINGS[row.id], row.plan)
    got = row.run(ops, torch, T)
    torch.cuda.synchronize()
    keep = row.keep
    flag_o = want.pop("flag", None)
    if "flag" in got:
        flag = got.pop("flag").view(L.REPS, L.D)
        bad = (flag != 0)
        expect = torch.zeros(L.D, dtype=torch.bool, device="cuda")
        if row.fail:
            expect[L.FAIL] = True
        assert torch.equal(bad, expect[None].expand_as(bad)), (row.id, "flag != 0 at", torch.nonzero(bad != expect[None])[:5].tolist())
        assert flag_o is not None and bool((torch.from_numpy(np.asarray(flag_o) != 0).cuda() == expect).all()), row.id
    assert set(want) <= set(got), (row.id, sorted(set(want) - set(got)))
    for name, xo in want.items():
        x = got[name]
        assert tuple(x.shape) == (L.B,) + xo.shape[1:], (row.id, name, tuple(x.shape), xo.shape)
        if not xo[0].size:
            continue
        allowed = np.ascontiguousarray(row.crit[name](xo, keep, inp))
        e = L.worst_ratio(torch, x, torch.from_numpy(np.ascontiguousarray(xo)).cuda(), torch.from_numpy(allowed).cuda(), keep,
                          where_ref=name in row.where_ref)
        key = "%s %s" % (row.id, name)
        WORST[key] = e
        print("%s: %.3g of the criterion" % (key, e))
        assert e <= 1.0, (row.id, name, e)
        if row.bits:
            xv = x.reshape((L.REPS, L.D) + tuple(x.shape[1:]))[:, keep]
            assert bool((xv == xv[:1]).all()), (row.id, name, "a repeat differs from its original", row.bits)


# ---- the front end ----------------------------------------------------------------------------------------------------------
def test_predict_with_variance_at_seventy_thousand(ops):
    """gp.predict(y, t, return_var=True) and ConditionalDistribution.variance at 70000 x 4, M = 3 (c2_colsumsq_over_d refused this
    batch): against dense conditioning of the seven series, with test_gpu_ops.test_predictive_variance_and_covariance's bounds
    (mean rtol 1e-8 / atol 1e-9, variance rtol 1e-7 / atol 1e-9)."""
    import torch
    from celerite2_amd import gp as gpmod, terms

    rng = np.random.default_rng(40583)
    x = np.sort(rng.uniform(0, 10, (L.D, L.N)), axis=1)
    ts = np.sort(rng.uniform(-1, 12, (L.D, L.M)), axis=1)
    diag = rng.uniform(0.1, 0.3, (L.D, L.N))
    y = np.sin(x)
    S0 = rng.uniform(4.0, 6.0, L.D)
    xd, tsd, dd, yd = (L.expand(torch, v) for v in (x, ts, diag, y))
    kernel = terms.SHOTerm(S0=np.tile(S0, L.REPS), w0=0.1, Q=3.45) + terms.RealTerm(a=1.0, c=0.1)
    gp = gpmod.GaussianProcess(kernel, mean=0.3)
    gp.compute(xd, diag=dd)
    mu, var = gp.predict(yd, tsd, return_var=True)
    var2 = gp.condition(yd, tsd).variance
    torch.cuda.synchronize()
    want_mu, want_var = np.empty((L.D, L.M)), np.empty((L.D, L.M))
    for b in range(L.D):
        kb = terms.SHOTerm(S0=float(S0[b]), w0=0.1, Q=3.45) + terms.RealTerm(a=1.0, c=0.1)
        K = kb.get_value(x[b][:, None] - x[b][None, :]) + np.diag(diag[b])
        Ks = kb.get_value(ts[b][:, None] - x[b][None, :])
        Kss = kb.get_value(ts[b][:, None] - ts[b][None, :])
        want_mu[b] = Ks @ np.linalg.solve(K, y[b] - 0.3) + 0.3
        want_var[b] = np.diag(Kss - Ks @ np.linalg.solve(K, Ks.T))
    keep = list(range(L.D))
    for name, x_, xo, rtol in (("mu", mu, want_mu, 1e-8), ("var", var, want_var, 1e-7), ("variance", var2, want_var, 1e-7)):
        assert tuple(x_.shape) == (L.B, L.M)
        allowed = rtol * np.abs(xo) + 1e-9
        e = L.worst_ratio(torch, x_, torch.from_numpy(xo).cuda(), torch.from_numpy(allowed).cuda(), keep)
        WORST["gp.predict " + name] = e
        print("gp.predict %s: %.3g of the criterion" % (name, e))
        assert e <= 1.0, (name, e)


def test_worst_case_report():
    for k in sorted(WORST):
        print("worst |err| / criterion, %s: %.3g" % (k, WORST[k]))
    for k in sorted(MAPPINGS):
        print("mapping reported by the plan, %s: %d" % (k, MAPPINGS[k]))
