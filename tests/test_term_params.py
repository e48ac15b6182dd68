# -*- coding: utf-8 -*-
"""The yardstick of the device term-parameter kernels (csrc/c2_term_params.hip), pinned on the CPU: the numpy restatement
of program -> coefficients (tests/term_params_ref.py) against the coefficients the REFERENCE's term classes produced
(tests/golden/ref_golden.npz, `coef_<name>_*`, written by tests/golden/make_golden_ref.py), and the hand-written reverse
formulas against the exact complex-step Jacobian of that restatement."""
import numpy as np
import pytest

import term_params_ref as R
from oracle import exact

NAMES = ("ar", "cr", "ac", "bc", "cc", "dc")
S, RH, TA = R.SIGMA, R.RHO, R.TAU

GOLDEN_CASES = R.GOLDEN_CASES


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_restatement_reproduces_the_reference_coefficients(golden, name):
    prog, P = GOLDEN_CASES[name]
    got = R.coefficients(prog, np.array(P))
    for cn, g in zip(NAMES, got):
        want = golden["coef_%s_%s" % (name, cn)]
        assert g.shape == want.shape, (cn, g.shape, want.shape)
        if want.size:
            assert np.max(np.abs(g - want)) <= 1e-14 * np.max(np.abs(want)), (name, cn, g, want)
    # the mixed regime: the active side carries the same numbers, the inactive side zero amplitudes and a finite rate
    if prog[0]["kind"] == "sho" and len(prog) == 1:
        mixed = [dict(prog[0], regime="mixed")]
        m = R.coefficients(mixed, np.array(P))
        side = (0, 1) if prog[0]["regime"] == "over" else (2, 3, 4, 5)
        for k in range(6):
            if k in side:
                assert np.array_equal(m[k], got[k])
        other = (2, 3, 5) if prog[0]["regime"] == "over" else (0,)
        for k in other:
            assert np.all(m[k] == 0.0)
        assert np.all(np.isfinite(m[1])) and np.all(np.isfinite(m[4])) and np.all(m[1] > 0) and np.all(m[4] > 0)


def jacobian_check(prog, P, rng, tol=1e-12):
    """bP of the hand-written reverse for random cotangents vs the complex-step gradient of sum(cot * coefficients),
    series by series; relative to the largest entry of each series' exact gradient."""
    P = np.asarray(P, dtype=np.float64)
    co = R.coefficients(prog, P)
    cots = R.zero_inactive_rate_cotangents(prog, P, [rng.standard_normal(c.shape) for c in co])
    got = R.coefficients_rev(prog, P, cots)

    def f(Pc):   # Pc (k, B, NP): every series perturbed in the same column at once (the series are independent)
        return sum(np.sum(g * c, axis=-1) for g, c in zip(cots, R.coefficients(prog, Pc)))

    want = np.empty_like(P)
    for k in range(P.shape[1]):
        d = np.zeros(P.shape[1]); d[k] = 1.0
        want[:, k] = np.imag(f(P + 1j * exact.H * d)) / exact.H
    scale = np.max(np.abs(want), axis=1, keepdims=True)
    err = np.max(np.abs(got - want) / scale)
    assert err <= tol, err
    return got, want


SHO_PARS = [0, S, RH, TA, S | RH, S | TA, RH | TA, S | RH | TA]


@pytest.mark.parametrize("regime", ["under", "over", "mixed"])
@pytest.mark.parametrize("par", SHO_PARS)
def test_reverse_sho(par, regime):
    rng = np.random.default_rng(1000 + 10 * par + len(regime))
    prog, P = R.draw("sho", rng, 256, par=par, regime=regime)
    jacobian_check(prog, P, rng)


@pytest.mark.parametrize("kind", ["real", "complex", "matern32", "rotation"])
def test_reverse_other_kinds(kind):
    rng = np.random.default_rng(77 + len(kind))
    prog, P = R.draw(kind, rng, 256)
    jacobian_check(prog, P, rng)


def test_reverse_sum_with_shared_columns():
    """SHO + Real + Matern32 in one program, and two terms reading the SAME column (contributions add)."""
    rng = np.random.default_rng(5)
    n = 200
    p_sho, P_sho = R.draw("sho", rng, n, par=S | RH | TA, regime="mixed")
    _, P_r = R.draw("real", rng, n)
    _, P_m = R.draw("matern32", rng, n)
    prog = [p_sho[0], R.rec("real", (3, 4)), R.rec("matern32", (5, 6))]
    jacobian_check(prog, np.concatenate([P_sho, P_r, P_m], axis=1), rng)
    prog = [R.rec("matern32", (0, 1)), R.rec("matern32", (0, 2)), R.rec("real", (0, 1))]
    jacobian_check(prog, np.stack([rng.uniform(0.3, 2, n), rng.uniform(0.5, 5, n), rng.uniform(0.5, 5, n)], 1), rng)


@pytest.mark.parametrize("name", ["sho_near_half_lo", "sho_near_half_hi"])
def test_reverse_clamped_branch_has_no_derivative_through_f(name):
    """Q = 1/2 -+ 1e-9: max(., eps) clamps, f = sqrt(eps) is a constant, and the reverse must say so exactly."""
    prog, P = GOLDEN_CASES[name]
    P = np.array([P])
    rng = np.random.default_rng(3)
    got, want = jacobian_check(prog, P, rng)
    # the same cotangents on a program whose f is a constant by construction (eps so large that it always clamps) at the
    # same f: identical bits -- nothing flows through f
    co = R.coefficients(prog, P)
    cots = [np.ones(c.shape) for c in co]
    a = R.coefficients_rev(prog, P, cots)
    S0, w0, Q = P[0]
    if prog[0]["regime"] == "under":   # bQ = ba S0 w0 - bc c / Q with f = sqrt(eps)
        f = np.sqrt(1e-5)
        bQ = (1 + 1 / f) * S0 * w0 - (1 + f) * (0.5 * w0 / Q) / Q
    else:
        f = np.sqrt(1e-5)
        bQ = ((1 + 1 / f) + (1 - 1 / f)) * 0.5 * S0 * w0 - ((1 - f) + (1 + f)) * (0.5 * w0 / Q) / Q
    assert abs(a[0, 2] - bQ) <= 1e-15 * abs(bQ)


def test_draws_keep_their_distance_from_one_half():
    rng = np.random.default_rng(0)
    for side in ("under", "over", "mixed"):
        Q = R.draw_Q(rng, 4096, side)
        assert np.min(np.abs(4 * Q**2 - 1)) >= 0.05
    Q = R.draw_Q(rng, 4096, "mixed")
    assert np.sum(Q < 0.5) == 2048


# ---- the host side of the device path: programs are built, and refused, without a GPU ------------------------------------
def test_kernel_with_tensor_parameters_builds_its_program_once():
    import torch
    from celerite2_amd import terms as T

    t = lambda v: torch.tensor(v, dtype=torch.float64)
    Qb = torch.tensor([0.3, 2.0, 0.4], dtype=torch.float64)
    k = (T.SHOTerm(sigma=t(1.5), rho=t(3.0), tau=Qb, regime="mixed") + T.RealTerm(a=1.0, c=t(0.1))
         + T.RotationTerm(sigma=t(1.5), period=t(3.45), Q0=t(1.3), dQ=t(1.05), f=t(0.5)) + T.SHOTerm(S0=1.0, w0=2.0, Q=0.2))
    prog = k.program
    assert prog is k.program
    recs = prog.records
    assert [r["kind"] for r in recs] == ["sho", "real", "rotation", "sho"]
    assert [(r["jr"], r["jc"]) for r in recs] == [(0, 0), (2, 1), (3, 1), (3, 3)]     # slot widths (2, 1), (1, 0), (0, 2), (2, 0), running sums
    assert recs[0]["par"] == R.SIGMA | R.RHO | R.TAU and recs[0]["regime"] == "mixed" and recs[3]["regime"] == "over"
    assert (prog.Jr, prog.Jc, k.width, prog.NP) == (5, 3, 11, 13)
    P = k.parameter_matrix()
    assert tuple(P.shape) == (3, 13) and torch.equal(P[:, 2], Qb) and float(P[1, 3]) == 1.0
    # the restatement reads the same records
    co = R.coefficients(recs, P.numpy())
    assert co[0].shape == (3, 5) and co[2].shape == (3, 3)
    # every parameter shared: P is (NP,)
    assert tuple(T.Matern32Term(sigma=t(0.5), rho=2.0).parameter_matrix().shape) == (2,)
    with pytest.raises(TypeError, match="tensor parameters"):
        k.get_coefficients()
    with pytest.raises(ValueError, match="regime"):
        T.SHOTerm(S0=1.0, w0=1.0, Q=t(1.0))
    with pytest.raises(ValueError, match="regime"):
        T.SHOTerm(sigma=1.0, rho=t(1.0), tau=2.0)        # Q derives from a tensor
    assert T.SHOTerm(S0=t(1.0), w0=1.0, Q=0.2).regime == "over" and T.SHOTerm(S0=t(1.0), rho=2.0, tau=3.0).regime == "under"
    wide = T.RealTerm(a=t(1.0), c=1.0)
    for _ in range(11):
        wide = wide + T.SHOTerm(S0=1.0, w0=1.0, Q=t(1.0), regime="mixed")
    with pytest.raises(ValueError, match="width"):
        wide.program                                         # 1 + 11 * 4 = 45 > 32
    # floats only: the host path, untouched
    kf = T.SHOTerm(S0=5.0, w0=0.1, Q=3.45) + T.RealTerm(a=1.0, c=0.1)
    assert not kf._has_tensors() and kf.width == 3 and kf.get_coefficients()[2].shape == (1,)


def test_entry_points_refuse_bad_programs_before_touching_the_device():
    import ctypes

    from celerite2_amd import _lib, build, ops

    build.build_all()
    lib = _lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)      # never dereferenced: every call below is rejected first
    prog = ops.TermProgram([dict(kind="sho", cols=(0, 1, 2), regime="mixed"), dict(kind="real", cols=(0, 1))], 3)
    call = lambda c, B=i64(4), P=one, bs=i64(3): lib.c2_term_coefficients(ctypes.byref(c), B, P, bs, one, one, one, one, one, one, one, null)
    assert call(prog._c, P=null) == _lib.C2_ERR_INVALID and call(prog._c, B=i64(0)) == _lib.C2_ERR_INVALID
    assert call(prog._c, bs=i64(2)) == _lib.C2_ERR_INVALID          # p_bs is NP or 0
    for field, value in (("nterms", 0), ("nterms", 17), ("Jr", 2), ("np", 2)):
        bad = ops._TermProgram.from_buffer_copy(prog._c)
        setattr(bad, field, value)
        assert call(bad) == _lib.C2_ERR_INVALID, field
    bad = ops._TermProgram.from_buffer_copy(prog._c)
    bad.term[1].jr = 1                                               # a slot that does not follow program order
    assert call(bad) == _lib.C2_ERR_INVALID
    bad = ops._TermProgram.from_buffer_copy(prog._c)
    bad.term[0].regime = 3
    assert call(bad) == _lib.C2_ERR_INVALID
    assert lib.c2_noise_mean_apply(i64(2), i64(0), one, 1, null, null, one, one, one, null) == _lib.C2_ERR_INVALID
    assert lib.c2_noise_mean_rev(i64(2), i64(3), null, one, one, null, null, null, null) == _lib.C2_ERR_INVALID
    with pytest.raises(ValueError, match="regime"):
        ops.TermProgram([dict(kind="sho", cols=(0, 1, 2))], 3)
    with pytest.raises(ValueError, match="parameter columns"):
        ops.TermProgram([dict(kind="real", cols=(0, 3))], 3)
