# -*- coding: utf-8 -*-
"""What the float64 oracle (oracle/cpu.py, the restatement of the reference) does with non-finite inputs -- the reference
of tests/test_gpu_nonfinite.py, pinned on the CPU so that it is under test itself: a NaN or an infinity raises no flag
(`d <= 0` is false for NaN), the poisoned series' log-likelihood is NaN, the recursions are causal (rows before the poison
of a lower form / after it of an upper form, and every other right-hand side, stay finite), and every other series of the
batch is bit-identical to the clean draw.  -inf on the diagonal is the one poison that fails the pivot test."""
import numpy as np
import pytest

import nonfinite_cases as NF
import parity_cases as P

B, N, J, SERIES, ROW = 6, 40, 4, 2, 17
NO_FLAG_KINDS = ("y_nan", "y_inf", "a_nan", "a_pinf", "U_nan", "series_nan")


@pytest.fixture(scope="module")
def clean(oracle):
    case = NF.as_case(P.problem(None, B, N, J))
    return case, NF.expect(oracle, case, "loglik_grad")


def test_poison_copies_and_never_touches_the_grid():
    case = NF.as_case(P.problem(None, B, N, J))
    before = {k: getattr(case, k).copy() for k in ("t", "c", "a", "U", "V", "y")}
    for kind in NF.LOGLIK_KINDS:
        bad = NF.poison(case, kind, SERIES, ROW)
        for k, v in before.items():
            assert np.array_equal(getattr(case, k), v)            # the draw itself is unchanged
        assert np.array_equal(bad.t, case.t) and np.array_equal(bad.c, case.c)
        changed = [k for k in ("a", "U", "V", "y") if not np.array_equal(getattr(bad, k), getattr(case, k), equal_nan=True)]
        assert changed and all(np.array_equal(getattr(bad, k)[NF.others(B, SERIES)], getattr(case, k)[NF.others(B, SERIES)])
                               for k in changed)
    with pytest.raises(ValueError):
        NF.poison(case, "t_nan", 0, 0)


@pytest.mark.parametrize("kind", NO_FLAG_KINDS)
def test_nan_raises_no_flag_and_stays_in_its_series(oracle, clean, kind):
    case, ref = clean
    got = NF.expect(oracle, NF.poison(case, kind, SERIES, ROW), "loglik_grad")
    assert got.flag.tolist() == [0] * B
    assert np.isnan(got.values["ll"][SERIES])
    assert not all(np.isfinite(got.values[g][SERIES]).all() for g in NF.GRAD_NAMES)
    keep = NF.others(B, SERIES)
    for name, v in got.values.items():
        assert np.array_equal(v[keep], ref.values[name][keep]), name      # bit-identical to the clean draw
        assert not got.nonfinite[name][keep].any()


def test_minus_inf_on_the_diagonal_fails_the_pivot_test(oracle, clean):
    case, ref = clean
    got = NF.expect(oracle, NF.poison(case, "a_ninf", SERIES, ROW), "loglik_grad")
    want = [0] * B; want[SERIES] = ROW
    assert got.flag.tolist() == want                                       # d = -inf <= 0: the flag is the poison row
    assert np.isneginf(got.values["ll"][SERIES])
    assert all(np.isnan(got.values[g][SERIES]).all() for g in NF.GRAD_NAMES)   # celerite2_amd.h: all six NaN
    keep = NF.others(B, SERIES)
    for name, v in got.values.items():
        assert np.array_equal(v[keep], ref.values[name][keep]), name


def test_factor_is_causal(oracle):
    case = P.factor_case(oracle, B, N, J)
    for kind in ("a_nan", "U_nan", "V_nan"):
        got = NF.expect(oracle, NF.poison(case, kind, SERIES, ROW), "factor")
        assert got.flag.tolist() == [0] * B
        d, W, S = (got.values[k] for k in ("d", "W", "S"))
        assert np.array_equal(d[SERIES, :ROW], case.d[SERIES, :ROW]) and np.array_equal(W[SERIES, :ROW], case.W[SERIES, :ROW])
        assert np.array_equal(S[SERIES, :ROW], case.S[SERIES, :ROW])
        first = ROW if kind != "V_nan" else ROW + 1                        # (V_n enters d only through W_n, one row on)
        assert not np.isfinite(d[SERIES, first:]).any()
        keep = NF.others(B, SERIES)
        assert np.array_equal(d[keep], case.d[keep]) and np.array_equal(W[keep], case.W[keep]) and np.array_equal(S[keep], case.S[keep])
    got = NF.expect(oracle, NF.poison(case, "a_ninf", SERIES, ROW), "factor")
    assert got.flag[SERIES] == ROW and np.isneginf(got.values["d"][SERIES, ROW])
    assert got.written["d"][SERIES].sum() == ROW + 1 and got.written["W"][SERIES].sum() == ROW


@pytest.mark.parametrize("name", P.SWEEPS)
def test_sweeps_are_causal_and_columns_independent(oracle, name):
    case = P.sweep_case(oracle, 11, B, N, J, 3)
    got = NF.expect(oracle, NF.poison(case, "Y_nan_col", SERIES, ROW, col=1), "sweep", name)
    Z, F, ref = got.values["Z"], NF.F_by_rhs(got.values["F"]), case.want[name]
    Fref = NF.F_by_rhs(ref.F)
    lower = name.endswith("lower")
    safe = slice(0, ROW) if lower else slice(ROW + 1, N)
    assert np.array_equal(Z[SERIES, safe, 1], ref.Z[SERIES, safe, 1])       # rows before (lower) / after (upper) the poison
    assert np.array_equal(F[SERIES, safe, 1], Fref[SERIES, safe, 1])
    assert np.isnan(Z[SERIES, ROW, 1]) or name.startswith("matmul")         # (the products' row n takes Y_n from later rows only)
    assert got.nonfinite["Z"][SERIES, :, 1].any()
    for col in (0, 2):                                                      # the other right-hand sides: untouched
        assert np.array_equal(Z[SERIES, :, col], ref.Z[SERIES, :, col]) and np.array_equal(F[SERIES, :, col], Fref[SERIES, :, col])
    keep = NF.others(B, SERIES)
    assert np.array_equal(Z[keep], ref.Z[keep]) and np.array_equal(F[keep], Fref[keep])


@pytest.mark.parametrize("name", P.SWEEPS)
@pytest.mark.parametrize("kind", NF.SWEEP_REV_KINDS)
def test_reverse_sweeps_keep_the_other_series(oracle, name, kind):
    case = P.sweep_case(oracle, 12, B, N, J, 3)
    got = NF.expect(oracle, NF.poison(case, kind, SERIES, ROW, col=1), "sweep_rev", name)
    keep = NF.others(B, SERIES)
    assert any(got.nonfinite[k][SERIES].any() for k in NF.REV_NAMES)
    for k, want in zip(NF.REV_NAMES, case.want[name].rev):
        assert np.array_equal(got.values[k][keep], want[keep]), k
    if kind == "bZ_nan":                                                    # columns of the cotangent are independent in bY
        for col in (0, 2):
            assert np.array_equal(got.values["bY"][SERIES, :, col], case.want[name].rev[4][SERIES, :, col])


def test_tables_name_every_kind_and_cite_a_line():
    assert set(NF.LOGLIK_KINDS) | set(NF.SWEEP_REV_KINDS) == set(NF.ALL_KINDS)
    for table in (NF.LOGLIK_PATHS, NF.FACTOR_PATHS):
        for key, (shape, width, opts, twin, decides, loops) in table.items():
            assert twin == "same" or isinstance(twin, dict), key
            assert ".hip:" in decides or ".hpp:" in decides, key
            assert loops == "none", key      # a path with a value-steered loop must not be run poisoned at all
    for key, (shape, width, nrhs, opts, with_F, which, twin) in NF.SWEEP_PATHS.items():
        assert which in ("all", "solve", "matmul") and (twin == "same" or isinstance(twin, tuple)), key
        assert shape is NF.ROWS or shape is NF.LONG, key
    for paths, decides in ((NF.SWEEP_PATHS, NF.SWEEP_DECIDES), (NF.SWEEP_REV_PATHS, NF.SWEEP_REV_DECIDES),
                           (NF.FACTOR_REV_PATHS, NF.FACTOR_REV_DECIDES)):
        assert set(paths) == set(decides)
        for key, (line, loops) in decides.items():
            assert (".hip:" in line or ".hpp:" in line) and loops == "none", key


def test_v_nan_reaches_the_gradients_through_w(oracle, clean):
    """V_n enters d only through W_n: a NaN in V at a middle row makes ll NaN (no flag); at the LAST row W_{N-1} is read by
    no forward recursion, ll stays finite -- and the reference's reverse pass still multiplies 0 by W_{N-1} (reverse.hpp:65),
    so ALL six gradients of that series are NaN.  The device kernels are held to exactly this."""
    case, ref = clean
    keep = NF.others(B, SERIES)
    mid = NF.expect(oracle, NF.poison(case, "V_nan", SERIES, ROW, col=1), "loglik_grad")
    assert mid.flag.tolist() == [0] * B and np.isnan(mid.values["ll"][SERIES])
    last = NF.expect(oracle, NF.poison(case, "V_nan", SERIES, N - 1, col=1), "loglik_grad")
    assert last.flag.tolist() == [0] * B
    assert last.values["ll"][SERIES] == ref.values["ll"][SERIES]                      # finite, and the clean value
    for g in ("bt", "bc", "ba"):
        assert np.isnan(last.values[g][SERIES]).all(), g                              # every element
    assert np.isnan(last.values["bU"][SERIES, 1:]).all()                              # (U of row 0 is read by nothing: 0)
    assert np.isnan(last.values["bV"][SERIES, :-1]).all()                             # (bV of the last row is 0 / d_{N-1} = 0)
    for got in (mid, last):
        for name, v in got.values.items():
            assert np.array_equal(v[keep], ref.values[name][keep]), name
