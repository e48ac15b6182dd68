# -*- coding: utf-8 -*-
"""CPU checks of the inverse-diagonal feature: the numpy restatement of the recurrence (tests/inverse_diag_ref.py, what the
GPU tests compare the kernels with) against np.linalg.inv of the dense matrix, the three identities built on it (variance
at the data, conditional mean, leave-one-out), and the argument validation of c2_inverse_diag.

Criterion everywhere: the standing one of the GPU parity tests, |x - x_o| <= 1e-10 |x_o| + 1e-12 max |x_o| (the floor of
the variance relative to max(k(0), max D)).  Every input has a condition number <= 1e6, asserted per draw."""
import ctypes

import numpy as np
import pytest

import inverse_diag_ref as R

GOLDEN_SETS = ["cpp_real_", "cpp_complex_", "cpp_sho1_", "cpp_sho2_", "cpp_sum1_", "cpp_sum2_", "cpp_sum3_", "cpp_sum4_", "py_"]
# (seed, N, J, gap in time, noise range in units of k(0))
DRAWS = [(1, 1, 1, False, (0.05, 0.5)), (2, 1, 8, False, (0.05, 0.5)), (3, 2, 2, False, (0.05, 0.5)),
         (4, 2, 4, False, (0.05, 0.5)), (5, 33, 1, False, (0.05, 0.5)), (6, 33, 2, False, (0.05, 0.5)),
         (7, 33, 4, False, (0.05, 0.5)), (8, 33, 8, True, (0.05, 0.5)), (9, 150, 4, False, (0.05, 0.5)),
         (10, 150, 8, False, (0.05, 0.5)), (11, 150, 8, True, (1e-3, 10.0)), (12, 33, 2, False, (1e-4, 1e-3)),
         (13, 150, 4, False, (1e-3, 1e-2))]


def _golden_case(golden, pre):
    g = {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}
    case = dict(t=g["x"], c=g["c"], a=g["a"], U=g["U"], V=g["V"], diag=g["diag"], K=g["K"])
    case["y"] = g["Y"][:, 0]
    return case


def _cases(golden):
    out = [(pre, _golden_case(golden, pre)) for pre in GOLDEN_SETS]
    for seed, N, J, gap, noise in DRAWS:
        case = R.draw(seed, N, J, gap=gap, noise=noise)
        case["K"] = R.dense(case["t"], case["c"], case["a"], case["U"], case["V"])
        out.append(("draw%d_N%d_J%d%s" % (seed, N, J, "_gap" if gap else ""), case))
    return out


@pytest.fixture(scope="module")
def cases(golden):
    out = _cases(golden)
    for name, case in out:
        cond = np.linalg.cond(case["K"])
        assert cond <= 1e6, (name, cond)   # a bad draw fails here instead of loosening anything below
        assert np.allclose(np.diag(case["K"]), case["a"], rtol=1e-14), name   # K carries the white noise
        case["d"], case["W"] = R.factor(case["t"], case["c"], case["a"], case["U"], case["V"])
    return out


def test_restatement_dense_matches_reference_K(golden):
    """R.dense (used for the seeded draws) reproduces the reference's own dense K from its matrices."""
    for pre in GOLDEN_SETS:
        case = _golden_case(golden, pre)
        K = R.dense(case["t"], case["c"], case["a"], case["U"], case["V"])
        assert R.err(K, case["K"]) <= 1.0, pre


def test_recurrence_vs_dense_inverse(cases):
    worst = 0.0
    for name, case in cases:
        q = R.inverse_diag(case["t"], case["c"], case["U"], case["W"], case["d"])
        e = R.err(q, np.diag(np.linalg.inv(case["K"])))
        worst = max(worst, e)
        assert e <= 1.0, (name, e)
        assert np.all(q <= 1.0 / case["diag"] * (1 + 1e-12)), name   # q_n <= 1 / D_n
    print("worst q error / criterion: %.3g" % worst)


def test_fused_alpha_vs_dense_solve(cases):
    for name, case in cases:
        z = R.solve_lower(case["t"], case["c"], case["U"], case["W"], case["y"])
        q, alpha = R.inverse_diag(case["t"], case["c"], case["U"], case["W"], case["d"], z=z)
        assert R.err(alpha, np.linalg.solve(case["K"], case["y"])) <= 1.0, name
        assert np.array_equal(q, R.inverse_diag(case["t"], case["c"], case["U"], case["W"], case["d"])), name


def test_variance_and_mean_identities(cases):
    """var_n = D_n - D_n^2 q_n against k(0) - diag(K^T (K + D)^-1 K), and the mean y - D alpha against K alpha."""
    for name, case in cases:
        D, Kfull = case["diag"], case["K"]
        K = Kfull - np.diag(D)
        z = R.solve_lower(case["t"], case["c"], case["U"], case["W"], case["y"])
        q, alpha = R.inverse_diag(case["t"], case["c"], case["U"], case["W"], case["d"], z=z)
        k0 = np.diag(K)
        var_o = k0 - np.einsum("nm,nm->m", K, np.linalg.solve(Kfull, K))
        floor = max(float(np.max(k0)), float(np.max(D)))
        assert R.err(D - D * D * q, var_o, floor) <= 1.0, (name, R.err(D - D * D * q, var_o, floor))
        mu_o = K @ np.linalg.solve(Kfull, case["y"])
        assert R.err(case["y"] - D * alpha, mu_o) <= 1.0, (name, R.err(case["y"] - D * alpha, mu_o))


def test_leave_one_out_vs_deleting_the_point(cases):
    """mu_-n = y_n - alpha_n / q_n, sigma^2_-n = 1 / q_n against conditioning with row and column n deleted (N <= 33)."""
    done = 0
    for name, case in cases:
        N = len(case["t"])
        if N > 33:
            continue
        z = R.solve_lower(case["t"], case["c"], case["U"], case["W"], case["y"])
        q, alpha = R.inverse_diag(case["t"], case["c"], case["U"], case["W"], case["d"], z=z)
        ref = np.array([R.delete_one(case["K"], case["y"], n) for n in range(N)])
        assert R.err(1.0 / q, ref[:, 1]) <= 1.0, name
        e = R.err(case["y"] - alpha / q, ref[:, 0], R.mean_floor(ref[:, 0], case["y"]))
        assert e <= 1.0, (name, e)
        done += 1
    assert done >= 8


def test_abi_argument_errors():
    """c2_inverse_diag rejects null pointers / non-positive sizes (C2_ERR_INVALID) and widths above C2_MAX_WIDTH
    (C2_ERR_UNSUPPORTED) before anything touches the device."""
    from celerite2_amd import _lib, build

    build.build_all()
    assert "c2_inverse_diag" in _lib.HEADERS["main"].symbols
    lib = _lib.load()
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)   # a non-null address that is never dereferenced: the checks come first

    def call(B, N, J, t=null, c=null, U=null, W=null, d=null, z=null, q=null, alpha=null):
        return lib.c2_inverse_diag(i64(B), i64(N), i64(J), t, i64(0), c, i64(0), U, W, d, z, q, alpha, null)

    assert call(1, 4, 2) == _lib.C2_ERR_INVALID
    assert call(0, 4, 2, one, one, one, one, one, null, one, null) == _lib.C2_ERR_INVALID
    assert call(1, 0, 2, one, one, one, one, one, null, one, null) == _lib.C2_ERR_INVALID
    assert call(1, 4, 0, one, one, one, one, one, null, one, null) == _lib.C2_ERR_INVALID
    assert call(1, 4, 2, one, one, one, one, one, one, one, null) == _lib.C2_ERR_INVALID    # z without alpha
    assert call(1, 4, 2, one, one, one, one, one, null, one, one) == _lib.C2_ERR_INVALID    # alpha without z
    assert call(1, 4, 2, one, one, one, one, one, null, null, null) == _lib.C2_ERR_INVALID  # no q
    assert call(1, 4, 129) == _lib.C2_ERR_UNSUPPORTED
    assert call(1, 4, 129, one, one, one, one, one, null, one, null) == _lib.C2_ERR_UNSUPPORTED
