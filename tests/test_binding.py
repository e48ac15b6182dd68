# -*- coding: utf-8 -*-
"""The Python binding takes its prototypes from include/celerite2_amd.h (celerite2_amd/_lib.py): a call that does not fit
its prototype is refused before C is entered, every kind of pointer argument the tests and tools pass still works, the
constants are the header's, and the shape helper of ops.py says what _shape said.  (That every declared symbol is typed:
tests/test_abi.py::test_public_header.)  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from celerite2_amd import _lib, build

    build.build_all()
    return _lib.load()


@pytest.fixture(scope="module")
def header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "celerite2_amd.h")).read(), flags=re.S)


def loglik_args(B=0, J=2, p=None):
    return [B, 4, J, p, 0, p, 0, p, p, p, p, p, p, None]


def test_bad_calls_are_refused_before_c(lib):
    refused = (TypeError, ctypes.ArgumentError)
    with pytest.raises(refused):
        lib.c2_loglik(*loglik_args()[:-1])
    with pytest.raises(refused):
        lib.c2_loglik(*loglik_args(), None)
    with pytest.raises(refused):
        lib.c2_loglik(*loglik_args(B=1.0))
    for text in ("t", b"t"):
        with pytest.raises(refused):
            lib.c2_loglik(*loglik_args(p=text))
    with pytest.raises(refused):   # int zero_z
        lib.c2_matmul_lower(0, 4, 2, 1, None, 0, None, 0, None, None, None, None, None, ctypes.c_int64(1), None)


def test_every_kind_of_pointer_argument(lib):
    """B = 0 and J = 129 are refused before anything is launched (tests/test_abi.py::test_argument_errors_without_gpu)."""
    from celerite2_amd import _lib

    class Tensor:
        def data_ptr(self):
            return keep.ctypes.data

    keep = np.ones(8)
    for p in (None, 0, ctypes.c_void_p(0), keep.ctypes.data_as(ctypes.c_void_p), Tensor()):
        assert lib.c2_loglik(*loglik_args(B=0, p=p)) == _lib.C2_ERR_INVALID
        assert lib.c2_loglik(*loglik_args(B=1, J=129, p=p)) == _lib.C2_ERR_UNSUPPORTED
    dflt = ctypes.c_double()
    assert lib.c2_option_info(0, None, None, ctypes.byref(dflt), None, None, None) == _lib.C2_OK   # byref(...)


def test_constants_are_the_headers(header):
    from celerite2_amd import _lib

    defined = {k: int(v.strip("()")) for k, v in re.findall(r"#define\s+(C2_\w+)\s+(\(?-?\d+\)?)", header)}
    assert _lib.C2_MAX_WIDTH == defined["C2_MAX_WIDTH"] == 128 and _lib.C2_FAST_WIDTH == defined["C2_FAST_WIDTH"] == 32
    for name in ("C2_OK", "C2_ERR_INVALID", "C2_ERR_UNSUPPORTED", "C2_ERR_HIP"):
        assert getattr(_lib, name) == defined[name], name
    assert (_lib.C2_OK, _lib.C2_ERR_INVALID, _lib.C2_ERR_UNSUPPORTED, _lib.C2_ERR_HIP) == (0, -1, -2, -3)


def test_an_unknown_type_fails_loudly():
    from celerite2_amd import _lib

    with pytest.raises(_lib.BackendError, match=r"c2_new_thing.*'const float \*'"):
        _lib._prototypes("int c2_new_thing(int64_t B, const float *x);")


def test_shape_specs_on_cpu_tensors():
    import torch
    from celerite2_amd import ops

    dims = dict(B=2, N=5, M=3, J=2, K=4)
    for spec in ("N|BN", "J|BJ", "BN", "BNJ", "BMJ", "BNJJ", "BNK", "B"):
        forms = [tuple(dims[k] for k in form) for form in spec.split("|")]
        expected = " or ".join(str(f) for f in forms)
        for form in forms:
            ops._shapes(dims, [("x", torch.zeros(form), spec), ("none", None, spec)])
            for k in range(len(form)):
                for step in (1, -1):
                    bad = form[:k] + (form[k] + step,) + form[k + 1:]
                    if bad in forms:
                        continue
                    with pytest.raises(ValueError) as e:
                        ops._shapes(dims, [("x", torch.zeros(bad), spec)])
                    assert str(e.value) == "Invalid shape: x (got %s, expected %s)" % (bad, expected)
    with pytest.raises(ValueError, match=r"^Invalid shape: first \(got \(6,\), expected \(5,\) or \(2, 5\)\)$"):
        ops._shapes(dims, [("ok", torch.zeros(2, 5, 2), "BNJ"), ("first", torch.zeros(6), "N|BN"), ("second", torch.zeros(9), "BN")])
