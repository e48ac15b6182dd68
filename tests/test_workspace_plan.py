# -*- coding: utf-8 -*-
"""The plans of the fused log-likelihood entry points (csrc/c2_plan.hpp; lane_mapping / grad_layout of c2_loglik.hip,
terms_mapping / terms_layout of c2_terms.hip).  Host functions only: no device is needed.

1. The workspace queries return what they returned before the dispatchers and the queries were derived from one plan
   (tests/golden/workspace_sizes.npz, recorded by tests/golden/make_workspace_sizes.py on the commit before).
2. Whatever mapping the dispatcher takes for a call -- either alignment of its arrays, with and without the time-parallel
   form, at default options, under every forced mapping and with thresholds set so that the ranges of two mappings
   overlap -- ends inside the size the matching query reports."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_workspace_sizes as golden  # noqa: E402

OVERLAPS = [("lanes1_min_batch_grad", 12000), ("lanes4_max_batch_grad", 20000), ("lanes2_min_batch_grad", 12000)]
TERMS_FORCED = [("terms_four_lanes", 1), ("terms_eight_lanes", 1), ("terms_two_lanes", 1), ("terms_fused", 1), ("terms_fused", 0)]
MAPPINGS = {1: "one", 2: "two", 4: "four", 8: "group", 9: "replay", 10: "timepar", 12: "wide", 13: "composed"}   # c2::Lanes


@pytest.fixture(scope="module")
def raw():
    from celerite2_amd import build

    build.build_all()
    lib = golden.queries()
    i64, out = ctypes.c_int64, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
    lib.c2_internal_loglik_grad_plan.restype, lib.c2_internal_loglik_grad_plan.argtypes = ctypes.c_int, [i64] * 3 + [ctypes.c_int] * 2 + out
    lib.c2_internal_loglik_terms_plan.restype, lib.c2_internal_loglik_terms_plan.argtypes = ctypes.c_int, [i64] * 4 + [ctypes.c_int] + out
    return lib


@pytest.fixture
def option():
    """set(name, value) for the length of one test"""
    from celerite2_amd import _lib

    touched = []

    def set_(name, value):
        touched.append(name)
        _lib.set_option(name, value)

    yield set_
    for name in touched:
        _lib.set_option(name, None)


def test_sizes_are_those_of_the_commit_before(raw, option):
    want = np.load(golden.OUT)
    assert [list(want[k]) for k in "BNJ"] == [golden.GRID_B, golden.GRID_N, golden.GRID_J]
    assert want["splits"].tolist() == [list(s) for s in golden.SPLITS]
    assert list(want["settings"]) == [golden.setting_name(s) for s in golden.SETTINGS]
    for s in golden.SETTINGS:
        if s is not None:
            option(*s)
        for name, got in golden.record(raw).items():
            key = "%s/%s" % (name, golden.setting_name(s))
            bad = np.argwhere(got != want[key])
            assert bad.size == 0, (key, bad[:5].tolist(), got[tuple(bad[0])], want[key][tuple(bad[0])])
        if s is not None:
            option(s[0], None)
    assert want["grad/default"].min() > 0 and want["rows/default"].min() > 0


def plan_fits(raw):
    """every (shape, alignment, allow_timepar): the mapping's need against the matching query; returns the mappings seen"""
    m, need = ctypes.c_int(), ctypes.c_size_t()
    seen = set()
    for B in golden.GRID_B:
        for N in golden.GRID_N:
            for J in golden.GRID_J:
                public = raw.c2_loglik_grad_workspace_bytes(B, N, J)
                rows = raw.c2_internal_loglik_grad_rows_workspace_bytes(B, N, J)
                assert rows >= public > 0, (B, N, J)
                for allow_timepar in (0, 1):
                    for aligned16 in (0, 1):
                        assert raw.c2_internal_loglik_grad_plan(B, N, J, allow_timepar, aligned16, ctypes.byref(m), ctypes.byref(need)) == 0
                        assert m.value in MAPPINGS and need.value > 0, (B, N, J, m.value)
                        assert need.value * 8 <= (public if allow_timepar else rows), (B, N, J, allow_timepar, aligned16, MAPPINGS[m.value])
                        assert allow_timepar or m.value != 10
                        assert aligned16 or m.value != 4
                        seen.add(MAPPINGS[m.value])
            for Jr, Jc in golden.SPLITS:
                for grad in (0, 1):
                    assert raw.c2_internal_loglik_terms_plan(B, N, Jr, Jc, grad, ctypes.byref(m), ctypes.byref(need)) == 0
                    assert need.value * 8 <= raw.c2_loglik_terms_workspace_bytes(B, N, Jr, Jc, grad), (B, N, Jr, Jc, grad, MAPPINGS[m.value])
                    seen.add("terms " + MAPPINGS[m.value])
    return seen


def test_the_plan_fits_its_own_size_at_default_options(raw):
    seen = plan_fits(raw)
    assert seen >= {"one", "two", "four", "group", "replay", "timepar", "wide", "terms four", "terms group", "terms two", "terms one",
                    "terms composed"}, seen


@pytest.mark.parametrize("name,value", [s for s in golden.SETTINGS if s is not None] + OVERLAPS + TERMS_FORCED)
def test_the_plan_fits_its_own_size_under(raw, option, name, value):
    option(name, value)
    seen = plan_fits(raw)
    if name == "lanes" and value != 8:
        assert MAPPINGS[value] in seen, seen
    if name == "timepar_grad":
        assert ("timepar" in seen) == bool(value), seen
    if name == "loglik_back":
        assert "group" not in seen and "replay" in seen, seen


def test_the_cases_worked_by_hand(raw, option):
    """Thresholds set so that two ranges overlap: the dispatcher's precedence decides (four lanes before two before one),
    and the size holds the mapping that runs AND the one arrays off a 16-byte boundary take instead."""
    m, need = ctypes.c_int(), ctypes.c_size_t()
    option("lanes1_min_batch_grad", 12000)
    assert raw.c2_loglik_grad_workspace_bytes(14000, 64, 8) // 8 == 13574718        # the one-lane size (unaligned arrays)
    raw.c2_internal_loglik_grad_plan(14000, 64, 8, 1, 1, ctypes.byref(m), ctypes.byref(need))
    assert (MAPPINGS[m.value], need.value) == ("four", 11985972)
    raw.c2_internal_loglik_grad_plan(14000, 64, 8, 1, 0, ctypes.byref(m), ctypes.byref(need))
    assert (MAPPINGS[m.value], need.value) == ("one", 13574718)
    option("lanes1_min_batch_grad", None)
    option("lanes4_max_batch_grad", 20000)
    assert raw.c2_loglik_grad_workspace_bytes(18000, 64, 8) // 8 == 17872720        # the two-lane size
    raw.c2_internal_loglik_grad_plan(18000, 64, 8, 1, 1, ctypes.byref(m), ctypes.byref(need))
    assert (MAPPINGS[m.value], need.value) == ("four", 15410534)
