# -*- coding: utf-8 -*-
"""Every public entry point stands beyond 65535 series somewhere: each name of ops.__all__ and every op and C symbol of every
record of _lib.HEADERS is in exactly one of large_batch_cases.ROWS (run by tests/test_gpu_large_batch.py at B = 70000),
COVERED_ELSEWHERE (an existing test that runs it there) and NO_BATCH_AXIS.  An entry point added later fails here, on the
CPU, until it has its case.

Every row's builder and host reference also run here on the seven distinct series: the inputs are valid and the references
finite without a GPU, and in a `fail` row the chosen series, and only that one, fails in the oracle."""
import ast
import os

import numpy as np
import pytest

import large_batch_cases as L

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def built():
    from celerite2_amd import build

    build.build_all()
    return build


def public_names():
    from celerite2_amd import _lib, ops

    names = list(ops.__all__)
    for record in _lib.HEADERS.values():
        names += (record.ops or []) + record.symbols
    return names


def test_every_entry_point_has_a_case_beyond_65535(built):
    names = public_names()
    assert len(names) == len(set(names))
    places = (L.table_names(), set(L.COVERED_ELSEWHERE), set(L.NO_BATCH_AXIS))
    for name in names:
        where = [name in p for p in places]
        assert sum(where) == 1, "%r is in %d of ROWS / COVERED_ELSEWHERE / NO_BATCH_AXIS (exactly one wanted)" % (name, sum(where))
    extra = (places[0] | places[1] | places[2]) - set(names)
    assert not extra, sorted(extra)   # (nothing is listed that the table does not name)
    for name, reason in L.NO_BATCH_AXIS.items():
        assert reason.strip(), name


def test_covered_elsewhere_names_existing_tests(built):
    for name, where in L.COVERED_ELSEWHERE.items():
        fname, _, test = where.partition("::")
        tree = ast.parse(open(os.path.join(HERE, fname)).read())
        fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
        assert test in fns, (name, where)
        # a batch beyond 65535 stands in the test's body or in its parametrize decorator: some integer literal above it
        nodes = list(ast.walk(fns[test])) + [n for d in fns[test].decorator_list for n in ast.walk(d)]
        ints = [n.value for n in nodes if isinstance(n, ast.Constant) and type(n.value) is int]
        assert any(v > 65535 for v in ints), (name, where)


def test_rows_with_a_plan_run_the_mapping_they_name(built):
    """The launchers' plans are host functions: the kernel family each such row stands on is known here already."""
    raw = L.plan_hooks()
    for row in L.ROWS:
        if row.plan:
            assert L.mapping_of(raw, row, row.build()) == row.plan[1], (row.id, row.plan)


def test_row_ids_are_unique_and_say_their_rule():
    ids = [r.id for r in L.ROWS]
    assert len(ids) == len(set(ids))
    for r in L.ROWS:
        assert r.bits is None or r.bits.strip()
        assert set(r.where_ref) <= set(r.crit)


@pytest.mark.parametrize("row", L.ROWS, ids=[r.id for r in L.ROWS])
def test_row_inputs_and_reference_on_the_host(oracle, row):
    inp = row.build()
    want = row.ref(oracle, inp)
    keep = row.keep
    for k, v in inp.items():
        if not k.startswith("_"):
            assert isinstance(v, np.ndarray) and v.shape[0] == L.D, (row.id, k)
            assert np.all(np.isfinite(v)), (row.id, k)
    flag = want.pop("flag", None)
    if flag is not None:
        bad = np.flatnonzero(np.asarray(flag) != 0).tolist()
        assert bad == ([L.FAIL] if row.fail else []), (row.id, bad)
    else:
        assert not row.fail, row.id
    assert set(want) <= set(row.crit), (row.id, sorted(set(want) - set(row.crit)))
    for name, xo in want.items():
        assert xo.shape[0] == L.D, (row.id, name)
        fin = np.isfinite(xo[keep])
        if name in row.where_ref or row.ragged:    # (rows beyond a ragged count: NaN = never written)
            assert fin.any() or not xo[keep].size, (row.id, name)
        else:
            assert fin.all(), (row.id, name)
        allowed = row.crit[name](xo, keep, inp)
        assert allowed.shape == xo.shape and np.all(allowed[keep][fin] >= 0), (row.id, name)
