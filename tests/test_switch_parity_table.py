# -*- coding: utf-8 -*-
"""Every switch of the dispatch table (csrc/c2_dispatch.hpp, read through _lib.options()) has a parity case: it is a key of
test_gpu_switch_parity.SWITCH_CASES (both sides run there), or COVERED_ELSEWHERE names a test file that sets it, or EXEMPT
says why it needs none.  A new switch without one fails here, on the CPU.  Reads the option table and test sources only."""
import os

import pytest

import test_gpu_switch_parity as T

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def built():
    from celerite2_amd import build

    build.build_all()
    return build


def test_every_switch_has_a_parity_case(built):
    from celerite2_amd import _lib

    table = {o["name"]: o for o in _lib.options()}
    switches = {n for n, o in table.items() if o["switch"]}
    places = (set(T.SWITCH_CASES), set(T.COVERED_ELSEWHERE), set(T.EXEMPT))
    for name in sorted(switches):
        where = [name in p for p in places]
        assert sum(where) == 1, "switch %r is in %d of SWITCH_CASES / COVERED_ELSEWHERE / EXEMPT (exactly one wanted)" \
            % (name, sum(where))
    # nothing listed that the table does not have, and nothing listed twice
    listed = places[0] | places[1] | places[2]
    assert listed <= set(table), sorted(listed - set(table))
    assert sum(len(p) for p in places) == len(listed)
    for name, reason in T.EXEMPT.items():
        assert reason.strip()


def test_covered_elsewhere_names_a_file_that_sets_the_switch(built):
    from celerite2_amd import _lib

    table = {o["name"]: o for o in _lib.options()}
    for name, fname in T.COVERED_ELSEWHERE.items():
        text = open(os.path.join(HERE, fname)).read()
        assert '"%s"' % table[name]["env"] in text or '"%s"' % name in text or "'%s'" % name in text, \
            "%s does not name %s / %s" % (fname, name, table[name]["env"])


def test_every_case_has_its_test(built):
    """SWITCH_CASES[option] is run by test_<option> of the GPU file, whose docstring names the dispatch line."""
    for name in T.SWITCH_CASES:
        fn = getattr(T, "test_" + name, None)
        assert fn is not None, name
        assert ".hip:" in (fn.__doc__ or ""), name
