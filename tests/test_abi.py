# -*- coding: utf-8 -*-
"""CPU-side checks of the drop-in boundary: the C-ABI library loads and every public header stands against its record
in celerite2_amd._lib.HEADERS (declared, exported, typed, in the build, its ops), the pybind11 modules expose the
reference's surface (python/celerite2/driver.cpp:482-499, backprop.cpp:906-926) and its argument validation, and the
product path fails loudly (no CPU fallback) when no GPU is present."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from celerite2_amd import build

    build.build_all()
    return build


def _header_keys():
    from celerite2_amd import _lib

    return list(_lib.HEADERS)


@pytest.fixture(scope="module")
def table(built):
    """What holds of _lib.HEADERS as a whole, checked once: (the table, the library as the linker sees it, as load() types it)."""
    import glob

    from celerite2_amd import _lib

    records = list(_lib.HEADERS.values())
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(r.file for r in records) and len(records) == 13
    symbols = [s for r in records for s in r.symbols]
    ops_names = [n for r in records if r.ops is not None for n in r.ops]
    assert len(symbols) == len(set(symbols)) == 88 and len(ops_names) == len(set(ops_names))
    main = [k for k, r in _lib.HEADERS.items() if r.ops is None]
    assert main == ["main"] and len(_lib.HEADERS["main"].symbols) == 68
    sources = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "celerite2_amd", "csrc", "*.hip"))}
    assert sources and sources == set(built.HIP_SOURCES), sources ^ set(built.HIP_SOURCES)
    so = ctypes.CDLL(_lib.LIB_PATH)
    so.c2_version.restype = ctypes.c_char_p
    assert b"gfx950" in so.c2_version()
    return _lib.HEADERS, so, _lib.load()


@pytest.mark.parametrize("key", _header_keys())
def test_public_header(table, built, key):
    """One public header against its record: the prototypes it declares are the record's symbols in order, nothing that looks
    like a c2_ call hides outside a prototype, every symbol is exported and typed from its prototype by load(), the header
    makes the build stale, and the record's ops exist on ops (in ops.__all__ exactly for the main header)."""
    from celerite2_amd import _lib, ops

    headers, so, lib = table
    record, text = headers[key], _lib.header_text(key)
    declared = re.findall(r"([\w \t*]+?)\b(c2h?_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [name for _, name, _ in declared] == list(_lib._prototypes(text)) == record.symbols
    loose = set(re.findall(r"\b(c2h?_[a-z0-9_]+)\s*\(", text))
    assert loose == set(record.symbols), loose ^ set(record.symbols)
    restypes = {"size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p, "void": None, "int64_t": ctypes.c_int64}
    for ret, name, params in declared:
        assert hasattr(so, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert len(fn.argtypes) == (0 if params.strip() == "void" else len(params.split(","))), name
        assert fn.restype is restypes.get(" ".join(ret.split()), ctypes.c_int), name
    assert _lib.header_path(key) in built.HIP_HEADERS
    assert os.path.samefile(_lib.header_path(key), os.path.join(ROOT, "include", record.file))
    for name in ops.__all__ if record.ops is None else record.ops:
        assert callable(getattr(ops, name)), name
        assert (name in ops.__all__) == (record.ops is None), name


def test_gfx950_code_object(built):
    """The shared library must carry a gfx950 code object (hipcc --offload-arch=gfx950)."""
    data = open(built.LIB).read() if False else open(built.LIB, "rb").read()
    assert b"gfx950" in data


def test_argument_errors_without_gpu(built):
    from celerite2_amd import _lib

    lib = _lib.load()
    i64 = ctypes.c_int64
    null = ctypes.c_void_p(0)
    # invalid sizes / null pointers are rejected before anything touches the device
    assert lib.c2_loglik(i64(0), i64(4), i64(2), *([null] * 1), i64(0), null, i64(0), null, null, null, null, null, null,
                         null) == _lib.C2_ERR_INVALID
    assert lib.c2_loglik(i64(1), i64(4), i64(129), null, i64(0), null, i64(0), null, null, null, null, null, null,
                         null) == _lib.C2_ERR_UNSUPPORTED   # beyond C2_MAX_WIDTH = 128 (33 .. 128: csrc/c2_wide.hip)
    # workspace = wave-blocked packed checkpoints (one per segment + the state after the last row) + the W rows (B,N,J)
    # + (d,z) pairs (B,N,2) + one stability word per wavefront, each part padded to 16 bytes  
    B, N, J = 2, 8, 3                      # G = 4, C = 8 -> 1 segment, 1 wavefront
    ck = 1 * (1 + 1) * (64 + 3 * 32 + 64 + 64)   # S slot 0 (64) + slots 1..3 (32 owners each) + F (64) + W (64)
    assert lib.c2_loglik_grad_workspace_bytes(B, N, J) == 8 * (ck + 1 * N * 64 + B * N * 2 + 2)   # W: lane-major per wavefront
    # chip-filling J = 8 batches take the one-lane-per-series path: records W (B,N,8) + (d,z) (B,N,2) + t (B,N) + a
    # checkpoint of 44 doubles every 32 rows and twice as many extra slots (re-anchoring in front of gaps in time) with
    # their row list, overlaid with the replay kernels' workspace, + the guard words (two head words and one per wavefront:
    # a wavefront that runs out of slots sends ITS 64 series to the replay kernels)
    waves, nck = 65536 // 64, 3 * ((4096 - 2) // 32 + 1)
    rec = waves * 64 * (4096 * 8 + 4096 * 2 + 4096 + nck * 44) + waves * (4096 // 2)   # + the slot of every row (int32)
    assert lib.c2_loglik_grad_workspace_bytes(65536, 4096, 8) == 8 * (2 + waves + rec) < 34 * 2**30
    assert lib.c2_loglik_grad_workspace_bytes(65536, 4096, 6) == 8 * (2 + waves + rec)   # width 6 runs as 8: same records
    assert lib.c2_loglik_grad_workspace_bytes(1, 4096, 129) == 0   # unsupported width
    # a wide model (33 .. 128) runs the literal op chain: d, W, S, z, F, bd, bz, bW in the workspace
    assert lib.c2_loglik_grad_workspace_bytes(2, 100, 40) == 8 * 2 * 100 * (1 + 40 + 1600 + 1 + 40 + 1 + 1 + 40)


def test_driver_surface_and_validation(built):
    from celerite2_amd import backprop, driver

    for name in ("factor", "solve_lower", "solve_upper", "matmul_lower", "matmul_upper", "general_matmul_lower",
                 "general_matmul_upper", "get_celerite_matrices", "LinAlgError", "__version__"):
        assert hasattr(driver, name), name
    for name in ("factor_fwd", "factor_rev", "solve_lower_fwd", "solve_lower_rev", "solve_upper_fwd",
                 "solve_upper_rev", "matmul_lower_fwd", "matmul_lower_rev", "matmul_upper_fwd", "matmul_upper_rev",
                 "general_matmul_lower_fwd", "general_matmul_upper_fwd", "LinAlgError"):
        assert hasattr(backprop, name), name
    assert driver.LinAlgError is not backprop.LinAlgError  # separate classes, as upstream
    N, J = 5, 2
    t, c, a = np.zeros(N), np.zeros(J), np.ones(N)
    U, V = np.zeros((N, J)), np.zeros((N, J))
    with pytest.raises(ValueError, match="Invalid shape: a"):
        driver.factor(t, c, np.ones(N + 1), U, V, a, V)
    with pytest.raises(ValueError, match="Invalid shape: W"):
        driver.factor(t, c, a, U, V, a, np.zeros((N, J + 1)))
    with pytest.raises(ValueError, match="Invalid number of dimensions: Y"):
        driver.solve_lower(t, c, U, V, np.zeros(N), np.zeros(N))  # 1-D Y rejected (driver.cpp:89-91)
    with pytest.raises(ValueError, match="Invalid shape: S"):
        backprop.factor_fwd(t, c, a, U, V, a, V, np.zeros((N, J)))
    with pytest.raises(ValueError, match="dimension mismatch: bc"):
        driver.get_celerite_matrices(np.zeros(1), np.zeros(1), np.zeros(2), np.zeros(1), t, a, a, np.zeros((N, 3)),
                                     np.zeros((N, 3)))


def test_fails_loudly_without_gpu(built):
    """No silent CPU fallback: without a HIP device the product raises."""
    from celerite2_amd import _lib, driver

    if _lib.load().c2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    N, J = 5, 2
    t = np.arange(N, dtype=float)
    with pytest.raises(RuntimeError, match=r"HIP error[^:]*: \S"):   # (the text of the HIP error behind the colon, not the colon alone)
        driver.factor(t, np.ones(J), np.ones(N), np.zeros((N, J)), np.zeros((N, J)), np.ones(N), np.zeros((N, J)))


def test_views_of_one_array_pass_argument_bookkeeping(built):
    """Arguments that are views of ONE array and start at its first element share a host address and differ in length
    (conditioning on x, predicting at x[:k]; coefficient arrays cut from one vector).  The reference takes such calls, so
    the staging layer must: without a device each of them gets as far as the device (RuntimeError naming the HIP error),
    not ValueError -- whichever of the two comes first, and for a tail view, which has an address of its own."""
    from celerite2_amd import _lib, backprop, driver

    if _lib.load().c2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    hip = dict(match=r"HIP error[^:]*: \S")
    n, k, J, nrhs = 10, 4, 2, 1
    x = np.linspace(0, 1, n)
    c = np.ones(J)
    for t1, t2 in ((x[:k], x), (x, x[:k]), (x[n - k:], x), (x, x[n - k:]), (x[::1], x)):
        assert t1.flags.c_contiguous and t2.flags.c_contiguous
        N, M = len(t1), len(t2)
        U, V, Y = np.ones((N, J)), np.ones((M, J)), np.ones((M, nrhs))
        for lower in ("general_matmul_lower", "general_matmul_upper"):
            with pytest.raises(RuntimeError, **hip):
                getattr(driver, lower)(t1, t2, c, U, V, Y, np.zeros((N, nrhs)))
            with pytest.raises(RuntimeError, **hip):
                getattr(backprop, lower + "_fwd")(t1, t2, c, U, V, Y, np.zeros((N, nrhs)), np.zeros((M, J, nrhs)))
    co = np.linspace(0.1, 1.0, 8)
    N = 5
    for Jr, Jc in ((1, 3), (3, 1), (2, 2)):
        Jw = Jr + 2 * Jc
        for ar, ac, bc, dc in ((co[:Jr], co[:Jc], co[:Jc], co[:Jc]),                    # all four from the front
                               (co[:Jr], co[Jr:Jr + Jc], co[:Jc], co[Jr:Jr + Jc]),      # front and middle, mixed
                               (co[8 - Jr:], co[:Jc], co[8 - Jc:], co[:Jc])):           # tails among them
            with pytest.raises(RuntimeError, **hip):
                driver.get_celerite_matrices(ar, ac, bc, dc, x[:N], np.ones(N), np.empty(N), np.empty((N, Jw)), np.empty((N, Jw)))


def test_output_on_a_view_of_another_length_is_refused(built):
    """The one refusal the staging layer keeps (include/celerite2_amd.h, "Aliasing"): an OUTPUT that starts at the address
    of an argument of another length.  The reference would read rows this very call has already overwritten, which no
    staged copy reproduces; the call is refused before anything touches the device, in either argument order."""
    from celerite2_amd import driver

    n, k, J = 10, 4, 2
    x = np.linspace(0, 1, n)
    buf = np.ones((n, 1))
    U, V, c = np.ones((k, J)), np.ones((n, J)), np.ones(J)
    with pytest.raises(ValueError, match="Invalid shape"):
        driver.general_matmul_lower(x[:k], x, c, U, V, buf, buf[:k])       # Z on the first rows of Y
    with pytest.raises(ValueError, match="Invalid shape"):
        driver.general_matmul_lower(x, x[:k], c, V, U, buf[:k], buf)       # Y on the first rows of Z


def test_every_entry_point_names_its_hip_error(built):
    """C2_ERR_HIP never comes without text: without a device every device entry point, handed valid small host arrays
    (B = 1, N = 4, J = 2, one right-hand side and eight; nothing is launched, so they are never dereferenced), returns
    C2_ERR_HIP and leaves the HIP error's text in c2_last_error() (csrc/c2_launch.hpp)."""
    from celerite2_amd import _lib

    lib = _lib.load()
    if lib.c2_device_count() > 0:
        pytest.skip("a GPU is visible here")
    B, N, M, J = 1, 4, 3, 2
    i64, null = ctypes.c_int64, ctypes.c_void_p(0)
    keep = []

    def a(*shape):   # a fresh array of ones; the pointer stays valid for the whole test
        keep.append(np.ones(shape))
        return keep[-1].ctypes.data_as(ctypes.c_void_p)

    t, ts, c = np.arange(N, dtype=float), np.arange(M, dtype=float) + 0.5, np.ones(J)
    keep += [t, ts, c]
    tp, tsp, cp = (x.ctypes.data_as(ctypes.c_void_p) for x in (t, ts, c))
    flag = np.zeros(B, dtype=np.int32)
    fp = flag.ctypes.data_as(ctypes.c_void_p)
    tc = (tp, i64(N), cp, i64(J))   # t, t_bs, c, c_bs
    sizes = (i64(B), i64(N), i64(J))

    def work(nbytes):
        keep.append(np.zeros(max(int(nbytes), 8) // 8 + 1))
        return keep[-1].ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(int(nbytes))

    calls = [("c2_factor", lambda: lib.c2_factor(*sizes, *tc, a(N), a(N, J), a(N, J), a(N), a(N, J), null, fp, null)),
             ("c2_factor_rev", lambda: lib.c2_factor_rev(*sizes, *tc, a(N), a(N, J), a(N, J), a(N), a(N, J), a(N, J, J), a(N), a(N, J),
                                                        a(N), a(J), a(N), a(N, J), a(N, J), null)),
             ("c2_loglik", lambda: lib.c2_loglik(*sizes, *tc, a(N), a(N, J), a(N, J), a(N), a(B), fp, null)),
             ("c2_loglik_grad", lambda: lib.c2_loglik_grad(*sizes, *tc, a(N), a(N, J), a(N, J), a(N), a(B), a(N), a(J), a(N), a(N, J),
                                                          a(N, J), a(N), fp, *work(lib.c2_loglik_grad_workspace_bytes(B, N, J)), null)),
             ("c2_get_celerite_matrices", lambda: lib.c2_get_celerite_matrices(i64(B), i64(N), i64(0), i64(1), null, a(1), a(1), a(1),
                                                                              ctypes.c_int(0), tp, i64(N), a(N), a(N), a(N, J), a(N, J), null)),
             ("c2_loglik_terms", lambda: lib.c2_loglik_terms(i64(B), i64(N), i64(0), i64(1), null, null, a(1), a(1), a(1), a(1),
                                                            ctypes.c_int(0), tp, i64(N), a(N), a(N), a(B), fp,
                                                            *work(lib.c2_loglik_terms_workspace_bytes(B, N, 0, 1, 0)), null)),
             ("c2_kron_loglik", lambda: lib.c2_kron_loglik(i64(B), i64(N), i64(2), i64(J), *tc, a(N), a(N, J), a(N, J), a(2), i64(2),
                                                          a(N, 2), a(N, 2), a(B), fp, ctypes.c_int(0),
                                                          *work(lib.c2_kron_loglik_workspace_bytes(B, N, 2, J, 0, 0)), null)),
             ("c2_inverse_diag", lambda: lib.c2_inverse_diag(*sizes, *tc, a(N, J), a(N, J), a(N), null, a(N), null, null)),
             ("c2_explained_variance", lambda: lib.c2_explained_variance(i64(B), i64(N), i64(M), i64(J), tp, i64(N), tsp, i64(M), cp, i64(J),
                                                                        a(N, J), a(N, J), a(N), a(M, J), a(M, J), a(M), a(M, J), null))]
    for K in (1, 8):   # right-hand sides / draws
        k = i64(K)
        tail = lambda: (a(N, J), a(N, J), a(N, K), a(N, K))   # U, V | W, Y, Z
        rev = lambda: (a(N, J), a(N, J), a(N, K), a(N, K), a(N, J, K), a(N, K), a(N), a(J), a(N, J), a(N, J), a(N, K))
        calls += [("c2_solve_lower[%d]" % K, lambda k=k, tail=tail: lib.c2_solve_lower(*sizes, k, *tc, *tail(), null, null)),
                  ("c2_solve_upper[%d]" % K, lambda k=k, tail=tail: lib.c2_solve_upper(*sizes, k, *tc, *tail(), null, null)),
                  ("c2_matmul_lower[%d]" % K, lambda k=k, tail=tail: lib.c2_matmul_lower(*sizes, k, *tc, *tail(), null, ctypes.c_int(1), null)),
                  ("c2_matmul_upper[%d]" % K, lambda k=k, tail=tail: lib.c2_matmul_upper(*sizes, k, *tc, *tail(), null, ctypes.c_int(1), null)),
                  ("c2_general_matmul_lower[%d]" % K,
                   lambda k=k, K=K: lib.c2_general_matmul_lower(i64(B), i64(N), i64(M), i64(J), k, tp, i64(N), tsp, i64(M), cp, i64(J), a(N, J),
                                                                a(M, J), a(M, K), a(N, K), null, ctypes.c_int(1), null)),
                  ("c2_solve_lower_rev[%d]" % K, lambda k=k, rev=rev: lib.c2_solve_lower_rev(*sizes, k, *tc, *rev(), null)),
                  ("c2_matmul_lower_rev[%d]" % K, lambda k=k, rev=rev: lib.c2_matmul_lower_rev(*sizes, k, *tc, *rev(), null)),
                  ("c2_prior_draw[%d]" % K,
                   lambda k=k, K=K: lib.c2_prior_draw(i64(B), i64(N), i64(M), i64(J), k, tp, i64(N), tsp, i64(M), cp, i64(J), a(N, J), a(N, J),
                                                      a(M, J), a(M, J), a(N, K), a(M, K), a(N, K), a(M, K), null))]
    assert {n.split("[")[0] for n, _ in calls} == {
        "c2_factor", "c2_solve_lower", "c2_solve_upper", "c2_matmul_lower", "c2_matmul_upper", "c2_general_matmul_lower",
        "c2_factor_rev", "c2_solve_lower_rev", "c2_matmul_lower_rev", "c2_loglik", "c2_loglik_grad", "c2_get_celerite_matrices",
        "c2_loglik_terms", "c2_kron_loglik", "c2_inverse_diag", "c2_explained_variance", "c2_prior_draw"}
    set_error = ctypes.CFUNCTYPE(None, ctypes.c_char_p)(("c2_internal_set_error", lib))   # (a prototype of this test's own)
    for name, call in calls:
        set_error(b"")
        rc = call()
        assert rc == _lib.C2_ERR_HIP, (name, rc)
        assert lib.c2_last_error().decode().strip(), name


def test_one_launch_error_path():
    """csrc/c2_launch.hpp is the only place that turns a HIP error into C2_ERR_HIP (and records its text): no .hip names the
    code, and hipGetLastError appears nowhere else -- a sticky error is cleared on purpose only behind a refused
    stream-ordered temporary, and those are that header's too (temp_alloc, StreamTemp)."""
    import glob

    csrc = os.path.join(ROOT, "celerite2_amd", "csrc")
    for src in sorted(glob.glob(os.path.join(csrc, "*"))):
        if os.path.basename(src) == "c2_launch.hpp":
            continue
        text = open(src).read()
        assert "hipGetLastError" not in text, src
        if src.endswith(".hip"):
            assert "C2_ERR_HIP" not in text, src


def test_dispatch_options_table(built):
    """One option table (csrc/c2_dispatch.hpp): the environment is read once at load, c2_set_option changes an option at
    run time, no kernel source calls getenv, and INTEGRATION.md section 5 is the table the library was compiled with."""
    import glob
    import subprocess

    from celerite2_amd import _lib

    lib = _lib.load()
    opts = {o["name"]: o for o in _lib.options()}
    assert {"lanes", "timepar", "timepar_grad", "factor_iter", "lanes1_min_batch_grad", "timepar_cond_limit"} <= set(opts)
    assert opts["lanes1_min_batch_grad"]["default"] == 24576 and not opts["lanes"]["is_set"]
    _lib.set_option("lanes", 1)
    v, st = ctypes.c_double(), ctypes.c_int()
    assert lib.c2_get_option(b"C2_LANES", ctypes.byref(v), ctypes.byref(st)) == _lib.C2_OK and v.value == 1.0 and st.value == 1
    # the workspace query follows the option (one lane per series: records + the 16-byte guard)
    big = lib.c2_loglik_grad_workspace_bytes(128, 64, 8)
    _lib.set_option("lanes", None)
    assert lib.c2_get_option(b"lanes", ctypes.byref(v), ctypes.byref(st)) == _lib.C2_OK and st.value == 0
    assert lib.c2_loglik_grad_workspace_bytes(128, 64, 8) != big
    assert lib.c2_set_option(b"no_such_option", b"1") == _lib.C2_ERR_INVALID
    assert lib.c2_set_option(b"lanes", b"x") == _lib.C2_ERR_INVALID
    for src in glob.glob(os.path.join(ROOT, "celerite2_amd", "csrc", "*")):
        if os.path.basename(src) != "c2_dispatch.hip":
            assert "getenv(" not in open(src).read(), src
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_dispatch_doc.py"), "--check"]) == 0, \
        "INTEGRATION.md section 5 is stale: run python tools/gen_dispatch_doc.py"


def test_internal_interface_is_declared_once():
    """The functions one .hip of csrc/ defines and another calls (c2_internal_*, c2_wide_*, c2_loglik_grad_composite*; C
    linkage, so a stale private prototype would still link) are declared in csrc/c2_internal.hpp and nowhere else, each
    name the header declares is defined in exactly one .hip, and that .hip sees the header -- directly or through the
    .hip it #includes -- so the compiler compares definition and declaration."""
    import glob

    csrc = os.path.join(ROOT, "celerite2_amd", "csrc")
    call = re.compile(r"\b(C2TG?_NAME\(\s*\w+\s*\)|(?:c2_internal_|c2_wide_|c2_loglik_grad_composite)\w*(?:##\w+)?)\s*\(")
    typed = re.compile(r"\b(?:int|int64_t|size_t|void|double|bool|char|long)[\s\\*&]*$")

    def code(path):   # the text without comments and, except on #include lines, string contents
        s = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(path).read(), flags=re.S)
        return re.sub(r'^(?!#include).*$', lambda m: re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', m.group(0)), s, flags=re.M)

    def signatures(s):   # (name, ';' or '{') of every prototype / definition: a return type in front, what follows the ')'
        for m in call.finditer(s):
            if not typed.search(s[:m.start()]):
                continue
            depth, j = 0, m.end() - 1
            while True:
                depth += {"(": 1, ")": -1}.get(s[j], 0)
                j += 1
                if depth == 0:
                    break
            tail = s[j:].lstrip(" \t\n\\")
            if tail[:1] in (";", "{"):
                yield m.group(1), tail[0]

    def macros(s, known):   # object-like #defines with a plain value; the first definition wins (#ifndef defaults)
        for name, value in re.findall(r"^#define[ \t]+(\w+)[ \t]+(\w+)[ \t]*$", s, flags=re.M):
            known.setdefault(name, value)
        return known

    def resolve(name, known):
        while name in known:
            name = known[name]
        return name

    paths = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(csrc, "*.cpp")))
    text = {os.path.basename(p): code(p) for p in paths}
    header = text.pop("c2_internal.hpp")
    stray = [(f, n) for f, s in text.items() for n, end in signatures(s) if end == ";"]
    assert not stray, stray

    declared = set()
    families = dict(re.findall(r"^#define[ \t]+(C2_DECL_\w+)\(\w+\)((?:.*\\\n)*.*)$", header, flags=re.M))
    for n, end in signatures(re.sub(r"^#define(?:.*\\\n)*.*$", "", header, flags=re.M)):
        assert end == ";", n   # declarations only
        declared.add(n)
    for fam, body in families.items():
        suffixes = re.findall(r"^%s\((\w+)\)" % fam, header, flags=re.M)
        assert suffixes, fam
        for n, end in signatures(body):
            assert end == ";" and "##" in n, (fam, n)
            declared |= {n.split("##")[0] + sfx for sfx in suffixes}
    assert len(declared) > 100, len(declared)

    defined = {}   # name -> [.hip that is compiled on its own and defines it]
    included = {f: re.findall(r'^#include "(\w+\.hip)"', s, flags=re.M) for f, s in text.items()}
    wrapped = {inc for incs in included.values() for inc in incs}
    for f, s in text.items():
        if not f.endswith(".hip"):
            continue
        known, units = macros(s, {}), [s]
        for inc in included[f]:
            macros(text[inc], known)
            units.append(text[inc])
        sees_header = any('#include "c2_internal.hpp"' in u for u in units)
        for u in units:
            for n, end in signatures(u):
                if end != "{":
                    continue
                m = re.match(r"(C2TG?_NAME)\(\s*(\w+)\s*\)", n)
                if m:   # stem + suffix: C2T_NAME -> C2T_JS (-> C2T_J), C2TG_NAME -> C2TG_ROWS
                    n = m.group(2) + resolve("C2T_JS" if m.group(1) == "C2T_NAME" else "C2TG_ROWS", known)
                if n in declared:
                    assert sees_header, (f, n)
                    defined.setdefault(n, []).append(f)
    assert set(defined) == declared, declared ^ set(defined)
    assert all(len(fs) == 1 for fs in defined.values()), {n: fs for n, fs in defined.items() if len(fs) != 1}
    assert wrapped == {"c2_loglik_t.hip", "c2_timepar_grad.hip"}
