# -*- coding: utf-8 -*-
"""CPU-side checks of the ragged batches (celerite2_amd/packed.py, csrc/c2_packed_api.h, csrc/c2_packed.hip): the Packed
container, celerite_rows against the oracle's get_celerite_matrices and against torch's gradcheck, the provisional header
held to its exports and its typing the way tests/test_abi.py holds the public ones, the public tables untouched, the
argument errors that come back before anything is launched, and the workspace formula with the condition it was built to."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from celerite2_amd import packed   # (the module is the feature: without it this file does not import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from celerite2_amd import build

    build.build_all()
    return build


def _series(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(np.sort(rng.uniform(0.0, 10.0, n))) for n in lengths]


# ---- the container ----------------------------------------------------------------------------------------------------------
def test_from_list_offsets_and_order():
    lengths = [3, 0, 7, 3, 1, 7, 0]
    pk = packed.Packed.from_list(_series(lengths))
    assert (pk.B, pk.R, pk.n_max) == (7, 21, 7)
    assert pk.offsets.dtype == torch.int64 and pk.offsets.tolist() == [0, 3, 3, 10, 13, 14, 21, 21]
    assert pk.lengths.tolist() == lengths
    assert pk.order.dtype == torch.int32 and pk.order.tolist() == [2, 5, 0, 3, 4, 1, 6]   # descending, ties in order
    assert pk.seg.dtype == torch.int64 and pk.seg.tolist() == sum(([b] * n for b, n in enumerate(lengths)), [])
    one = packed.Packed(torch.zeros(0, dtype=torch.float64), [0])
    assert (one.B, one.R, one.n_max) == (1, 0, 0) and one.offsets.tolist() == [0, 0] and one.seg.numel() == 0
    same = packed.Packed(pk.t, torch.tensor(lengths))
    assert same.offsets.tolist() == pk.offsets.tolist()


def test_unpack_and_padded_round_trip():
    lengths = [3, 0, 7, 1]
    ts = _series(lengths, 1)
    pk = packed.Packed.from_list(ts)
    views = pk.unpack(pk.t)
    assert [v.tolist() for v in views] == [x.tolist() for x in ts]
    assert views[2].data_ptr() == pk.t.data_ptr() + 8 * 3   # views, not copies
    X = torch.arange(pk.R * 2, dtype=torch.float64).reshape(pk.R, 2)
    P = pk.to_padded(X, fill=-1.0)
    assert tuple(P.shape) == (4, 7, 2)
    for b, n in enumerate(lengths):
        assert torch.equal(P[b, :n], pk.unpack(X)[b]) and bool((P[b, n:] == -1.0).all())
    assert torch.equal(pk.from_padded(P), X)
    assert torch.equal(pk.from_padded(pk.to_padded(pk.t)), pk.t)
    with pytest.raises(ValueError):
        pk.unpack(torch.zeros(pk.R + 1))
    with pytest.raises(ValueError):
        pk.from_padded(torch.zeros(4, 6))


def test_construction_checks():
    t = torch.arange(6, dtype=torch.float64)
    with pytest.raises(ValueError):
        packed.Packed(t.float(), [6])              # dtype
    with pytest.raises(ValueError):
        packed.Packed(torch.arange(12, dtype=torch.float64)[::2], [6])   # contiguity
    with pytest.raises(ValueError):
        packed.Packed(t.reshape(2, 3), [6])        # one dimension
    with pytest.raises(ValueError):
        packed.Packed(t, [2, 3])                   # sum(lengths) != R
    with pytest.raises(ValueError):
        packed.Packed(t, [7, -1])                  # negative length
    with pytest.raises(ValueError):
        packed.Packed(t, [])                       # no series
    with pytest.raises(ValueError):
        packed.Packed(t, [2.0, 4.0])               # lengths are integers
    back = torch.tensor([0.0, 1.0, 0.5, 2.0, 3.0, 4.0], dtype=torch.float64)
    with pytest.raises(ValueError):
        packed.Packed(back, [4, 2])                # times decrease inside series 0
    assert packed.Packed(back, [4, 2], check_sorted=False).R == 6
    assert packed.Packed(back, [2, 4]).B == 2      # ... but not when the drop is a series boundary
    assert packed.Packed(back, [2, 0, 4]).B == 3
    with pytest.raises(ValueError):
        packed.Packed.from_list([])
    with pytest.raises(ValueError):
        packed.Packed.from_list([torch.zeros(2, 2, dtype=torch.float64)])


# ---- celerite_rows ------------------------------------------------------------------------------------------------------------
def _coefs(rng, B, Jr, Jc):
    return [torch.from_numpy(rng.uniform(0.1, 1.5, (B, n))) for n in (Jr, Jr, Jc, Jc, Jc, Jc)]


@pytest.mark.parametrize("Jr,Jc", [(1, 0), (0, 1), (2, 3)])
def test_celerite_rows_against_the_oracle(oracle, Jr, Jc):
    lengths = (0, 1, 7, 40)
    rng = np.random.default_rng(10 * Jr + Jc)
    pk = packed.Packed.from_list(_series(lengths, 3))
    ar, cr, ac, bc, cc, dc = coefs = _coefs(rng, pk.B, Jr, Jc)
    diag = torch.from_numpy(rng.uniform(0.5, 1.0, pk.R))
    c, a, U, V = packed.celerite_rows(coefs, pk, diag)
    J = Jr + 2 * Jc
    assert tuple(c.shape) == (pk.B, J) and tuple(a.shape) == (pk.R,) and tuple(U.shape) == tuple(V.shape) == (pk.R, J)
    for b, n in enumerate(lengths):
        x = np.ascontiguousarray(pk.unpack(pk.t)[b].numpy())
        ao, Uo, Vo = np.empty(n), np.empty((n, J)), np.empty((n, J))
        h = lambda v: np.ascontiguousarray(v[b].numpy())
        if n:
            oracle.get_celerite_matrices(h(ar), h(ac), h(bc), h(dc), x, np.ascontiguousarray(pk.unpack(diag)[b].numpy()), ao, Uo, Vo)
        for got, want in ((pk.unpack(a)[b], ao), (pk.unpack(U)[b], Uo), (pk.unpack(V)[b], Vo)):
            got = got.numpy()
            assert got.shape == want.shape
            if n:
                assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), (b, np.abs(got - want).max())
        co = np.concatenate([cr[b].numpy(), np.repeat(cc[b].numpy(), 2)])   # (terms.py:171-173)
        assert np.array_equal(c[b].numpy(), co)
    # coefficients shared by the batch: (Jr,) / (Jc,)
    c1, a1, U1, V1 = packed.celerite_rows([v[2] for v in coefs], pk, diag)
    sel = pk.seg == 2
    assert torch.equal(a1[sel], a[sel]) and torch.equal(U1[sel], U[sel]) and torch.equal(c1[3], c[2])


def test_celerite_rows_gradcheck():
    rng = np.random.default_rng(5)
    lengths = [2, 0, 3]
    t0 = torch.cat(_series(lengths, 7))
    coefs = [v.requires_grad_() for v in _coefs(rng, 3, 2, 1)]
    diag = torch.from_numpy(rng.uniform(0.5, 1.0, 5)).requires_grad_()

    def f(t, diag, *co):
        return packed.celerite_rows(co, packed.Packed(t, lengths, check_sorted=False), diag)

    assert torch.autograd.gradcheck(f, (t0.clone().requires_grad_(), diag, *coefs), eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- the provisional header against its exports and its typing ---------------------------------------------------------------
def test_header_exports_typing(built):
    from celerite2_amd import _lib

    text = packed.header_text()
    declared = re.findall(r"([\w \t*]+?)\b(c2h?_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [name for _, name, _ in declared] == list(_lib._prototypes(text)) == packed.SYMBOLS
    assert len(packed.SYMBOLS) == len(set(packed.SYMBOLS)) == 3
    loose = set(re.findall(r"\b(c2h?_[a-z0-9_]+)\s*\(", text))
    assert loose == set(packed.SYMBOLS), loose ^ set(packed.SYMBOLS)
    so = ctypes.CDLL(_lib.LIB_PATH)
    fns = packed._load()
    assert list(fns) == packed.SYMBOLS
    restypes = {"size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p, "void": None, "int64_t": ctypes.c_int64}
    for ret, name, params in declared:
        assert hasattr(so, name), name
        fn = fns[name]
        assert fn.argtypes is not None, name
        assert len(fn.argtypes) == len(params.split(",")), name
        assert fn.restype is restypes.get(" ".join(ret.split()), ctypes.c_int), name
        want = [_lib._ctype(re.sub(r"\w+$", "", p.strip()), name) for p in params.split(",")]
        assert list(fn.argtypes) == want, name
        with pytest.raises(TypeError):   # exactly that many arguments
            fn(*([0] * (len(want) + 1)))
    assert os.path.samefile(packed.HEADER, os.path.join(ROOT, "celerite2_amd", "csrc", "c2_packed_api.h"))
    assert packed.HEADER in built.HIP_HEADERS
    assert "c2_packed.hip" in built.HIP_SOURCES


def test_public_tables_untouched():
    from celerite2_amd import _lib, ops

    public = {s for r in _lib.HEADERS.values() for s in r.symbols}
    assert not public & set(packed.SYMBOLS)
    names = set(ops.__all__) | {n for r in _lib.HEADERS.values() if r.ops for n in r.ops}
    assert not any("packed" in n for n in names) and not names & {s[3:] for s in packed.SYMBOLS}
    assert not any("packed" in n for n in dir(ops))
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(r.file for r in _lib.HEADERS.values())
    assert not any("packed" in f for f in os.listdir(os.path.join(ROOT, "include")))
    lib = _lib.load()
    assert all(getattr(lib, n).argtypes is None for n in packed.SYMBOLS)   # _lib.load() has not typed them
    src = open(os.path.join(ROOT, "celerite2_amd", "csrc", "c2_packed.hip")).read()
    assert not re.search(r"\bc2_(internal|wide)_\w+\s*\([^)]*\)\s*\{", src)   # defines no cross-file name
    assert not re.search(r'#include\s+"\w+\.hip"', src)


# ---- argument errors before anything is launched (no device needed) -----------------------------------------------------------
def test_argument_errors_without_gpu(built):
    from celerite2_amd import _lib

    fns = packed._load()
    fwd, grad, query = fns["c2_packed_loglik"], fns["c2_packed_loglik_grad"], fns["c2_packed_loglik_grad_workspace_bytes"]
    p = ctypes.c_void_p(64)   # stands for a valid pointer: every call below returns before it would be used
    null = None

    def f_args(B=2, R=5, J=3, ptrs=None):
        q = ptrs or {}
        g = lambda k: q.get(k, p)
        return (B, R, J, g("offsets"), null, g("t"), g("c"), 0, g("a"), g("U"), g("V"), g("y"), g("ll"), g("flag"), null, null, null, null)

    def g_args(B=2, R=5, Nmax=3, J=3, ptrs=None, short=0):
        q = ptrs or {}
        g = lambda k: q.get(k, p)
        return (B, R, Nmax, J, g("offsets"), null, g("t"), g("c"), 0, g("a"), g("U"), g("V"), g("y"), g("ll"), g("bt"), g("bc"),
                g("ba"), g("bU"), g("bV"), g("by"), g("flag"), g("work"), max(query(B, R, Nmax, J), 1) - short, null)

    assert fwd(*f_args(B=0)) == grad(*g_args(B=0)) == _lib.C2_ERR_INVALID
    assert fwd(*f_args(J=0)) == grad(*g_args(J=0)) == _lib.C2_ERR_INVALID
    assert fwd(*f_args(R=-1)) == grad(*g_args(R=-1)) == _lib.C2_ERR_INVALID
    assert grad(*g_args(Nmax=-1)) == _lib.C2_ERR_INVALID
    assert fwd(*f_args(J=33)) == grad(*g_args(J=33)) == _lib.C2_ERR_UNSUPPORTED
    assert grad(*g_args(Nmax=2**30 + 1)) == _lib.C2_ERR_UNSUPPORTED
    for k in ("offsets", "t", "c", "a", "U", "V", "y", "ll", "flag"):
        assert fwd(*f_args(ptrs={k: null})) == _lib.C2_ERR_INVALID, k
    for k in ("offsets", "t", "c", "a", "U", "V", "y", "ll", "bt", "bc", "ba", "bU", "bV", "by", "flag", "work"):
        assert grad(*g_args(ptrs={k: null})) == _lib.C2_ERR_INVALID, k
    assert grad(*g_args(short=1)) == _lib.C2_ERR_INVALID
    assert grad(*g_args(B=70000, R=175000, Nmax=5, J=32, short=1)) == _lib.C2_ERR_INVALID
    for J in (0, 33, 128):
        assert query(4, 100, 50, J) == 0
    assert query(0, 100, 50, 8) == query(4, -1, 50, 8) == query(4, 100, -1, 8) == 0


# ---- the workspace ------------------------------------------------------------------------------------------------------------
def _formula(B, R, Nmax, J):   # csrc/c2_packed_api.h
    C = max(1, math.isqrt(Nmax - 1) + 1 if Nmax > 0 else 1)
    assert (C - 1) ** 2 < max(Nmax, 1) <= C * C
    return 8 * (R * (J + 2) + 2 * B * C * (J * J + J) + 32), C


def test_workspace_formula_and_condition(built):
    query = packed._load()["c2_packed_loglik_grad_workspace_bytes"]
    for B, R, Nmax, J in [(1, 1, 1, 1), (3, 200, 150, 5), (130, 5000, 49, 17), (2, 0, 0, 8)]:
        want, C = _formula(B, R, Nmax, J)
        assert query(B, R, Nmax, J) == want, (B, R, Nmax, J)
        assert packed.checkpoint_interval(Nmax) == C
    assert "8 * (R * (J + 2) + 2 * B * C * (J^2 + J) + 32)" in open(packed.HEADER).read()
    # the condition the scheme was built to: rows x J, not rows x J^2
    for B, R, Nmax, J in [(1, 1, 1, 1), (3, 200, 150, 5), (8192, 8192 * 4096, 4096, 8), (70000, 175000, 5, 32)]:
        C = math.isqrt(Nmax - 1) + 1   # ceil(sqrt(Nmax))
        bound = 8 * R * (J + 4) + 8 * B * (2 * C + 2) * (J * J + J + 4) + 4096
        got = query(B, R, Nmax, J)
        assert 0 < got <= bound, (B, R, Nmax, J, got, bound)
    got = query(8192, 8192 * 4096, 4096, 8)
    assert got < 3.4e9 and got < (8192 * 4096 * 8 * (8 + 64)) / 5   # filter_append_rev's ws alone: 19.3 GB
    assert [packed.checkpoint_interval(n) for n in (0, 1, 2, 4, 5, 9, 10, 150, 4096, 4097)] == [1, 1, 2, 2, 3, 3, 4, 13, 64, 65]


def test_ops_refuse_bad_arguments_without_gpu():
    """The Python layer's own checks come before the library is asked for anything."""
    pk = packed.Packed.from_list(_series([2, 3]))
    z = torch.zeros
    with pytest.raises(ValueError):
        packed.loglik(pk, z(2, dtype=torch.float64), z(5, dtype=torch.float64), z(5, 2, dtype=torch.float64),
                      z(5, 2, dtype=torch.float64), z(5, dtype=torch.float64))   # CPU tensors: no fallback
    with pytest.raises(TypeError):
        packed.loglik(None, None, None, z(5, 2), None, None)
    with pytest.raises(ValueError):
        packed.celerite_rows([z(3, 1, dtype=torch.float64)] * 6, pk, z(5, dtype=torch.float64))   # B = 2
    with pytest.raises(ValueError):
        packed.celerite_rows([z(2, 1, dtype=torch.float64)] * 6, pk, z(4, dtype=torch.float64))   # R = 5
