# -*- coding: utf-8 -*-
"""The workspace of the interleaved 2-D gradient (c2_kron_loglik_grad, method C2_KRON_INTERLEAVED) holds what its 1-D pass
writes.  That pass is c2_internal_loglik_grad_rows, the row-by-row forms only; where c2_loglik_grad itself would run parallel
along time, c2_loglik_grad_workspace_bytes is the room of the time-parallel form, which can be LESS than the backward
recursion's W records (2 series x 12000 rows x width 4: 651268 doubles against 1248290) -- the 2-D plan used to reserve the
former and the kernels wrote past the end of the caller's workspace.  Host functions only: no device is needed."""
import ctypes

import pytest

SHAPES = [(5, 300, 16, 6), (3, 1000, 5, 8), (9, 33, 7, 3), (2, 1, 4, 2), (70, 50, 2, 4), (2, 1500, 8, 4), (1, 4000, 3, 2),
          (1, 20000, 4, 8), (300, 200, 2, 8)]   # (B, N, M, J): tests/test_gpu_kron.py's, and longer and larger ones


@pytest.fixture(scope="module")
def raw():
    from celerite2_amd import _lib, build

    build.build_all()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("c2_loglik_grad_workspace_bytes", "c2_internal_loglik_grad_rows_workspace_bytes", "c2_internal_loglik_g8_tt_doubles",
                 "c2_internal_loglik_grad_replay_doubles"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int64] * 3
    lib.c2_kron_loglik_workspace_bytes.restype = ctypes.c_size_t
    lib.c2_kron_loglik_workspace_bytes.argtypes = [ctypes.c_int64] * 4 + [ctypes.c_int] * 2
    return lib


@pytest.mark.parametrize("B,N,M,J", SHAPES)
def test_interleaved_gradient_workspace_holds_the_row_by_row_pass(raw, B, N, M, J):
    R = N * M
    rows = raw.c2_internal_loglik_grad_rows_workspace_bytes(B, R, J)
    # the row-by-row pass never needs less than the public size, and holds the backward form (W records) and the replay pair
    assert rows >= raw.c2_loglik_grad_workspace_bytes(B, R, J) > 0
    if R >= 2:
        assert rows >= 8 * raw.c2_internal_loglik_g8_tt_doubles(B, R, J)
    assert rows >= 8 * raw.c2_internal_loglik_grad_replay_doubles(B, R, J)
    # the 2-D plan: t', a', U', V' and their four gradients (each padded to an even count), the partial sums, then that pass
    even = lambda n: (n + 1) & ~1
    arrays = 8 * (4 * even(B * R) + 4 * even(B * R * J))
    assert raw.c2_kron_loglik_workspace_bytes(B, N, M, J, 1, 1) >= arrays + rows


def test_the_shape_that_overflowed(raw):
    assert raw.c2_loglik_grad_workspace_bytes(2, 12000, 4) // 8 == 651268             # the time-parallel form's room
    assert raw.c2_internal_loglik_grad_rows_workspace_bytes(2, 12000, 4) // 8 == 1248290   # what the row-by-row pass writes
