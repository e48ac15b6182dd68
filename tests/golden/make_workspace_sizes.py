# -*- coding: utf-8 -*-
"""Records what the workspace queries of the fused log-likelihood entry points return, so that a change of the host-side
dispatch can be held to the sizes of the commit it started from (tests/test_workspace_plan.py).  Host functions only: no
device is needed.

    python tests/golden/make_workspace_sizes.py          # writes tests/golden/workspace_sizes.npz

Run it on the commit whose sizes are the reference, never to make a failing test pass.  Keys of the file:
    B, N, J, splits                the grid (splits: the (Jr, Jc) of the coefficient-level query, Jr + 2 Jc <= 8)
    settings                       "default" and the forced options, as "name=value"
    grad/<setting>                 c2_loglik_grad_workspace_bytes                       [B, N, J]
    rows/<setting>                 c2_internal_loglik_grad_rows_workspace_bytes         [B, N, J]
    replay/<setting>               c2_internal_loglik_grad_replay_doubles               [B, N, J]
    terms/<setting>                c2_loglik_terms_workspace_bytes                      [B, N, split, grad]
    kron/<setting>                 c2_kron_loglik_workspace_bytes, grad = 1             [B, N, J, M, method]
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

GRID_B = [1, 63, 64, 65, 300, 9215, 9216, 16384, 16385, 24575, 24576, 32768, 32769, 65536]
GRID_N = [1, 2, 33, 384, 1024, 4096, 12000]
GRID_J = [1, 2, 3, 4, 6, 8, 12, 16, 32, 40]
SPLITS = [(Jr, Jc) for J in GRID_J if J <= 8 for Jc in range(J // 2 + 1) for Jr in [J - 2 * Jc]]
KRON_M = [2, 3]
SETTINGS = [None] + [("lanes", v) for v in (1, 2, 4, 8)] + [("timepar_grad", v) for v in (0, 1)] + [("loglik_back", 0)]
OUT = os.path.join(HERE, "workspace_sizes.npz")


def setting_name(s):
    return "default" if s is None else "%s=%d" % s


def queries():
    """The five size queries, typed (the internal ones are exported but in no public header)."""
    from celerite2_amd import _lib

    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    i64 = ctypes.c_int64
    for name in ("c2_loglik_grad_workspace_bytes", "c2_internal_loglik_grad_rows_workspace_bytes", "c2_internal_loglik_grad_replay_doubles"):
        getattr(raw, name).restype, getattr(raw, name).argtypes = ctypes.c_size_t, [i64] * 3
    raw.c2_loglik_terms_workspace_bytes.restype, raw.c2_loglik_terms_workspace_bytes.argtypes = ctypes.c_size_t, [i64] * 4 + [ctypes.c_int]
    raw.c2_kron_loglik_workspace_bytes.restype, raw.c2_kron_loglik_workspace_bytes.argtypes = ctypes.c_size_t, [i64] * 4 + [ctypes.c_int] * 2
    return raw


def record(raw):
    """name -> array of one setting, at the options in force"""
    nB, nN, nJ = len(GRID_B), len(GRID_N), len(GRID_J)
    out = {"grad": np.zeros((nB, nN, nJ), np.uint64), "rows": np.zeros((nB, nN, nJ), np.uint64),
           "replay": np.zeros((nB, nN, nJ), np.uint64), "terms": np.zeros((nB, nN, len(SPLITS), 2), np.uint64),
           "kron": np.zeros((nB, nN, nJ, len(KRON_M), 2), np.uint64)}
    for ib, B in enumerate(GRID_B):
        for iN, N in enumerate(GRID_N):
            for ij, J in enumerate(GRID_J):
                out["grad"][ib, iN, ij] = raw.c2_loglik_grad_workspace_bytes(B, N, J)
                out["rows"][ib, iN, ij] = raw.c2_internal_loglik_grad_rows_workspace_bytes(B, N, J)
                out["replay"][ib, iN, ij] = raw.c2_internal_loglik_grad_replay_doubles(B, N, J)
                for im, M in enumerate(KRON_M):
                    for method in (0, 1):
                        out["kron"][ib, iN, ij, im, method] = raw.c2_kron_loglik_workspace_bytes(B, N, M, J, method, 1)
            for isp, (Jr, Jc) in enumerate(SPLITS):
                for grad in (0, 1):
                    out["terms"][ib, iN, isp, grad] = raw.c2_loglik_terms_workspace_bytes(B, N, Jr, Jc, grad)
    return out


def record_all():
    from celerite2_amd import _lib

    raw = queries()
    data = {"B": np.array(GRID_B), "N": np.array(GRID_N), "J": np.array(GRID_J), "splits": np.array(SPLITS),
            "settings": np.array([setting_name(s) for s in SETTINGS])}
    for s in SETTINGS:
        if s is not None:
            _lib.set_option(s[0], s[1])
        try:
            for k, v in record(raw).items():
                data["%s/%s" % (k, setting_name(s))] = v
        finally:
            if s is not None:
                _lib.set_option(s[0], None)
    return data


if __name__ == "__main__":
    np.savez_compressed(OUT, **record_all())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
