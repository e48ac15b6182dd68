#!/usr/bin/env python
"""Host cost of one call through the Python binding (profiles/binding_overhead.md).

  bare marshalling   lib.c2_loglik with B = 0 -- refused with C2_ERR_INVALID before anything is launched, so it needs no
                     device -- 1e5 calls.  --wrapped: every argument wrapped by hand (c_int64 / c_void_p), as ops.py did
                     before the prototypes came from the header; otherwise plain values.
  whole ops          (with a GPU) ops.solve_lower and ops.explained_variance_rev at B = 2, N = 5, M = 3, J = 2, nrhs = 2,
                     caller-owned outputs: 2000 calls after 200 warm-up calls, one synchronize at the end.
Five repeats each; prints one JSON line of microseconds per call.  --package NAME measures another copy of ops.py / _lib.py
(say, an earlier commit's, saved as a package on PYTHONPATH, with C2_LIB_PATH pointing at the same library)."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--package", default="celerite2_amd")
ap.add_argument("--wrapped", action="store_true")
args = ap.parse_args()
_lib = importlib.import_module(args.package + "._lib")
ops = importlib.import_module(args.package + ".ops")


def per_call_us(f, calls, warmup, sync=lambda: None):
    reps = []
    for _ in range(5):
        for _ in range(warmup):
            f()
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        sync()
        reps.append(round((time.perf_counter() - t0) / calls * 1e6, 3))
    return reps


lib = _lib.load()
t, c, a, U, V, y, ll = (torch.zeros(4, dtype=torch.float64) for _ in range(7))
flag = torch.zeros(1, dtype=torch.int32)
if args.wrapped:
    i64, p = ctypes.c_int64, lambda x: ctypes.c_void_p(x.data_ptr())
    bare = lambda: lib.c2_loglik(i64(0), i64(4), i64(2), p(t), i64(0), p(c), i64(0), p(a), p(U), p(V), p(y), p(ll), p(flag),
                                 ctypes.c_void_p(0))
else:
    bare = lambda: lib.c2_loglik(0, 4, 2, t, 0, c, 0, a, U, V, y, ll, flag, ctypes.c_void_p(0))
assert bare() == _lib.C2_ERR_INVALID
res = {"package": args.package, "wrapped": args.wrapped, "us_per_call": {"c2_loglik(B=0)": per_call_us(bare, 100000, 1000)}}

if torch.cuda.is_available():
    B, N, M, J, R = 2, 5, 3, 2, 2
    g = torch.Generator().manual_seed(20)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64).cuda()
    t, ts = torch.cumsum(0.3 + rand(N), 0), 0.3 + torch.cumsum(0.45 + rand(M), 0)
    ac, bc, cc, dc = (torch.tensor([v], dtype=torch.float64, device="cuda") for v in (1.0, 0.1, 0.5, 1.3))
    c = torch.cat([cc, cc])
    a, U, V = ops.get_celerite_matrices(rand(0), ac, bc, dc, t, 0.1 + rand(B, N))
    _, Us, Vs = ops.get_celerite_matrices(rand(0), ac, bc, dc, ts, torch.zeros((B, M), dtype=torch.float64, device="cuda"))
    d, W, _ = ops.factor(t, c, a, U, V)
    Y = rand(B, N, R)
    Z = torch.empty_like(Y)
    work = torch.empty((B, M, J), dtype=torch.float64, device="cuda")
    _, ws = ops.explained_variance(t, ts, c, U, W, d, Us, Vs, work=work, workspace=True)
    br = rand(B, M)
    out = ops.explained_variance_rev(t, ts, c, U, W, d, Us, Vs, work, ws, br)
    for name, f in (("solve_lower", lambda: ops.solve_lower(t, c, U, W, Y, Z=Z)),
                    ("explained_variance_rev", lambda: ops.explained_variance_rev(t, ts, c, U, W, d, Us, Vs, work, ws, br, out=out))):
        res["us_per_call"][name] = per_call_us(f, 2000, 200, torch.cuda.synchronize)
print(json.dumps(res))
