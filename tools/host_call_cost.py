"""Per-call cost of the host-pointer drop-in modules (celerite2_amd.driver / backprop over c2h_*): one PCIe round trip,
one hipMalloc / hipMemcpy / hipFree per argument and a device sync per call (c2_host.hip).
--loglik: the host cost of c2_loglik_grad / c2_loglik_terms_grad on device arrays instead (below)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

if "--loglik" in sys.argv:
    # python tools/host_call_cost.py --loglik: what the HOST spends per call of the fused entry points on device arrays --
    # dispatch plan, argument checks, launches -- at a shape whose kernels take less than that (8 series of 16 rows,
    # J = 8): n calls enqueued back to back, one synchronisation at the end, the median of five rounds
    import torch
    from celerite2_amd import ops, synth
    dev = torch.device("cuda:0")
    B, N, J = 8, 16, 8
    t, c, a, U, V, y = synth.device_batch(0, B, N, J, dev)
    rng = np.random.default_rng(3)
    ac = rng.uniform(0.5, 2.0, (B, 4)); cc = rng.uniform(0.02, 0.3, (B, 4)); dc = rng.uniform(0.2, 3.0, (B, 4))
    co = [torch.zeros((B, 0), dtype=torch.float64, device=dev)] * 2 + [torch.from_numpy(v).to(dev) for v in (ac, 0.5 * ac * cc / dc, cc, dc)]
    diag = torch.full((B, N), 0.2, dtype=torch.float64, device=dev)
    work = ops.loglik_grad_workspace(B, N, J, dev)
    out = ops.loglik_grad(t, c, a, U, V, y, work=work)[1]
    twork = ops.loglik_terms_workspace(B, N, 0, 4, dev)
    tout = ops.loglik_terms_grad(*co, t, diag, y, work=twork)[1]
    calls = {"c2_loglik_grad": lambda: ops.loglik_grad(t, c, a, U, V, y, work=work, out=out),
             "c2_loglik_terms_grad": lambda: ops.loglik_terms_grad(*co, t, diag, y, work=twork, out=tout)}
    n = 2000
    for name, call in calls.items():
        rounds = []
        for _ in range(6):   # (the first round warms up and is dropped)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n): call()
            torch.cuda.synchronize()
            rounds.append((time.perf_counter() - t0) / n * 1e6)
        print("%s (through ops, B=%d N=%d J=%d): %.2f us per call (rounds: %s)" % (name, B, N, J, float(np.median(rounds[1:])),
                                                                               " ".join("%.2f" % r for r in rounds[1:])), flush=True)
    sys.exit(0)

from celerite2_amd import driver
from oracle import dense
for (N, J) in [(1000, 2), (4096, 8), (100000, 8)]:
    co = dense.sho_sum_coeffs(J)
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(0, N / 10.0, N)); diag = rng.uniform(0.1, 0.3, N)
    c, a, U, V = dense.celerite_matrices(co, t, diag)
    Y = rng.standard_normal((N, 1))
    d, W = np.empty_like(a), np.empty_like(V)
    Z = np.empty_like(Y)
    for _ in range(3): driver.factor(t, c, a, U, V, d, W); driver.solve_lower(t, c, U, W, Y, Z)
    n = 20
    t0 = time.perf_counter()
    for _ in range(n): driver.factor(t, c, a, U, V, d, W)
    tf = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    for _ in range(n): driver.solve_lower(t, c, U, W, Y, Z)
    ts = (time.perf_counter() - t0) / n
    print("N=%d J=%d: driver.factor %.0f us per call (%.1f KB each way), driver.solve_lower %.0f us" % (N, J, tf * 1e6, 8 * N * (3 + 3 * J) / 1e3, ts * 1e6), flush=True)


# the reverse-mode chain of the drop-in (celerite2_amd.backprop, same signatures as the reference's backprop module) on
# ONE series -- factor_fwd, solve_lower_fwd, solve_lower_rev, factor_rev -- beside the CPU restatement (oracle/, one thread)
from celerite2_amd import backprop
from oracle import cpu as ocpu
ocpu.build()
for (N, J) in [(1000, 2), (4096, 8), (20000, 4), (100000, 8)]:
    co = dense.sho_sum_coeffs(J)
    rng = np.random.default_rng(2)
    t = np.sort(rng.uniform(0, N / 10.0, N)); diag = rng.uniform(0.1, 0.3, N)
    c, a, U, V = dense.celerite_matrices(co, t, diag)
    Y = rng.standard_normal((N, 1)); bZ = rng.standard_normal((N, 1))
    d, W, S = np.empty_like(a), np.empty_like(V), np.empty((N, J, J))
    Z, F = np.empty_like(Y), np.empty((N, J, 1))
    bt, bc, ba, bU, bV, bY = np.zeros(N), np.zeros(J), np.zeros(N), np.zeros((N, J)), np.zeros((N, J)), np.zeros((N, 1))
    bd, bW = rng.standard_normal(N), rng.standard_normal((N, J))

    def chain(m):
        m.factor_fwd(t, c, a, U, V, d, W, S)
        m.solve_lower_fwd(t, c, U, W, Y, Z, F)
        m.solve_lower_rev(t, c, U, W, Y, Z, F, bZ, bt, bc, bU, bV, bY)
        m.factor_rev(t, c, a, U, V, d, W, S, bd, bW, bt, bc, ba, bU, bV)

    res = {}
    for name, m in (("drop-in", backprop), ("cpu", ocpu)):
        for _ in range(2): chain(m)
        n = 10
        t0 = time.perf_counter()
        for _ in range(n): chain(m)
        res[name] = (time.perf_counter() - t0) / n
    print("N=%d J=%d: factor_fwd + solve_lower_fwd + solve_lower_rev + factor_rev: drop-in (host arrays, copies included) %.2f ms, "
          "CPU restatement (1 thread) %.2f ms" % (N, J, res["drop-in"] * 1e3, res["cpu"] * 1e3), flush=True)
