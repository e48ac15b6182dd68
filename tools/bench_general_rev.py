# -*- coding: utf-8 -*-
"""What the reverse of general_matmul_lower costs (csrc/c2_general_rev.hip), on one device, in ONE fresh process:

    python tools/bench_general_rev.py [--steps 20] [--out profiles/general_rev.md] [--quick]
    python tools/bench_general_rev.py --regs-only --out profiles/general_rev.md     # no GPU: refresh the register table

  (a) ops.general_matmul_lower(workspace=True) and ops.general_matmul_lower_rev, one right-hand side, at
      8192 x 4096 x 4096 x 8 and 64 x 4096 x 4096 x 8 (B x N x M x J), alternating step by step;
  (b) autograd.predict_mean forward + backward (all nine gradients) at 64 x 4096 x 4096 x 8 beside the dense route under
      torch autograd on the same device -- K from the semiseparable form, linalg.solve, the N x M cross-covariance -- which
      is run on --dense-series series at a time (its (N, M, J) intermediates are 1 GB per series) and reported per series.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the tables give the median
(min .. max) and, for (a), the algorithmic bytes as a fraction of the 8 TB/s roofline.  In doubles:
    general_matmul_lower + workspace   N (3 + J)   (t1, U, Z read and written)      + M (2 + 2 J)  (t2, Y, V; F out)
    general_matmul_lower_rev           N (3 + 2 J) (t1, bZ, U; bt1, bU out)         + M (4 + 3 J)  (t2, Y, V, F; bt2, bY, bV out)
The query grid of the measurement is the data grid shifted by a third of its mean spacing with the data's own U, V as the
queries' rows: the arithmetic and the traffic of a prediction, not its values.  The register table comes from
tools/kernel_regs.py (the built objects, celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_general_rev.py --regs-only) -->", "<!-- registers:end -->"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_general_rev.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::general_rev::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_general_rev<lanes per series, lower>`)."
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_general_rev.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built objects)\n\n" + block + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dense-series", type=int, default=4)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--regs-only", action="store_true")
    a = ap.parse_args()
    if a.regs_only:
        text = open(a.out).read() if a.out and os.path.exists(a.out) else ""
        text = with_registers(text)
        if a.out:
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import autograd as ag, ops, synth

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")

    def stats(ms):
        ms = sorted(ms)
        return ms[len(ms) // 2], ms[0], ms[-1]

    def alternate(runs, steps):
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        # events made beforehand and ONE synchronise at the end: the device never idles between steps
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for k in runs}
        torch.cuda.synchronize()
        for i in range(steps):
            for k, fn in runs.items():
                ev[k][i][0].record()
                fn()
                ev[k][i][1].record()
        torch.cuda.synchronize()
        return {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}

    def problem(B, N, J):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        ts = (t + (t[:, -1:] - t[:, :1]) / (3.0 * N)).contiguous()
        return t, c, av, U, V, y, ts

    N, J = (4096, 8) if not a.quick else (512, 8)
    lines = ["# ops.general_matmul_lower with its workspace and ops.general_matmul_lower_rev, one right-hand side", "",
             "One process, steps alternating between the two, %d timed steps each after %d warm-up steps; ms: median (min .. max)."
             % (a.steps, a.warmup), "",
             "| B x N x M x J | op | ms | algorithmic bytes per series | GB/s | of the 8 TB/s roofline |", "|---|---|---|---|---|---|"]
    for B in ((8192, 64) if not a.quick else (256, 64)):
        t, c, av, U, V, y, ts = problem(B, N, J)
        M = N
        Y = y[..., None].contiguous()
        Z, F = ops.general_matmul_lower(ts, t, c, U, V, Y, workspace=True, zero_z=True)
        bZ = torch.ones_like(Z)
        out = ops.general_matmul_lower_rev(ts, t, c, U, V, Y, F, bZ)
        runs = {"general_matmul_lower + workspace": lambda: ops.general_matmul_lower(ts, t, c, U, V, Y, Z=Z, F=F, zero_z=True),
                "general_matmul_lower_rev": lambda: ops.general_matmul_lower_rev(ts, t, c, U, V, Y, F, bZ, out=out)}
        doubles = {"general_matmul_lower + workspace": N * (3 + J) + M * (2 + 2 * J), "general_matmul_lower_rev": N * (3 + 2 * J) + M * (4 + 3 * J)}
        for op, st in alternate(runs, a.steps).items():
            nb = 8 * doubles[op]
            rate = nb * B / (st[0] * 1e-3)
            lines.append("| %d x %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% |"
                         % (B, N, M, J, op, st[0], st[1], st[2], nb, rate / 1e9, 100 * rate / PEAK))
            print(lines[-1], flush=True)
        del t, c, av, U, V, y, ts, Y, Z, F, bZ, out, runs
        torch.cuda.empty_cache()

    def dense_operator(t1, t2, c, U, V, lower):
        diff = t1[..., :, None] - t2[..., None, :]
        mask = diff >= 0 if lower else diff < 0
        lag = torch.where(mask, diff if lower else -diff, torch.zeros_like(diff))
        K = (U[..., :, None, :] * V[..., None, :, :] * torch.exp(-c[..., None, None, :] * lag[..., None])).sum(-1)
        return torch.where(mask, K, torch.zeros_like(K))

    def dense_mean(t, c, av, U, V, y, ts, Us, Vs):
        low = torch.tril(dense_operator(t, t, c, U, V, True), -1)
        K = low + low.transpose(-1, -2) + torch.diag_embed(av)
        alpha = torch.linalg.solve(K, y[..., None])
        return ((dense_operator(ts, t, c, Us, V, True) + dense_operator(ts, t, c, Vs, U, False)) @ alpha)[..., 0]

    B = 64
    t, c, av, U, V, y, ts = problem(B, N, J)
    Us, Vs = U.clone(), V.clone()
    args = [x.requires_grad_() for x in (t, c, av, U, V, y, ts, Us, Vs)]
    nd = min(a.dense_series, B)
    dargs = [x[:nd].detach().clone().requires_grad_() for x in args]

    def step(fn, xs):
        for x in xs:
            x.grad = None
        fn(*xs).sum().backward()

    res = alternate({"predict_mean, %d series" % B: lambda: step(ag.predict_mean, args),
                     "dense torch autograd, %d series" % nd: lambda: step(dense_mean, dargs)}, max(5, a.steps // 2))
    lines += ["", "# autograd.predict_mean forward + backward beside the dense route under torch autograd, N = M = %d, J = %d" % (N, J), "",
              "| step | ms per step: median (min .. max) | ms per series |", "|---|---|---|"]
    for (k, st), nb in zip(res.items(), (B, nd)):
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.4f |" % ((k,) + st + (st[0] / nb,)))
        print(lines[-1], flush=True)
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
