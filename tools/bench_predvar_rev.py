# -*- coding: utf-8 -*-
"""What the reverse of explained_variance costs (csrc/c2_predvar_rev.hip), on one device, in ONE fresh process:

    python tools/bench_predvar_rev.py [--steps 20] [--out profiles/predvar_rev.md] [--quick]
    python tools/bench_predvar_rev.py --regs-only --out profiles/predvar_rev.md     # no GPU: refresh the register table

  (a) ops.explained_variance without and with its workspace and ops.explained_variance_rev at 8192 x 4096 x 4096 x 8 and
      64 x 4096 x 4096 x 8 (B x N x M x J), alternating step by step (the large batch in chunks of --chunk series: the
      workspace is 16 N J^2 bytes, 4.2 MB, per series);
  (b) autograd.predictive_log_density forward + backward (every gradient) at 64 x 4096 x 4096 x 8 beside the dense route
      under torch autograd on the same device -- K from the semiseparable form, linalg.solve against the N x M
      cross-covariance -- which is run on --dense-series series at a time and reported per series.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the tables give the median
(min .. max) and, for (a), the algorithmic bytes as a fraction of the 8 TB/s roofline.  In doubles, both sweeps together:
    explained_variance                 N (4 + 4 J) (t, d twice; W twice, U, W)   + M (4 + 4 J)  (ts twice, r out / in / out; Us, Vs, X out, X in)
    explained_variance + workspace     the same + 2 N J^2                          (Sws, Rws out)
    explained_variance_rev             N (7 + 6 J + 2 J^2)                         + M (7 + 5 J)
      (t, d twice, bd out / in / out, bt out / in / out; W, U, bU, bW out | W, bW in / out; Rws, Sws)
      (ts, br twice, bts out / in / out; X, bVs out | Us, bVs, bUs out)
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
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_predvar_rev.py --regs-only) -->", "<!-- registers:end -->"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_predvar_rev.o") + [r for r in kernel_rows("c2_predvar.o") if ", true>" in r[1]]
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::predvar_rev::", "").replace("c2::predvar::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes over %d kernels (`k_predvar_rev<lanes per series, BACK>`: BACK = true is pass A, and "
              "`k_predvar<lanes per series, BACK, WS = true>`, the forward sweeps that store their states).  Spilled registers "
              "with no scratch are copies into accumulation registers: one wavefront per SIMD has 512 registers and these "
              "kernels use no MFMA." % (max(r[4] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_predvar_rev.py --regs-only --out <this file>` where the library was built)"
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
    ap.add_argument("--chunk", type=int, default=2048, help="series per call of the large batch (8.6 GB of workspace at 2048)")
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
    M = N
    lines = ["# ops.explained_variance without and with its workspace, and ops.explained_variance_rev", "",
             "One process, steps alternating between the three, %d timed steps each after %d warm-up steps; ms: median (min .. max). "
             "A batch beyond %d series runs in chunks of that many (one workspace, reused), the chunks' times added." % (a.steps, a.warmup, a.chunk), "",
             "| B x N x M x J | op | ms | algorithmic bytes per series | GB/s | of the 8 TB/s roofline |", "|---|---|---|---|---|---|"]
    doubles = {"explained_variance": N * (4 + 4 * J) + M * (4 + 4 * J),
               "explained_variance + workspace": N * (4 + 4 * J + 2 * J * J) + M * (4 + 4 * J),
               "explained_variance_rev": N * (7 + 6 * J + 2 * J * J) + M * (7 + 5 * J)}
    for B in ((8192, 64) if not a.quick else (256, 64)):
        Bc = min(B, a.chunk)
        t, c, av, U, V, y, ts = problem(Bc, N, J)
        d, W, flag = ops.factor(t, c, av, U, V)
        r, work = torch.empty((Bc, M), dtype=torch.float64, device=dev), torch.empty((Bc, M, J), dtype=torch.float64, device=dev)
        _, ws = ops.explained_variance(t, ts, c, U, W, d, U, V, out=r, work=work, workspace=True)
        br = torch.ones_like(r)
        out = ops.explained_variance_rev(t, ts, c, U, W, d, U, V, work, ws, br)
        runs = {"explained_variance": lambda: ops.explained_variance(t, ts, c, U, W, d, U, V, out=r, work=work),
                "explained_variance + workspace": lambda: ops.explained_variance(t, ts, c, U, W, d, U, V, out=r, work=work, ws=ws),
                "explained_variance_rev": lambda: ops.explained_variance_rev(t, ts, c, U, W, d, U, V, work, ws, br, out=out)}
        for op, st in alternate(runs, a.steps).items():
            st = tuple(s * (B / Bc) for s in st)
            nb = 8 * doubles[op]
            rate = nb * B / (st[0] * 1e-3)
            lines.append("| %d x %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% |"
                         % (B, N, M, J, op, st[0], st[1], st[2], nb, rate / 1e9, 100 * rate / PEAK))
            print(lines[-1], flush=True)
        del t, c, av, U, V, y, ts, d, W, r, work, ws, br, out, runs
        torch.cuda.empty_cache()

    def dense_operator(t1, t2, c, U, V, lower):
        diff = t1[..., :, None] - t2[..., None, :]
        mask = diff >= 0 if lower else diff < 0
        lag = torch.where(mask, diff if lower else -diff, torch.zeros_like(diff))
        K = (U[..., :, None, :] * V[..., None, :, :] * torch.exp(-c[..., None, None, :] * lag[..., None])).sum(-1)
        return torch.where(mask, K, torch.zeros_like(K))

    def dense_density(t, c, av, U, V, y, ts, Us, Vs, k0, ys):
        low = torch.tril(dense_operator(t, t, c, U, V, True), -1)
        K = low + low.transpose(-1, -2) + torch.diag_embed(av)
        Ks = dense_operator(ts, t, c, Us, V, True) + dense_operator(ts, t, c, Vs, U, False)      # (B, M, N)
        sol = torch.linalg.solve(K, torch.cat([y[..., None], Ks.transpose(-1, -2)], dim=-1))
        mu = (Ks @ sol[..., :1])[..., 0]
        var = k0[:, None] - (Ks.transpose(-1, -2) * sol[..., 1:]).sum(-2)
        return -0.5 * ((ys - mu) ** 2 / var + torch.log(var)).sum(-1)

    B = 64
    t, c, av, U, V, y, ts = problem(B, N, J)
    Us, Vs = U.clone(), V.clone()
    k0 = av.max(dim=1).values.contiguous()   # (any k0 that keeps the variance positive: the cost does not depend on it)
    ys = torch.zeros((B, M), dtype=torch.float64, device=dev)
    args = [x.requires_grad_() for x in (t, c, av, U, V, y, ts, Us, Vs, k0, ys)]
    nd = min(a.dense_series, B)
    dargs = [x[:nd].detach().clone().requires_grad_() for x in args]

    def step(fn, xs):
        for x in xs:
            x.grad = None
        fn(*xs).sum().backward()

    res = alternate({"predictive_log_density, %d series" % B: lambda: step(ag.predictive_log_density, args),
                     "dense torch autograd, %d series" % nd: lambda: step(dense_density, dargs)}, max(5, a.steps // 2))
    lines += ["", "# autograd.predictive_log_density forward + backward beside the dense route under torch autograd, N = M = %d, J = %d" % (N, J), "",
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
