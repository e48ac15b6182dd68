# -*- coding: utf-8 -*-
"""What the fused whitened Gram matrix costs (csrc/c2_gram.hip) beside the route it replaces, on one device, in ONE fresh
process:

    python tools/bench_linear.py [--steps 20] [--out profiles/linear_model.md] [--quick]
    python tools/bench_linear.py --regs-only --out profiles/linear_model.md     # no GPU: refresh the register table

  (a) ops.whitened_gram against the composed route on the ops that were there before it -- ops.solve_lower writes
      Z = L^-1 [A | y], torch forms Z / d, torch.bmm reads both -- alternating step by step, at 8192 x 4096 x 8 and
      64 x 4096 x 8 (B x N x J) with Q = 4, 8, 16 columns ([A | y], A per series), every buffer of both routes allocated
      beforehand;
  (b) autograd.marginal_log_likelihood_kernel forward + backward (every hyper-parameter, jitter and mean) with four
      under-damped SHO terms (J = 8) and P = Q - 1 = 7 regressors at --step-series x 4096.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the tables give the median
(min .. max) and, for (a), the algorithmic bytes as a fraction of the 8 TB/s roofline.  In doubles per series:
    fused       N (2 J + Q + 2) read  (t, d; U, W; [A | y]),  Q^2 written
    composed    N (2 J + 3 Q + 2) at the least  (solve_lower: t, U, W, Y in, Z out; Z / d: Z, d in, a second (N, Q) array out
                -- counted as ONE pass over it here; bmm: both in), Q^2 written
so the bytes predict a time ratio fused / composed of (2 J + Q + 2) / (2 J + 3 Q + 2) or better.  The register table comes
from tools/kernel_regs.py (the built objects, celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_linear.py --regs-only) -->", "<!-- registers:end -->"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_gram.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in sorted(rows, key=lambda r: [int(v) for v in re.findall(r"\d+", re.sub(r"\(.*", "", r[1]))[-2:]]):
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::gram::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes over %d kernels (`k_gram<JR, QR>`: J and Q rounded up to 4, 8, 16 or 32; the group is "
              "max(JR, QR) lanes).  Spilled registers with no scratch are copies into accumulation registers: one wavefront per "
              "SIMD has 512 registers and these kernels use no MFMA." % (max(r[4] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_linear.py --regs-only --out <this file>` where the library was built)"
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
    ap.add_argument("--step-series", type=int, nargs="+", default=[64, 2048], help="batch sizes of the whole training step")
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
    from celerite2_amd import autograd as ag, ops, synth, terms as T

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

    def design(t, P):
        x = (t - t.mean(dim=-1, keepdim=True)) / (t[..., -1:] - t[..., :1])
        return (x[..., None] ** torch.arange(P, dtype=torch.float64, device=t.device)).contiguous()

    N, J = (4096, 8) if not a.quick else (512, 8)
    lines = ["# ops.whitened_gram beside ops.solve_lower + torch (Z / d, bmm)", "",
             "One process, steps alternating between the two routes, %d timed steps each after %d warm-up steps; ms: median "
             "(min .. max).  The two results agree to the standing criterion at every shape timed (checked before timing)."
             % (a.steps, a.warmup), "",
             "| B x N x J, Q | route | ms | algorithmic bytes per series | GB/s | of the 8 TB/s roofline | fused / composed: measured (bytes predict) |",
             "|---|---|---|---|---|---|---|"]
    for B in ((8192, 64) if not a.quick else (256, 64)):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, flag = ops.factor(t, c, av, U, V)
        assert int(flag.abs().sum()) == 0
        for Q in (4, 8, 16):
            A = design(t, Q - 1)
            Y = torch.cat([A, y[..., None]], dim=-1).contiguous()
            S, Z, X = ops.whitened_gram(t, c, U, W, d, A, y), torch.empty_like(Y), torch.empty_like(Y)
            S2 = torch.empty_like(S)

            def composed():
                ops.solve_lower(t, c, U, W, Y, Z=Z)
                torch.div(Z, d[..., None], out=X)
                torch.bmm(Z.transpose(1, 2), X, out=S2)

            composed()
            torch.cuda.synchronize()
            tol = 1e-10 * S2.abs() + 1e-12 * S2.abs().amax(dim=(1, 2), keepdim=True)
            assert bool(((S - S2).abs() <= tol).all()), "the two routes disagree"
            res = alternate({"fused": lambda: ops.whitened_gram(t, c, U, W, d, A, y, S=S), "composed": composed}, a.steps)
            doubles = {"fused": N * (2 * J + Q + 2) + Q * Q, "composed": N * (2 * J + 3 * Q + 2) + Q * Q}
            for op, st in res.items():
                nb = 8 * doubles[op]
                rate = nb * B / (st[0] * 1e-3)
                ratio = "%.2f (%.2f)" % (res["fused"][0] / res["composed"][0], (2 * J + Q + 2) / (2 * J + 3 * Q + 2)) if op == "fused" else ""
                lines.append("| %d x %d x %d, %d | %s | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% | %s |"
                             % (B, N, J, Q, op, st[0], st[1], st[2], nb, rate / 1e9, 100 * rate / PEAK, ratio))
                print(lines[-1], flush=True)
            del A, Y, S, Z, X, S2
        del t, c, av, U, V, y, d, W
        torch.cuda.empty_cache()

    P = 7
    lines += ["", "# autograd.marginal_log_likelihood_kernel forward + backward, N = %d, four under-damped SHO terms (J = 8), P = %d" % (N, P), "",
              "| series | ms per step: median (min .. max) | ms per series |", "|---|---|---|"]
    for B in (a.step_series if not a.quick else [16]):
        t, c, av, U, V, y = synth.device_batch_fast(1, B, N, J, dev)
        tn = lambda v: torch.full((B,), v, dtype=torch.float64, device=dev).requires_grad_()
        params = [tn(v) for k in range(4) for v in (0.5 + 0.2 * k, 1.0 + 0.7 * k, 2.0 + k)]
        kernel = T.SHOTerm(S0=params[0], w0=params[1], Q=params[2], regime="under")
        for k in range(1, 4):
            kernel = kernel + T.SHOTerm(S0=params[3 * k], w0=params[3 * k + 1], Q=params[3 * k + 2], regime="under")
        jitter, mean = tn(0.1), tn(0.0)
        A, yerr = design(t, P), torch.full_like(y, 0.3)
        leaves = params + [jitter, mean]

        def step():
            for x in leaves:
                x.grad = None
            ag.marginal_log_likelihood_kernel(kernel, t, y, A, yerr=yerr, jitter=jitter, mean=mean).sum().backward()

        st = alternate({"step": step}, max(5, a.steps // 2))["step"]
        lines.append("| %d | %.3f (%.3f .. %.3f) | %.4f |" % ((B,) + st + (st[0] / B,)))
        print(lines[-1], flush=True)
        del t, c, av, U, V, y, A, yerr, kernel, params, leaves
        torch.cuda.empty_cache()
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
