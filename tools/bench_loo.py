# -*- coding: utf-8 -*-
"""What the leave-one-out objective's gradient costs (csrc/c2_invdiag.hip with its workspace, csrc/c2_invdiag_rev.hip), on one
device, in ONE fresh process:

    python tools/bench_loo.py [--steps 20] [--out profiles/loo_grad.md] [--quick]
    python tools/bench_loo.py --regs-only --out profiles/loo_grad.md     # no GPU: refresh the register table

  (a) ops.inverse_diag with z, without and with the workspace, and ops.inverse_diag_rev beside ops.factor_rev and
      ops.solve_lower_rev (one right-hand side), at 8192 x 4096 x 8 and 64 x 4096 x 8, alternating step by step;
  (b) the whole autograd.loo_log_predictive_kernel step (value and every gradient: they come out of the forward call) beside
      ops.loglik_kernel_grad on the same kernel and data, at the same two shapes.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the tables give the median
(min .. max) of --steps steps and the algorithmic bytes as a fraction of the 8 TB/s roofline.  The workspace dominates them:
8 J (J + 1) bytes per row, written once by the forward sweep and read once by the reverse.  Per row, in doubles:
    inverse_diag + z            2 + 2 J (t, d, U, W) + 1 (z) + 2 (q, alpha)
    ... with the workspace      + J^2 + J
    inverse_diag_rev            7 (t, d, q, bq, z, alpha, balpha) + 2 J (U, W) + J^2 + J (workspace) + 3 (bt, bd, bz) + 2 J (bU, bW)
    factor_rev                  5 (t, a, d, bd; bt, ba out: 6) + 6 J (U, V, W, bW; bU, bV), its states replayed from d, W
    solve_lower_rev             5 (t, y, z, bz; bt, by out: 6) + 5 J (U, W, F; bU, bW)
The register table comes from tools/kernel_regs.py (the built objects, celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_loo.py --regs-only) -->", "<!-- registers:end -->"


def register_table():
    """Registers, LDS and scratch of the workspace forms of k_invdiag_group and of k_invdiag_rev, from tools/kernel_regs.py
    (None if the objects are not on this machine)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = [r for r in kernel_rows("c2_invdiag.o") if re.search(r"k_invdiag_group<\d+, \w+, true>", r[1])]
    rows += kernel_rows("c2_invdiag_rev.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::invdiag::", "").replace("c2::invdiag_rev::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_invdiag_group<lanes per series, with z, "
              "workspace>`, `k_invdiag_rev<lanes per series, with z>`)." % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_loo.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built objects)\n\n" + block + "\n"


def row_doubles(op, J):
    return {"inverse_diag + z": 5 + 2 * J, "inverse_diag + z, workspace": 5 + 3 * J + J * J,
            "inverse_diag_rev": 10 + 5 * J + J * J, "factor_rev": 6 + 6 * J, "solve_lower_rev": 6 + 5 * J}[op]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
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

    shapes = [(8192, 4096, 8), (64, 4096, 8)] if not a.quick else [(256, 512, 8), (64, 512, 8)]
    lines = ["# ops.inverse_diag with its workspace and ops.inverse_diag_rev beside factor_rev and solve_lower_rev", "",
             "One process, steps alternating between the ops, %d timed steps each after %d warm-up steps; ms: median (min .. max)."
             % (a.steps, a.warmup), "",
             "| B x N x J | op | ms | algorithmic bytes per row | GB/s | of the 8 TB/s roofline |", "|---|---|---|---|---|---|"]
    for B, N, J in shapes:
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, S, flag = ops.factor(t, c, av, U, V, workspace=True)
        assert int(flag.abs().sum()) == 0
        Y = y[..., None].contiguous()
        Z, F = ops.solve_lower(t, c, U, W, Y, workspace=True)
        z = Z[..., 0]
        q, alpha, ws = ops.inverse_diag(t, c, U, W, d, z=z, workspace=True)
        q0, alpha0 = torch.empty_like(q), torch.empty_like(q)
        bq = 0.5 / q + 0.5 * alpha * alpha / (q * q)
        balpha = -alpha / q
        out = ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, balpha)
        bW, bd, bz = out[3], out[4], out[5]
        bZ = bz[..., None].contiguous()
        runs = {"inverse_diag + z": lambda: ops.inverse_diag(t, c, U, W, d, q=q0, z=z, alpha=alpha0),
                "inverse_diag + z, workspace": lambda: ops.inverse_diag(t, c, U, W, d, q=q, z=z, alpha=alpha, ws=ws),
                "inverse_diag_rev": lambda: ops.inverse_diag_rev(t, c, U, W, d, z, q, alpha, ws, bq, balpha, out=out),
                "factor_rev": lambda: ops.factor_rev(t, c, av, U, V, d, W, S, bd, bW),
                "solve_lower_rev": lambda: ops.solve_lower_rev(t, c, U, W, Y, Z, F, bZ)}
        res = alternate(runs, a.steps)
        for op, st in res.items():
            nb = 8 * row_doubles(op, J)
            rate = nb * B * N / (st[0] * 1e-3)
            lines.append("| %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% |"
                         % (B, N, J, op, st[0], st[1], st[2], nb, rate / 1e9, 100 * rate / PEAK))
            print(lines[-1], flush=True)
        del t, c, av, U, V, y, d, W, S, Y, Z, F, z, q, alpha, ws, q0, alpha0, bq, balpha, out, bW, bd, bz, bZ, runs
        torch.cuda.empty_cache()

    lines += ["", "# The whole step: autograd.loo_log_predictive_kernel beside ops.loglik_kernel_grad (four SHO terms, J = 8)", "",
              "Value and every gradient per step (both produce them in the forward call).", "",
              "| B x N | step | ms per step: median (min .. max) |", "|---|---|---|"]
    tn = lambda v: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True)
    kernel = T.SHOTerm(S0=tn(1.0), w0=tn(3.0), Q=tn(2.0), regime="under") + T.SHOTerm(S0=tn(0.5), w0=tn(1.0), Q=tn(1.5), regime="under") \
        + T.SHOTerm(S0=tn(0.3), w0=tn(0.3), Q=tn(0.8), regime="under") + T.SHOTerm(S0=tn(0.2), w0=tn(6.0), Q=tn(4.0), regime="under")
    for B, N, _ in shapes:
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.cumsum(0.02 + 0.16 * torch.rand((B, N), dtype=torch.float64, device=dev, generator=gen), dim=1)
        yy = torch.sin(x) + 0.1 * torch.randn((B, N), dtype=torch.float64, device=dev, generator=gen)
        ye = torch.full((B, N), 0.3, dtype=torch.float64, device=dev)
        P = kernel.parameter_matrix(B).detach().contiguous()
        work = ops.loglik_kernel_workspace(kernel.program, B, N, dev)
        ll, outk, flag = ops.loglik_kernel_grad(kernel.program, P, x, ye, None, None, yy, work=work)
        assert int(flag.abs().sum()) == 0
        res = alternate({"loo_log_predictive_kernel": lambda: ag.loo_log_predictive_kernel(kernel, x, yy, yerr=ye),
                         "loglik_kernel_grad": lambda: ops.loglik_kernel_grad(kernel.program, P, x, ye, None, None, yy, work=work, out=outk)},
                        max(5, a.steps // 2))
        for k, st in res.items():
            lines.append("| %d x %d | %s | %.3f (%.3f .. %.3f) |" % ((B, N, k) + st))
            print(lines[-1], flush=True)
        del x, yy, ye, P, work, ll, outk
        torch.cuda.empty_cache()
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
