# -*- coding: utf-8 -*-
"""What the linear-time inverse diagonal costs (csrc/c2_invdiag.hip), on one device, in ONE fresh process:

    python tools/bench_inverse_diag.py [--steps 20] [--out profiles/inverse_diag.md] [--quick]
    python tools/bench_inverse_diag.py --regs-only --out profiles/inverse_diag.md     # no GPU: refresh the register table

  (a) ops.inverse_diag, with and without z, at 8192 and 65536 x 4096 x 8 and at 64 x 4096 x {8, 16, 32}; beside it, in the
      same process and alternating step by step, ops.solve_upper with one right-hand side (the existing kernel with the same
      row traffic) and ops.factor (the existing kernel with the same state size).
  (b) gp.predict_observed(return_var=True) against the existing gp.predict(return_var=True) at 16 x 4096 x 8 (the old path
      needs 2 GB of cross-covariance there), and predict_observed alone at 65536 x 4096 x 8, where the old path cannot
      allocate.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the tables give the median (min .. max) of --steps steps,
the algorithmic bytes -- 8 (2 + 2 J) per row for t, d, U, W, plus 8 for z and 8 each for q and alpha -- as a fraction of the
8 TB/s roofline, and the ratio to solve_upper.  The register table comes from tools/kernel_regs.py (the built object,
celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_inverse_diag.py --regs-only) -->", "<!-- registers:end -->"


def register_table():
    """Registers, LDS and scratch of the kernels of c2_invdiag.o, from tools/kernel_regs.py (None if the object is not on this
    machine)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_invdiag.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::invdiag::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d (to accumulation registers where scratch is 0) over %d kernels "
              "(`group<lanes per series, with z, workspace of the reverse pass: tools/bench_loo.py>`)."
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_inverse_diag.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def row_bytes(J, z):
    return 8 * (2 + 2 * J) + (8 if z else 0) + 8 + (8 if z else 0)


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
    from celerite2_amd import gp as G, ops, synth, terms as T

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")

    def stats(ms):
        ms = sorted(ms)
        return ms[len(ms) // 2], ms[0], ms[-1]

    def alternate(runs, steps):
        for _ in range(a.warmup):
            for fn in runs.values():
                fn()
        # events made beforehand and ONE synchronise at the end: the device never idles between steps (an idle millisecond
        # costs the next kernels up to a third of their speed: profiles/r05_clock_ramp.md)
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for k in runs}
        torch.cuda.synchronize()
        for i in range(steps):
            for k, fn in runs.items():
                ev[k][i][0].record()
                fn()
                ev[k][i][1].record()
        torch.cuda.synchronize()
        return {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}

    shapes = [(8192, 4096, 8), (65536, 4096, 8), (64, 4096, 8), (64, 4096, 16), (64, 4096, 32)]
    if a.quick:
        shapes = [(256, 512, 8), (64, 512, 16)]
    lines = ["# ops.inverse_diag beside solve_upper (one right-hand side) and factor", "",
             "One process, steps alternating between the ops, %d timed steps each after %d warm-up steps; ms: median (min .. max)."
             % (a.steps, a.warmup), "",
             "| B x N x J | op | ms | algorithmic bytes per row | GB/s | of the 8 TB/s roofline | time / solve_upper |", "|---|---|---|---|---|---|---|"]
    for B, N, J in shapes:
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W = torch.empty_like(av), torch.empty_like(V)
        d, W, flag = ops.factor(t, c, av, U, V, d=d, W=W)
        assert int(flag.abs().sum()) == 0
        Y = y[..., None].contiguous()
        z = ops.solve_lower(t, c, U, W, Y)
        zu = torch.empty_like(z)
        del Y
        q, alpha = torch.empty_like(d), torch.empty_like(d)
        zv = z[..., 0]

        runs = {"factor": lambda: ops.factor(t, c, av, U, V, d=d, W=W),
                "solve_upper": lambda: ops.solve_upper(t, c, U, W, z, Z=zu),
                "inverse_diag": lambda: ops.inverse_diag(t, c, U, W, d, q=q),
                "inverse_diag + z": lambda: ops.inverse_diag(t, c, U, W, d, q=q, z=zv, alpha=alpha)}
        res = alternate(runs, a.steps)
        su = res["solve_upper"][0]
        for op, st in res.items():
            if op == "factor":
                nb = 8 * (2 + 2 * J) + 8 * (1 + J)          # t, a, U, V in; d, W out
            elif op == "solve_upper":
                nb = 8 * (1 + 2 * J) + 16                    # t, U, W, y in; z out
            else:
                nb = row_bytes(J, op.endswith("z"))
            rate = nb * B * N / (st[0] * 1e-3)
            lines.append("| %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% | %.2f |"
                         % (B, N, J, op, st[0], st[1], st[2], nb, rate / 1e9, 100 * rate / PEAK, st[0] / su))
            print(lines[-1], flush=True)
        if (B, N, J) == (65536, 4096, 8):   # the frontend at the shape the old path cannot allocate (134 MB per series)
            kernel = T.SHOTerm(S0=1.0, w0=3.0, Q=2.0) + T.SHOTerm(S0=0.5, w0=1.0, Q=1.5) + T.SHOTerm(S0=0.3, w0=0.3, Q=0.8) \
                + T.SHOTerm(S0=0.2, w0=6.0, Q=4.0)
            del U, V, W, z, zu, d, q, alpha, zv, runs
            torch.cuda.empty_cache()
            gp = G.GaussianProcess(kernel, t, diag=torch.full((B, N), 0.1, dtype=torch.float64, device=dev), check_sorted=False)
            st = alternate({"big": lambda: gp.predict_observed(y, return_var=True)}, max(3, a.steps // 4))["big"]
            big = "gp.predict_observed(return_var=True) at %d x %d x %d completes: %.2f ms (%.2f .. %.2f) per call (solve_lower + inverse_diag + the elementwise tail)" % ((B, N, gp._U.shape[-1]) + st)
            print(big, flush=True)
            del gp
        else:
            big = None
        if big:
            lines_big = big
        del t, c, av, y
        torch.cuda.empty_cache()

    # (b) the frontend against the existing O(N^2) path
    B, N = (16, 4096) if not a.quick else (4, 256)
    kernel = T.SHOTerm(S0=1.0, w0=3.0, Q=2.0) + T.SHOTerm(S0=0.5, w0=1.0, Q=1.5) + T.SHOTerm(S0=0.3, w0=0.3, Q=0.8) \
        + T.SHOTerm(S0=0.2, w0=6.0, Q=4.0)
    gen = torch.Generator(device=dev).manual_seed(7)
    x = torch.cumsum(0.02 + 0.16 * torch.rand((B, N), dtype=torch.float64, device=dev, generator=gen), dim=1)
    yy = torch.sin(x) + 0.1 * torch.randn((B, N), dtype=torch.float64, device=dev, generator=gen)
    gp = G.GaussianProcess(kernel, x, diag=torch.full((B, N), 0.1, dtype=torch.float64, device=dev))
    res = alternate({"new": lambda: gp.predict_observed(yy, return_var=True), "old": lambda: gp.predict(yy, return_var=True)},
                    max(5, a.steps // 4))
    mn, vn = gp.predict_observed(yy, return_var=True)
    mo, vo = gp.predict(yy, return_var=True)
    dv = float((vn - vo).abs().max() / vo.abs().max())
    lines += ["", "# gp.predict_observed(return_var=True) against gp.predict(return_var=True), %d x %d x %d" % (B, N, gp._U.shape[-1]), "",
              "| path | ms per call: median (min .. max) |", "|---|---|",
              "| predict_observed: solve_lower + inverse_diag, O(N J^2) | %.3f (%.3f .. %.3f) |" % res["new"],
              "| predict: N x N cross-covariance, solve_lower with N right-hand sides, column sums, O(N^2 J) | %.3f (%.3f .. %.3f) |" % res["old"],
              "", "ratio old / new: %.1f; largest difference of the two variances: %.2e of the largest variance" % (res["old"][0] / res["new"][0], dv)]
    if not a.quick:
        lines += ["", lines_big]
    assert res["new"][0] < res["old"][0], "predict_observed is O(N J^2) against O(N^2 J): anything else is a bug"
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
