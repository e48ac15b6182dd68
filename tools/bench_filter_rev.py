# -*- coding: utf-8 -*-
"""What the gradient of a streaming append costs (csrc/c2_filter_rev.hip), on one device, in ONE fresh process:

    python tools/bench_filter_rev.py [--steps 20] [--out profiles/filter_rev.md] [--quick]
    python tools/bench_filter_rev.py --regs-only --out profiles/filter_rev.md     # no GPU: refresh the register table

ops.filter_append_rev of M in {1, 4, 16} new rows at B = 65536 series of width J in {2, 8} whose first N = 4096 rows are in the
state -- alone, and behind the ops.filter_append it reverses -- beside the only route to the same gradient there was before it:
ops.loglik_grad over all N + M rows.  The routes alternate step by step in the same process; before timing, the ba and by the
reverse gives for the new rows under the log-likelihood's cotangent are held to those of loglik_grad by the standing criterion.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the table gives the median
(min .. max) of --steps steps, and the bytes the reverse moves per series -- three states (state_in and bstate_out read,
bstate_in written), 24 SW with SW = 4 + J + J^2, bc, and per row t, d, z, U, W and the three row cotangents in, the five row
gradients out and the J + J^2 words of ws written and read back -- as a fraction of the 8 TB/s roofline.  The register table
comes from tools/kernel_regs.py (the built object, celerite2_amd/build)."""
import argparse
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_filter_rev.py --regs-only) -->", "<!-- registers:end -->"
TITLE = "# ops.filter_append_rev beside ops.loglik_grad of the whole series"
NOT_MEASURED = TITLE + "\n\nNot measured yet: run `python tools/bench_filter_rev.py --out profiles/filter_rev.md` on an MI355X.\n"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_filter_rev.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::filter_rev::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_filter_rev<lanes per series>`)."
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_filter_rev.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def rev_bytes(J, M):
    return 24 * (4 + J + J * J) + 8 * J + M * (8 * (3 + 2 * J) + 8 * (2 + J) + 8 * (3 + 2 * J) + 16 * (J + J * J))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--regs-only", action="store_true")
    a = ap.parse_args()
    if a.regs_only:
        text = open(a.out).read() if a.out and os.path.exists(a.out) else NOT_MEASURED
        text = with_registers(text)
        if a.out:
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import ops, synth

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

    def worst(x, xo):   # the standing criterion, as tests/inverse_diag_ref.py::err
        return float(((x - xo).abs() / (1e-10 * xo.abs() + 1e-12 * xo.abs().max())).max())

    B, N = (65536, 4096) if not a.quick else (512, 256)
    lines = [TITLE, "",
             "B = %d series with N = %d rows in the state, M new rows; the cotangent is that of the log-likelihood of the state "
             "behind them.  One process, steps alternating between the routes, %d timed steps each after %d warm-up steps; ms: median "
             "(min .. max).  The reverse's ba, by of the new rows meet the standing criterion against loglik_grad's at every shape "
             "timed (checked before timing)." % (B, N, a.steps, a.warmup), "",
             "| J | M | route | ms | bytes per series | GB/s | of the 8 TB/s roofline | reverse / append | loglik_grad / (append + reverse) |",
             "|---|---|---|---|---|---|---|---|---|"]
    findings = []
    for J in (2, 8):
        for M in (1, 4, 16):
            t, c, av, U, V, y = synth.device_batch_fast(0, B, N + M, J, dev)
            d, W, flag = ops.factor(t, c, av, U, V)
            assert int(flag.abs().sum()) == 0
            z = ops.solve_lower(t, c, U, W, y[..., None].contiguous())[..., 0]
            head = lambda x: x[:, :N].contiguous()
            state = ops.filter_absorb(ops.filter_init(B, J, dev), head(t), c, head(W), head(d), head(z))
            del d, W, z
            torch.cuda.empty_cache()
            tail = lambda x: x[:, N:].contiguous()
            tm, am, Um, Vm, ym = (tail(x) for x in (t, av, U, V, y))
            out, dm, Wm, zm = torch.empty_like(state), torch.empty_like(am), torch.empty_like(Vm), torch.empty_like(ym)
            _, _, _, _, fl = ops.filter_append(state, tm, c, am, Um, Vm, ym, out=out, d=dm, W=Wm, z=zm)
            assert int(fl.abs().sum()) == 0
            bstate = torch.zeros_like(state)
            bstate[:, 1], bstate[:, 2], bstate[:, 3] = -0.5 * math.log(2 * math.pi), -0.5, -0.5
            ws = torch.empty((B, M, ops.filter_rev_workspace_words(J)), dtype=torch.float64, device=dev)
            grads = ops.filter_append_rev(state, tm, c, Um, Wm, dm, zm, fl, bstate, ws=ws)
            work = ops.loglik_grad_workspace(B, N + M, J, dev)
            _, whole, flag = ops.loglik_grad(t, c, av, U, V, y, work=work)
            assert int(flag.abs().sum()) == 0
            e = max(worst(grads[3], whole[2][:, N:]), worst(grads[6], whole[5][:, N:]))
            assert e <= 1.0, ("reverse against loglik_grad", J, M, e)

            def append():
                ops.filter_append(state, tm, c, am, Um, Vm, ym, out=out, d=dm, W=Wm, z=zm)

            def reverse():
                ops.filter_append_rev(state, tm, c, Um, Wm, dm, zm, fl, bstate, ws=ws, out=grads)

            def both():
                append()
                reverse()

            res = alternate({"append": append, "reverse": reverse, "both": both,
                             "whole": lambda: ops.loglik_grad(t, c, av, U, V, y, work=work, out=whole)}, a.steps)
            ap_ms, rv_ms, bo_ms, wh_ms = res["append"], res["reverse"], res["both"], res["whole"]
            nb = rev_bytes(J, M)
            rate = nb * B / (rv_ms[0] * 1e-3)
            lines.append("| %d | %d | reverse | %.4f (%.4f .. %.4f) | %d | %.0f | %.1f %% | %.2f | |"
                         % (J, M, rv_ms[0], rv_ms[1], rv_ms[2], nb, rate / 1e9, 100 * rate / PEAK, rv_ms[0] / ap_ms[0]))
            lines.append("| %d | %d | append | %.4f (%.4f .. %.4f) | | | | | |" % (J, M, ap_ms[0], ap_ms[1], ap_ms[2]))
            lines.append("| %d | %d | append + reverse | %.4f (%.4f .. %.4f) | | | | | %.0f |"
                         % (J, M, bo_ms[0], bo_ms[1], bo_ms[2], wh_ms[0] / bo_ms[0]))
            lines.append("| %d | %d | loglik_grad, %d rows | %.3f (%.3f .. %.3f) | | | | | |" % (J, M, N + M, wh_ms[0], wh_ms[1], wh_ms[2]))
            print("\n".join(lines[-4:]), flush=True)
            if bo_ms[0] > wh_ms[0]:   # the one condition on this kernel; a finding to report, not to tune away
                findings.append("FINDING: at J = %d, M = %d append + reverse (%.4f ms) takes longer than loglik_grad over the whole "
                                "series (%.3f ms)." % (J, M, bo_ms[0], wh_ms[0]))
            del t, c, av, U, V, y, state, out, tm, am, Um, Vm, ym, dm, Wm, zm, bstate, ws, grads, work, whole
            torch.cuda.empty_cache()
    lines += [""] + (findings or ["Append + reverse of the new rows is faster than loglik_grad over the whole series at every shape timed."])
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
