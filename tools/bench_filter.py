# -*- coding: utf-8 -*-
"""What appending rows to a filter state costs (csrc/c2_filter.hip), on one device, in ONE fresh process:

    python tools/bench_filter.py [--steps 20] [--out profiles/filter.md] [--quick]
    python tools/bench_filter.py --regs-only --out profiles/filter.md     # no GPU: refresh the register table

ops.filter_append of M in {1, 4, 16} new rows at B = 65536 series of width J in {2, 8} whose first N = 4096 rows are in the
state, beside the only route there was before it: ops.factor + ops.solve_lower over all N + M rows.  The two alternate step by
step in the same process; before timing, the appended d, z are held to the refactored ones by the standing criterion.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the table gives the median
(min .. max) of --steps steps, and the bytes an append moves per series -- the state read and written, 16 SW with
SW = 4 + J + J^2, and 8 (5 + 3 J) per row for t, a, y, U, V in and d, z, W out -- as a fraction of the 8 TB/s roofline.  The
register table comes from tools/kernel_regs.py (the built object, celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_filter.py --regs-only) -->", "<!-- registers:end -->"
NOT_MEASURED = "# ops.filter_append beside ops.factor + ops.solve_lower of the whole series\n\nNot measured yet: run `python tools/bench_filter.py --out profiles/filter.md` on an MI355X.\n"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_filter.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::filter::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_filter<lanes per series, mode>`: mode 0 append, "
              "1 absorb, 2 forecast)." % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_filter.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def append_bytes(J, M):
    return 16 * (4 + J + J * J) + 8 * (5 + 3 * J) * M


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
    lines = ["# ops.filter_append beside ops.factor + ops.solve_lower of the whole series", "",
             "B = %d series with N = %d rows in the state, M new rows.  One process, steps alternating between the two routes, %d "
             "timed steps each after %d warm-up steps; ms: median (min .. max).  The appended d, z meet the standing criterion against "
             "the refactored ones at every shape timed (checked before timing)." % (B, N, a.steps, a.warmup), "",
             "| J | M | route | ms | bytes per series | GB/s | of the 8 TB/s roofline | refactor / append |", "|---|---|---|---|---|---|---|---|"]
    findings = []
    for J in (2, 8):
        for M in (1, 4, 16):
            t, c, av, U, V, y = synth.device_batch_fast(0, B, N + M, J, dev)
            d, W = torch.empty_like(av), torch.empty_like(V)
            d, W, flag = ops.factor(t, c, av, U, V, d=d, W=W)
            assert int(flag.abs().sum()) == 0
            Y = y[..., None].contiguous()
            z = ops.solve_lower(t, c, U, W, Y)
            head = lambda x: x[:, :N].contiguous()
            state = ops.filter_absorb(ops.filter_init(B, J, dev), head(t), c, head(W), head(d), head(z[..., 0]))
            tail = lambda x: x[:, N:].contiguous()
            tm, am, Um, Vm, ym = (tail(x) for x in (t, av, U, V, y))
            out, dm, Wm, zm = torch.empty_like(state), torch.empty_like(am), torch.empty_like(Vm), torch.empty_like(ym)
            ops.filter_append(state, tm, c, am, Um, Vm, ym, out=out, d=dm, W=Wm, z=zm)
            e = max(worst(dm, d[:, N:]), worst(zm, z[:, N:, 0]))
            assert e <= 1.0, ("append against refactoring", J, M, e)
            Z = torch.empty_like(z)

            def refactor():
                ops.factor(t, c, av, U, V, d=d, W=W)
                ops.solve_lower(t, c, U, W, Y, Z=Z)

            res = alternate({"append": lambda: ops.filter_append(state, tm, c, am, Um, Vm, ym, out=out, d=dm, W=Wm, z=zm),
                             "refactor": refactor}, a.steps)
            ap_ms, rf_ms = res["append"], res["refactor"]
            nb = append_bytes(J, M)
            rate = nb * B / (ap_ms[0] * 1e-3)
            lines.append("| %d | %d | append | %.4f (%.4f .. %.4f) | %d | %.0f | %.1f %% | %.0f |"
                         % (J, M, ap_ms[0], ap_ms[1], ap_ms[2], nb, rate / 1e9, 100 * rate / PEAK, rf_ms[0] / ap_ms[0]))
            nb = (8 * (3 + 3 * J) + 8 * (3 + 2 * J)) * (N + M)   # factor: t, a, U, V in, d, W out; solve_lower: t, U, W, y in, z out
            rate = nb * B / (rf_ms[0] * 1e-3)
            lines.append("| %d | %d | factor + solve_lower, %d rows | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% | |"
                         % (J, M, N + M, rf_ms[0], rf_ms[1], rf_ms[2], nb, rate / 1e9, 100 * rate / PEAK))
            print("\n".join(lines[-2:]), flush=True)
            if M == 1 and ap_ms[0] > rf_ms[0]:   # the one condition on this kernel; a finding to report, not to tune away
                findings.append("FINDING: at J = %d an append of ONE row (%.4f ms) takes longer than the refactoring it replaces "
                                "(%.3f ms)." % (J, ap_ms[0], rf_ms[0]))
            del t, c, av, U, V, y, d, W, z, Z, Y, state, out, tm, am, Um, Vm, ym, dm, Wm, zm
            torch.cuda.empty_cache()
    lines += [""] + (findings or ["An append of one row is faster than the refactoring it replaces at both widths."])
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
