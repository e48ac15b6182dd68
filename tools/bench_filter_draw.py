# -*- coding: utf-8 -*-
"""What joint draws of the future from a filter state cost (csrc/c2_filter_draw.hip), on one device, in ONE fresh process:

    python tools/bench_filter_draw.py [--steps 20] [--out profiles/filter_draw.md] [--quick]
    python tools/bench_filter_draw.py --regs-only --out profiles/filter_draw.md     # no GPU: refresh the register table

ops.filter_draw of K in {1, 16, 64} paths over M in {1, 4, 16} query rows at B = 65536 series of width J in {2, 8} whose
first N = 4096 rows are in the state, beside the best route the older ops give: the state replicated K times (a batch of B K
series) and, row by row, ops.filter_forecast of one row, torch.randn and y = mu + sqrt(var) eps, ops.filter_append of that row
-- 2 M kernel launches and K copies of S.  Where the B K replicated states and their rows exceed --baseline-budget-gib the
baseline runs on fewer series and its time is scaled to B (said in the table).  The two routes alternate step by step in the
same process; before timing, with the same normals given to both, the fused paths are held to the baseline's by the standing
criterion.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the table gives the median
(min .. max) of --steps steps of whole calls, and the bytes the fused call moves per series -- the state read, 8 SW with
SW = 4 + J + J^2, per row 8 (3 + 2 J) for t, a, U, V in and d out, and 16 K for eps in and paths out -- as a fraction of the
8 TB/s roofline.  The register table comes from tools/kernel_regs.py (the built object, celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
TITLE = "# ops.filter_draw beside forecast + randn + append per row on K replicated states"
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_filter_draw.py --regs-only) -->", "<!-- registers:end -->"
NOT_MEASURED = TITLE + "\n\nNot measured yet: run `python tools/bench_filter_draw.py --out profiles/filter_draw.md` on an MI355X.\n"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_filter_draw.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::filter_draw::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_filter_draw<lanes per series>`)."
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_filter_draw.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def draw_bytes(J, M, K):
    return 8 * (4 + J + J * J) + 8 * (3 + 2 * J) * M + 16 * M * K


def baseline_bytes(J, M):
    """Device bytes one replicated series holds in the baseline: two states (the replica and the one being advanced), the M
    rows of t, a, U, V, and one row of mu, var, eps, y, d, z, W."""
    return 16 * (4 + J + J * J) + 8 * (2 + 2 * J) * M + 8 * (6 + J)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-budget-gib", type=float, default=24.0)
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
             "B = %d series with N = %d rows in the state, K joint draws of M query rows behind them.  One process, steps alternating "
             "between the two routes, %d timed steps each after %d warm-up steps; ms of whole calls: median (min .. max).  Given the "
             "same normals, the fused paths meet the standing criterion against the baseline's at every shape timed (checked before "
             "timing).  Baseline: the state replicated K times, then per row `ops.filter_forecast` (1 row), `torch.randn`, "
             "y = mu + sqrt(var) eps, `ops.filter_append` (1 row)." % (B, N, a.steps, a.warmup), "",
             "| J | M | K | fused ms | bytes per series | GB/s | of the 8 TB/s roofline | baseline ms | baseline series | baseline / fused |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for J in (2, 8):
        for M in (1, 4, 16):
            t, c, av, U, V, y = synth.device_batch_fast(0, B, N + M, J, dev)
            d, W = torch.empty_like(av), torch.empty_like(V)
            d, W, flag = ops.factor(t, c, av, U, V, d=d, W=W)
            assert int(flag.abs().sum()) == 0
            z = ops.solve_lower(t, c, U, W, y[..., None].contiguous())
            head = lambda x: x[:, :N].contiguous()
            state = ops.filter_absorb(ops.filter_init(B, J, dev), head(t), c, head(W), head(d), head(z[..., 0]))
            tail = lambda x: x[:, N:].contiguous()
            tm, am, Um, Vm = (tail(x) for x in (t, av, U, V))
            del t, av, U, V, y, d, W, z
            torch.cuda.empty_cache()
            for K in (1, 16, 64):
                eps = torch.randn((B, M, K), dtype=torch.float64, device=dev)
                paths, dm = torch.empty_like(eps), torch.empty_like(am)
                _, _, flag = ops.filter_draw(state, tm, c, am, Um, Vm, eps, paths=paths, d=dm)
                assert int(flag.abs().sum()) == 0

                # the baseline: Bb series (all of them where B K replicas fit the budget), each replicated K times
                Bb = min(B, max(1, int(a.baseline_budget_gib * 2**30 / (baseline_bytes(J, M) * K))))
                rep = lambda x: x[:Bb].repeat_interleave(K, dim=0).contiguous()
                srep, crep = rep(state), rep(c)
                rows = [tuple(rep(x[:, m:m + 1]) for x in (tm, am, Um, Vm)) for m in range(M)]
                work = torch.empty_like(srep)
                mu, var, yk, e1, dk, zk = (torch.empty((Bb * K, 1), dtype=torch.float64, device=dev) for _ in range(6))
                Wk = torch.empty((Bb * K, 1, J), dtype=torch.float64, device=dev)

                def baseline(normals=None):
                    out = []
                    for m, (t1, a1, U1, V1) in enumerate(rows):
                        st = srep if m == 0 else work
                        ops.filter_forecast(st, t1, crep, a1, U1, mu=mu, var=var)
                        if normals is None:
                            torch.randn(e1.shape, dtype=torch.float64, device=dev, out=e1)
                        else:
                            e1.copy_(normals[:Bb, m].reshape(Bb * K, 1))
                        torch.addcmul(mu, torch.sqrt(var), e1, out=yk)
                        ops.filter_append(st, t1, crep, a1, U1, V1, yk, out=work, d=dk, W=Wk, z=zk)
                        if normals is not None:
                            out.append(yk.reshape(Bb, K).clone())
                    return out

                ref = torch.stack(baseline(eps), dim=1)   # (Bb, M, K)
                e = worst(paths[:Bb], ref)
                assert e <= 1.0, ("fused against forecast + append per row", J, M, K, e)

                res = alternate({"fused": lambda: ops.filter_draw(state, tm, c, am, Um, Vm, eps, paths=paths, d=dm),
                                 "baseline": baseline}, a.steps)
                fu, ba = res["fused"], res["baseline"]
                scale = B / Bb
                nb = draw_bytes(J, M, K)
                rate = nb * B / (fu[0] * 1e-3)
                lines.append("| %d | %d | %d | %.4f (%.4f .. %.4f) | %d | %.0f | %.1f %% | %.3f (%.3f .. %.3f)%s | %d x %d | %.1f |"
                             % (J, M, K, fu[0], fu[1], fu[2], nb, rate / 1e9, 100 * rate / PEAK, ba[0] * scale, ba[1] * scale,
                                ba[2] * scale, "" if Bb == B else " scaled from %d series" % Bb, Bb, K, ba[0] * scale / fu[0]))
                print(lines[-1], flush=True)
                if fu[0] > ba[0] * scale:
                    slower.append("FINDING: at J = %d, M = %d, K = %d the fused call (%.4f ms) is SLOWER than the baseline (%.4f ms)."
                                  % (J, M, K, fu[0], ba[0] * scale))
                del eps, paths, dm, srep, crep, rows, work, mu, var, yk, e1, dk, zk, Wk, ref
                torch.cuda.empty_cache()
            del state, tm, am, Um, Vm, c
            torch.cuda.empty_cache()
    lines += [""] + (slower or ["The condition set in advance holds: the fused call is not slower than the baseline at any measured shape."])
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
