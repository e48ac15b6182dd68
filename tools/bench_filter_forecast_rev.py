# -*- coding: utf-8 -*-
"""What the gradient of a streaming forecast and of a streaming absorb costs (csrc/c2_filter_stream_rev.hip), on one device, in
ONE fresh process:

    python tools/bench_filter_forecast_rev.py [--steps 10] [--out profiles/filter_forecast_rev.md] [--quick]
    python tools/bench_filter_forecast_rev.py --regs-only --out profiles/filter_forecast_rev.md   # no GPU: the register table

FORECAST PLUS REVERSE: ops.filter_forecast, the cotangents of sum log N(y | mu, var) in torch, ops.filter_forecast_rev, of M in
{1, 4, 16} query rows at width J in {2, 8} from a state that holds N = 4096 rows -- at B = 65536 series, and at the largest
batch (a power of two, at most 65536) at which the only route there was before fits its 16 N J^2 bytes per series of workspace
into --old-budget-gib: autograd.predictive_log_density, two sweeps and their reverses over all N + M rows.  The condition set
in advance: forecast plus reverse must not take longer than that old route at the same batch.

ABSORB REVERSE: ops.filter_absorb_rev of N = 4096 rows at B = 64 and 8192 series beside ops.filter_append +
ops.filter_append_rev over the same rows -- a report with no threshold.  Its ws costs 8 N (J + J^2) bytes per series.

The routes alternate step by step in the same process; every step is timed by its own pair of HIP events after a warm-up; the
table gives the median (min .. max) of --steps steps and the bytes a call moves per series as a fraction of the 8 TB/s
roofline.  The register table comes from tools/kernel_regs.py (the built object, celerite2_amd/build)."""
import argparse
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_filter_forecast_rev.py --regs-only) -->", "<!-- registers:end -->"
TITLE = "# ops.filter_forecast_rev and ops.filter_absorb_rev beside the whole-series routes"
NOT_MEASURED = (TITLE + "\n\nNot measured yet: run `python tools/bench_filter_forecast_rev.py --out profiles/filter_forecast_rev.md` "
                "on an MI355X.\n")


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_filter_stream_rev.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::filter_stream_rev::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`<lanes per series>`)."
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or ("(the built objects are not on this machine: run `python tools/bench_filter_forecast_rev.py --regs-only "
                                 "--out <this file>` where the library was built)")
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def forecast_bytes(J, M):
    """forecast (state, per row t, a, U in, mu, var out) + reverse (state in, bstate and bc out, per row t, U, bmu, bvar in and
    bt, ba, bU out), per series."""
    SW = 4 + J + J * J
    return 8 * SW + M * 8 * (4 + J) + 16 * SW + 8 * J + M * 8 * (5 + 2 * J)


def absorb_rev_bytes(J, M):
    """state_in and bstate_out in, bstate_in and bc out, per row t, d, z, W in, bt, bd, bz, bW out, ws written and read back."""
    return 24 * (4 + J + J * J) + 8 * J + M * (8 * (3 + J) + 8 * (3 + J) + 16 * (J + J * J))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--old-budget-gib", type=float, default=64.0, help="what the old route's 16 N J^2 B bytes of workspace may take")
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

    def worst(x, xo):   # the standing criterion, as tests/inverse_diag_ref.py::err
        return float(((x - xo).abs() / (1e-10 * xo.abs() + 1e-12 * xo.abs().max())).max())

    def ms(r):
        return "%.4f (%.4f .. %.4f)" % r

    Bbig, N = (65536, 4096) if not a.quick else (512, 256)
    lines = [TITLE, "",
             "## Forecast plus reverse", "",
             "N = %d rows in the state, M query rows, the objective sum log N(y | mu, var) of the rows behind the state.  `new`: "
             "ops.filter_forecast, the objective's cotangents in torch, ops.filter_forecast_rev.  `old`: "
             "autograd.predictive_log_density forward and backward over all N + M rows (its workspace: 16 N J^2 bytes per series; "
             "timed where that fits %.0f GiB).  One process, steps alternating between the routes, %d timed steps each after %d "
             "warm-up steps; ms: median (min .. max).  `worst`: the new route's value against the old one's in units of the "
             "standing criterion (reported, not asserted: the two condition differently over N rows)."
             % (N, a.old_budget_gib, a.steps, a.warmup), "",
             "| J | M | B | new, ms | bytes per series | GB/s | of the 8 TB/s roofline | old, ms | old / new | worst |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    findings = []
    for J in (2, 8):
        fits = Bbig
        while fits > 1 and 16.0 * N * J * J * fits > a.old_budget_gib * 2**30:
            fits //= 2
        for Bx in sorted({Bbig, fits}, reverse=True):
            for M in (1, 4, 16):
                t, c, av, U, V, y = synth.device_batch_fast(0, Bx, N + M, J, dev)
                d, W, flag = ops.factor(t, c, av, U, V)
                assert int(flag.abs().sum()) == 0
                z = ops.solve_lower(t, c, U, W, y[..., None].contiguous())[..., 0]
                head = lambda x: x[:, :N].contiguous()
                tail = lambda x: x[:, N:].contiguous()
                state = ops.filter_absorb(ops.filter_init(Bx, J, dev), head(t), c, head(W), head(d), head(z))
                del d, W, z
                tm, am, Um, ym = (tail(x) for x in (t, av, U, y))
                mu, var = torch.empty_like(am), torch.empty_like(am)
                grads = ops.filter_forecast_rev(state, tm, c, Um, torch.zeros_like(am), torch.zeros_like(am))
                val = [None]

                def new():
                    ops.filter_forecast(state, tm, c, am, Um, mu=mu, var=var)
                    r = ym - mu
                    val[0] = (-0.5 * (r * r / var + torch.log(var) + math.log(2 * math.pi))).sum(dim=1)
                    ops.filter_forecast_rev(state, tm, c, Um, r / var, 0.5 * (r * r / (var * var) - 1.0 / var), out=grads)

                runs = {"new": new}
                old_ok = Bx <= fits
                if old_ok:
                    th, ah, Uh, Vh, yh = (head(x) for x in (t, av, U, V, y))
                    Vm = tail(V)
                    del t, av, U, V, y
                    torch.cuda.empty_cache()
                    k0 = (Um * Vm).sum(dim=-1)[:, 0].contiguous()   # k(0) = u . v of any row
                    noise = am - k0[:, None]
                    leaves = [x.requires_grad_() for x in (th, c.clone(), ah, Uh, Vh, yh, tm.clone(), Um.clone(), Vm)]
                    vo = [None]

                    def old():
                        for x in leaves:
                            x.grad = None
                        vo[0] = ag.predictive_log_density(*leaves[:6], *leaves[6:], k0, ym, noise)
                        vo[0].sum().backward()

                    runs["old"] = old
                else:
                    del t, av, U, V, y
                    torch.cuda.empty_cache()
                res = alternate(runs, a.steps)
                nb = forecast_bytes(J, M)
                rate = nb * Bx / (res["new"][0] * 1e-3)
                w = worst(val[0], vo[0].detach()) if old_ok else float("nan")
                lines.append("| %d | %d | %d | %s | %d | %.0f | %.2f %% | %s | %s | %s |"
                             % (J, M, Bx, ms(res["new"]), nb, rate / 1e9, 100 * rate / PEAK, ms(res["old"]) if old_ok else "does not fit",
                                "%.0f" % (res["old"][0] / res["new"][0]) if old_ok else "", "%.2g" % w if old_ok else ""))
                print(lines[-1], flush=True)
                if old_ok and res["new"][0] > res["old"][0]:   # the one condition; a finding to report, not to tune away
                    findings.append("FINDING: at J = %d, M = %d, B = %d forecast plus reverse (%.4f ms) takes longer than the old route "
                                    "(%.3f ms)." % (J, M, Bx, res["new"][0], res["old"][0]))
                if old_ok:
                    del leaves, th, ah, Uh, Vh, yh, Vm, vo, old
                del runs, new, state, tm, am, Um, ym, mu, var, grads, val
                torch.cuda.empty_cache()
    lines += [""] + (findings or ["Forecast plus reverse is faster than the old route at every shape at which the old route was timed."])

    lines += ["", "## Absorb reverse", "",
              "ops.filter_absorb_rev of N = %d rows from the empty state, the cotangent that of the log-likelihood of the state left, "
              "beside ops.filter_append + ops.filter_append_rev over the same rows (the only reverse over given rows there was).  A "
              "report with no threshold.  ws costs 8 N (J + J^2) bytes per series." % N, "",
              "| J | B | absorb_rev, ms | bytes per series (ws of them) | GB/s | of the 8 TB/s roofline | absorb, ms | append + append_rev, ms |",
              "|---|---|---|---|---|---|---|---|"]
    for J in (2, 8):
        for Bx in ((64, 8192) if not a.quick else (64,)):
            t, c, av, U, V, y = synth.device_batch_fast(0, Bx, N, J, dev)
            st0 = ops.filter_init(Bx, J, dev)
            out, d, W, z, fl = ops.filter_append(st0, t, c, av, U, V, y)
            assert int(fl.abs().sum()) == 0
            bstate = torch.zeros_like(st0)
            bstate[:, 1], bstate[:, 2], bstate[:, 3] = -0.5 * math.log(2 * math.pi), -0.5, -0.5
            ws = torch.empty((Bx, N, ops.filter_rev_workspace_words(J)), dtype=torch.float64, device=dev)
            g_ab = ops.filter_absorb_rev(st0, t, c, W, d, z, bstate, ws=ws)
            g_ap = ops.filter_append_rev(st0, t, c, U, W, d, z, fl, bstate, ws=ws)
            o2 = torch.empty_like(st0)

            def both():
                ops.filter_append(st0, t, c, av, U, V, y, out=out, d=d, W=W, z=z)
                ops.filter_append_rev(st0, t, c, U, W, d, z, fl, bstate, ws=ws, out=g_ap)

            res = alternate({"absorb_rev": lambda: ops.filter_absorb_rev(st0, t, c, W, d, z, bstate, ws=ws, out=g_ab),
                             "absorb": lambda: ops.filter_absorb(st0, t, c, W, d, z, out=o2), "both": both}, a.steps)
            nb = absorb_rev_bytes(J, N)
            rate = nb * Bx / (res["absorb_rev"][0] * 1e-3)
            lines.append("| %d | %d | %s | %d (%d) | %.0f | %.2f %% | %s | %s |"
                         % (J, Bx, ms(res["absorb_rev"]), nb, 8 * N * (J + J * J), rate / 1e9, 100 * rate / PEAK, ms(res["absorb"]),
                            ms(res["both"])))
            print(lines[-1], flush=True)
            del t, c, av, U, V, y, st0, out, d, W, z, fl, bstate, ws, g_ab, g_ap, o2, both
            torch.cuda.empty_cache()
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
