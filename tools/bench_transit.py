# -*- coding: utf-8 -*-
"""What the transit search under correlated noise costs (csrc/c2_transit.hip) beside the only route there was before it, on
one device, in ONE fresh process:

    python tools/bench_transit.py [--steps 10] [--out profiles/transit_search.md] [--quick]
    python tools/bench_transit.py --static-only --out profiles/transit_search.md   # no GPU: registers and instruction mix

  fused     ops.solve_lower ([1 | y]) + ops.whitened_transits + transit.finish (torch)
  kernel    ops.whitened_transits alone (the figure the share of the fp64 rate is taken from)
  composed  ops.whitened_gram on [1 | b_k ... | y] in chunks of at most 30 trials (Q <= 32), the templates built with torch
            inside the timed region, then the same finish on the blocks of S

alternating step by step at B x N x J x K = 64 x 4096 x 8 x 4096, 1 x 4096 x 8 x 4096, 1024 x 1024 x 4 x 1024 and
64 x 4096 x 32 x 512 on folded box trials, every step timed by its own pair of HIP events after a warm-up, plus one run of
single events sorted by epoch at the first shape (fused and kernel only).  The composed route takes hundreds of launches a
step and is given fewer steps (--composed-steps).  The two routes' delta_chi2 are compared before timing.

The kernel has no memory floor to quote (O(N K J) arithmetic on O(N J) bytes); its yardstick is the vector fp64 rate, as for
the periodogram: the static part counts the fp64 VALU instructions of one row of one lane from the compiler's
own assembly (the ramp's division, which a wavefront skips when no lane is on an ingress or egress, left out), and the timed
part turns lane-rows per second into a share of 39.3e12 fp64 instructions per lane and second -- the public 78.6 TFLOP/s
vector fp64 figure of the part counted as fused multiply-adds."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trial_static import MIX_HEAD, alternate, fp64_valu, kept_block, mix_cells, row_loop_mix, sweep_asm, sweep_label, sweep_registers, sweep_symbol, with_block  # noqa: E402

FP64_PEAK = 78.6e12 / 2.0   # fp64 VALU instructions per lane and second
SHAPES = [(64, 4096, 8, 4096), (1, 4096, 8, 4096), (1024, 1024, 4, 1024), (64, 4096, 32, 512)]
CHUNK = 30
TOOL = "tools/bench_transit.py --static-only"


def instruction_table():
    """The row loop's instruction mix per width; the forward-skipped region that holds the ramp's division (v_div_fmas_f64)
    is counted apart."""
    asm = sweep_asm("transit")
    if asm is None:
        return None
    lines = [MIX_HEAD + " the ramp's block (fp64 VALU / all) |", "|---|---|---|---|---|---|---|---|"]
    per_row = {}
    for jr, qr in ((4, 2), (8, 2), (16, 2), (32, 2), (8, 1), (8, 8)):
        c, ramp = row_loop_mix(asm, sweep_symbol("transit", jr, qr), "v_div_fmas_f64")
        if qr == 2:
            per_row[jr] = fp64_valu(c)
        lines.append("| `%s` | %s %d / %d |" % (sweep_label("transit", jr, qr), mix_cells(c), fp64_valu(ramp), sum(ramp.values())))
    lines += ["", "One row of one lane (one trial), the path a wavefront takes when no lane is on an ingress or egress (box trials "
              "always); the last column is the block with the ramp's division, entered by a wavefront with at least one such lane.  "
              "fp64 VALU per lane-row, machine-readable: " + " ".join("JR%d=%d" % kv for kv in sorted(per_row.items()))]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--composed-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--static-only", action="store_true")
    a = ap.parse_args()
    old = open(a.out).read() if a.out and os.path.exists(a.out) else ""
    if a.static_only:
        text = with_block(old, "registers", sweep_registers("transit"), TOOL)
        text = with_block(text, "instructions", instruction_table(), TOOL)
        if a.out:
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import ops, periodogram as pg, synth, transit as tr

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")
    per_row = dict((int(k), int(v)) for k, v in re.findall(r"JR(\d+)=(\d+)", kept_block(old, "instructions", TOOL) or ""))

    lines = ["# gp.transit_search's route beside ops.whitened_gram in chunks of %d trials" % CHUNK, "",
             "One process, steps alternating between the routes, %d timed steps each (composed: %d) after %d warm-up steps "
             "(composed: 1); ms: median (min .. max).  Trials: folded boxes (periods from a fiftieth to a third of the baseline, "
             "durations 2 %% of the period, epochs uniform over the baseline), shared by the batch; \"single\": single events of "
             "1 %% of the baseline sorted by epoch over the baseline (no composed route timed).  The routes' delta_chi2 are compared before "
             "timing (neither is a reference: the worst distance in units of the standing criterion is listed under the table).  "
             "Share of the fp64 rate: lane-rows a second (B N K) times the fp64 VALU instructions of a lane-row (the table below) "
             "over 39.3e12." % (a.steps, a.composed_steps, a.warmup), "",
             "| B x N x J x K | trials | route | ms | lane-rows / s | share of the vector fp64 rate | fused / composed |", "|---|---|---|---|---|---|---|"]
    agree = []
    shapes = [s + ("folded",) for s in (SHAPES if not a.quick else [(8, 256, 8, 100), (4, 128, 32, 40)])]
    shapes.insert(1, shapes[0][:4] + ("single",))
    for B, N, J, K, kind in shapes:
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, flag = ops.factor(t, c, av, U, V)
        t_lo, span = float(t.min()), float(t.max() - t.min())
        gen = torch.Generator(device="cpu").manual_seed(1)
        if kind == "folded":
            P = span / torch.linspace(3.0, 50.0, K, dtype=torch.float64)
            trials = torch.stack([P, t_lo + span * torch.rand(K, dtype=torch.float64, generator=gen), 0.02 * P, torch.zeros_like(P)], dim=1)
        else:
            one = torch.ones(K, dtype=torch.float64)
            trials = torch.stack([0.0 * one, t_lo + span * torch.linspace(0.0, 1.0, K, dtype=torch.float64), 0.01 * span * one, 0.0 * one], dim=1)
        trials = trials.to(dev).contiguous()
        Y0 = torch.stack([torch.ones_like(y), y], dim=-1).contiguous()
        Z0, T = torch.empty_like(Y0), torch.empty((B, K, 3), dtype=torch.float64, device=dev)
        ok = flag == 0
        chunks = [(lo, min(lo + CHUNK, K)) for lo in range(0, K, CHUNK)]
        T2 = torch.empty_like(T)
        A = torch.empty((B, N, 1 + CHUNK), dtype=torch.float64, device=dev)
        S = torch.empty((B, 2 + CHUNK, 2 + CHUNK), dtype=torch.float64, device=dev)
        zero, one_ = torch.zeros((), dtype=torch.float64, device=dev), torch.ones((), dtype=torch.float64, device=dev)
        res = {}

        def fused():
            ops.solve_lower(t, c, U, W, Y0, Z=Z0)
            ops.whitened_transits(t, c, U, W, d, Z0, trials, out=T)
            res["fused"] = tr.finish(pg.null_products(Z0, d), T, N, ok=ok, trials=trials).delta_chi2

        def kernel():
            ops.whitened_transits(t, c, U, W, d, Z0, trials, out=T)

        def composed():
            S0 = None
            for lo, hi in chunks:
                n = hi - lo
                P, t0, w, tau = [trials[lo:hi, i] for i in range(4)]
                x = t[:, :, None] - t0
                phi = x - torch.round(x * torch.where(P != 0, 1.0 / P, zero)) * P
                u = 0.5 * w - phi.abs()
                Ac, Sc = (A, S) if n == CHUNK else (torch.empty((B, N, 1 + n), dtype=torch.float64, device=dev),
                                                    torch.empty((B, 2 + n, 2 + n), dtype=torch.float64, device=dev))
                Ac[..., 0] = 1.0
                Ac[..., 1:] = torch.where(u >= tau, one_, torch.where(u >= 0, u / tau, zero))
                ops.whitened_gram(t, c, U, W, d, Ac, y, S=Sc)
                k, q = torch.arange(1, 1 + n, device=dev), 1 + n
                T2[:, lo:hi, 0], T2[:, lo:hi, 1], T2[:, lo:hi, 2] = Sc[:, k, k], Sc[:, k, 0], Sc[:, k, q]
                S0 = Sc[:, [0, q]][:, :, [0, q]]
            res["composed"] = tr.finish(S0, T2, N, ok=ok, trials=trials).delta_chi2

        fused()
        runs = {"fused": (fused, None), "kernel": (kernel, None)}
        if kind == "folded":
            composed()
            torch.cuda.synchronize()
            p1, p2 = res["fused"], res["composed"]
            fin = torch.isfinite(p2) & ok[:, None]
            tol = 1e-10 * p2.abs() + 1e-12 * torch.nan_to_num(p2).abs().amax(dim=1, keepdim=True)
            worst = float(((p1 - p2).abs() / tol)[fin].max())
            assert bool(torch.equal(torch.isnan(p1), torch.isnan(p2))) and worst < 1e4, "the two routes disagree: %g" % worst
            agree.append("%d x %d x %d x %d: %.3g (%d series not factored, %d trials NaN in each)"
                         % (B, N, J, K, worst, int((~ok).sum()), int(torch.isnan(p1[ok]).sum())))
            runs["composed"] = (composed, a.composed_steps)
        out = alternate(runs, a.steps, a.warmup)
        jr = 4 if J <= 4 else 8 if J <= 8 else 16 if J <= 16 else 32
        lane_rows = B * N * K
        for op, st in out.items():
            rate = lane_rows / (st[0] * 1e-3)
            share = "%.1f %%" % (100.0 * rate * per_row[jr] / FP64_PEAK) if op == "kernel" and jr in per_row else ""
            lines.append("| %d x %d x %d x %d | %s | %s | %.3f (%.3f .. %.3f) | %s | %s | %s |"
                         % (B, N, J, K, kind, op, st[0], st[1], st[2], "%.3g" % rate if op == "kernel" else "", share,
                            "%.4f" % (out["fused"][0] / out["composed"][0]) if op == "fused" and "composed" in out else ""))
            print(lines[-1], flush=True)
        del t, c, av, U, V, y, d, W, trials, Y0, Z0, T, T2, A, S
        torch.cuda.empty_cache()
    lines += ["", "Worst |fused - composed| delta_chi2 in units of the standing criterion: " + "; ".join(agree) + "."]
    text = "\n".join(lines) + "\n"
    for key in ("registers", "instructions"):
        text = with_block(text, key, kept_block(old, key, TOOL), TOOL)
    # whatever follows the generated part of an earlier file (hand-written notes) is kept
    if "<!-- notes -->" in old:
        text += "\n<!-- notes -->" + old.split("<!-- notes -->", 1)[1]
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
