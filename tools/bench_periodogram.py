# -*- coding: utf-8 -*-
"""What the periodogram under correlated noise costs (csrc/c2_periodogram.hip) beside the only route there was before it, on
one device, in ONE fresh process:

    python tools/bench_periodogram.py [--steps 10] [--out profiles/periodogram.md] [--quick]
    python tools/bench_periodogram.py --static-only --out profiles/periodogram.md   # no GPU: registers and instruction mix

  fused     ops.solve_lower ([1 | y]) + ops.whitened_sinusoids + periodogram.finish (torch)
  kernel    ops.whitened_sinusoids alone (the figure the share of the fp64 peak is taken from)
  composed  ops.whitened_gram on [1 | cos | sin ... | y] in chunks of at most 15 frequencies (Q <= 32), the design matrices
            built with torch inside the timed region, then the same finish on the blocks of S

alternating step by step at B x N x J x F = 64 x 4096 x 8 x 4096, 1 x 4096 x 8 x 4096, 1024 x 1024 x 4 x 1024 and
64 x 4096 x 32 x 512, every step timed by its own pair of HIP events after a warm-up.  The composed route takes hundreds of
launches a step and is given fewer steps (--composed-steps).  The two routes' powers are compared before timing.

The kernel has no memory floor to quote (O(N F J) arithmetic on O(N J) bytes); its yardstick is the vector fp64 rate.  The
static part counts the fp64 VALU instructions of one row of one lane from the compiler's own assembly (the blocks of the
device library's large-argument sine and cosine, which a wavefront skips when no lane needs them, left out), and the
timed part turns lane-rows per second into a share of 39.3e12 fp64 instructions per lane and second -- the public
78.6 TFLOP/s vector fp64 figure of the part counted as fused multiply-adds, half the 157.3 TFLOP/s fp32 vector peak."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trial_static import MIX_HEAD, alternate, fp64_valu, kept_block, mix_cells, row_loop_mix, sweep_asm, sweep_label, sweep_registers, sweep_symbol, with_block  # noqa: E402

FP64_PEAK = 78.6e12 / 2.0   # fp64 VALU instructions per lane and second
SHAPES = [(64, 4096, 8, 4096), (1, 4096, 8, 4096), (1024, 1024, 4, 1024), (64, 4096, 32, 512)]
TOOL = "tools/bench_periodogram.py --static-only"
REGISTER_NOTE = ("  About 80 of each instance's registers hold the double-precision constants of the sine "
                 "and cosine, which the compiler keeps in vector registers across the row loop.")


def instruction_table():
    """The row loop's instruction mix per width, without the forward-skipped regions that hold the device library's
    large-argument reduction (v_trig_preop_f64)."""
    asm = sweep_asm("periodogram")
    if asm is None:
        return None
    mix = lambda jr, qr: row_loop_mix(asm, sweep_symbol("periodogram", jr, qr), "v_trig_preop_f64")[0]
    lines = [MIX_HEAD, "|---|---|---|---|---|---|---|"]
    for jr, qr in ((4, 2), (8, 2), (16, 2), (32, 2), (8, 1), (8, 8)):
        lines.append("| `%s` | %s" % (sweep_label("periodogram", jr, qr), mix_cells(mix(jr, qr))))
    lines += ["", "One row of one lane (one frequency; at JR = 32 one of a frequency's two columns), the path a wavefront takes when "
              "every phase is below kSincosFastMax.  fp64 VALU per lane-row, machine-readable: "
              + " ".join("JR%d=%d" % (jr, fp64_valu(mix(jr, 2))) for jr in (4, 8, 16, 32))]
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
        text = with_block(old, "registers", sweep_registers("periodogram", REGISTER_NOTE), TOOL)
        text = with_block(text, "instructions", instruction_table(), TOOL)
        if a.out:
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import ops, periodogram as pg, synth

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")
    per_row = dict((int(k), int(v)) for k, v in re.findall(r"JR(\d+)=(\d+)", kept_block(old, "instructions", TOOL) or ""))

    lines = ["# gp.periodogram's route beside ops.whitened_gram in chunks of 15 frequencies", "",
             "One process, steps alternating between the routes, %d timed steps each (composed: %d) after %d warm-up steps "
             "(composed: 1); ms: median (min .. max).  The routes' \"standard\" powers are compared before timing (neither is a reference: the "
             "worst distance in units of the standing criterion is listed under the table).  Share of the fp64 peak: lane-rows a second (B N F, twice that at J = 32, where a "
             "frequency takes two lanes) times the fp64 VALU instructions of a lane-row (the table below) over 39.3e12."
             % (a.steps, a.composed_steps, a.warmup), "",
             "| B x N x J x F | route | ms | lane-rows / s | share of the vector fp64 peak | fused / composed |", "|---|---|---|---|---|---|"]
    agree = []
    for B, N, J, F in (SHAPES if not a.quick else [(8, 256, 8, 100), (4, 128, 32, 40)]):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, flag = ops.factor(t, c, av, U, V)
        span = (t[:, -1] - t[:, 0])[:, None]
        freq = (2.0 * torch.pi / span * torch.linspace(1.0, N / 4.0, F, dtype=torch.float64, device=dev)[None, :]).contiguous()
        Y0 = torch.stack([torch.ones_like(y), y], dim=-1).contiguous()
        Z0, T = torch.empty_like(Y0), torch.empty((B, F, 7), dtype=torch.float64, device=dev)
        ok = flag == 0
        chunks = [(lo, min(lo + 15, F)) for lo in range(0, F, 15)]
        T2 = torch.empty_like(T)
        A = torch.empty((B, N, 31), dtype=torch.float64, device=dev)
        A[..., 0] = 1.0
        S = torch.empty((B, 32, 32), dtype=torch.float64, device=dev)
        res = {}

        def fused():
            ops.solve_lower(t, c, U, W, Y0, Z=Z0)
            ops.whitened_sinusoids(t, c, U, W, d, Z0, freq, out=T)
            res["fused"] = pg.finish(pg.null_products(Z0, d), T, N, ok=ok).power

        def kernel():
            ops.whitened_sinusoids(t, c, U, W, d, Z0, freq, out=T)

        def composed():
            S0 = None
            for lo, hi in chunks:
                n = hi - lo
                x = freq[:, None, lo:hi] * t[:, :, None]
                Ac, Sc = (A, S) if n == 15 else (torch.empty((B, N, 1 + 2 * n), dtype=torch.float64, device=dev),
                                                 torch.empty((B, 2 + 2 * n, 2 + 2 * n), dtype=torch.float64, device=dev))
                Ac[..., 0] = 1.0
                torch.cos(x, out=Ac[..., 1:1 + n])
                torch.sin(x, out=Ac[..., 1 + n:])
                ops.whitened_gram(t, c, U, W, d, Ac, y, S=Sc)
                k, q = torch.arange(1, 1 + n, device=dev), 1 + 2 * n
                T2[:, lo:hi, 0], T2[:, lo:hi, 1], T2[:, lo:hi, 2] = Sc[:, k, k], Sc[:, k, k + n], Sc[:, k + n, k + n]
                T2[:, lo:hi, 3], T2[:, lo:hi, 4] = Sc[:, k, 0], Sc[:, k, q]
                T2[:, lo:hi, 5], T2[:, lo:hi, 6] = Sc[:, k + n, 0], Sc[:, k + n, q]
                S0 = Sc[:, [0, q]][:, :, [0, q]]
            res["composed"] = pg.finish(S0, T2, N, ok=ok).power

        fused()
        composed()
        torch.cuda.synchronize()
        p1, p2 = res["fused"], res["composed"]
        fin = torch.isfinite(p2).all(dim=1) & ok
        tol = 1e-10 * p2.abs() + 1e-12 * p2.abs().amax(dim=1, keepdim=True)
        worst = float(((p1 - p2).abs() / tol)[fin].max())
        assert bool(torch.equal(torch.isnan(p1), torch.isnan(p2))) and worst < 1e4, "the two routes disagree: %g" % worst
        agree.append("%d x %d x %d x %d: %.3g (%d series not factored)" % (B, N, J, F, worst, int((~ok).sum())))
        out = alternate({"fused": (fused, None), "kernel": (kernel, None), "composed": (composed, a.composed_steps)}, a.steps, a.warmup)
        jr = 4 if J <= 4 else 8 if J <= 8 else 16 if J <= 16 else 32
        lane_rows = B * N * F * (2 if jr == 32 else 1)
        for op, st in out.items():
            rate = lane_rows / (st[0] * 1e-3)
            share = "%.1f %%" % (100.0 * rate * per_row[jr] / FP64_PEAK) if op == "kernel" and jr in per_row else ""
            lines.append("| %d x %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %s | %s | %s |"
                         % (B, N, J, F, op, st[0], st[1], st[2], "%.3g" % rate if op == "kernel" else "", share,
                            "%.4f" % (out["fused"][0] / out["composed"][0]) if op == "fused" else ""))
            print(lines[-1], flush=True)
        del t, c, av, U, V, y, d, W, freq, Y0, Z0, T, T2, A, S
        torch.cuda.empty_cache()
    lines += ["", "Worst |fused - composed| power in units of the standing criterion: " + "; ".join(agree) + "."]
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
