# -*- coding: utf-8 -*-
"""What the Keplerian search under correlated noise costs (csrc/c2_kepler.hip) beside the only route there was before it, on
one device, in ONE fresh process:

    python tools/bench_kepler.py [--steps 10] [--out profiles/keplerian_search.md] [--quick]
    python tools/bench_kepler.py --static-only --out profiles/keplerian_search.md   # no GPU: registers and instruction mix

  fused     ops.solve_lower ([1 | y]) + ops.whitened_keplerians + kepler.finish (torch): gp.keplerian_search's route
  kernel    ops.whitened_keplerians alone (the figure the share of the fp64 peak is taken from)
  composed  ops.whitened_gram on [1 | cos nu | sin nu ... | y] in chunks of at most 15 trials (Q <= 32), Kepler's equation
            solved and the design matrices built with torch inside the timed region, then the same finish on the blocks of S

alternating step by step at B x N x J x K = 64 x 4096 x 8 x 4096, 1 x 4096 x 8 x 4096, 1024 x 1024 x 4 x 1024 and
64 x 4096 x 32 x 512 (the shapes of profiles/periodogram.md with K trials for F frequencies), every step timed by its own
pair of HIP events after a warm-up.  The composed route takes thousands of launches a step and is given fewer steps
(--composed-steps).  The two routes' powers are compared before timing.

The kernel has no memory floor to quote (O(N K J) arithmetic on O(N J) bytes); its yardstick is the vector fp64 rate, as
in tools/bench_periodogram.py: the static part counts the fp64 VALU instructions of one row of one lane from the compiler's
own assembly, and the timed part turns lane-rows per second into a share of 39.3e12 fp64 instructions per lane and second.
The solver's share of a row is what is left of those instructions beside the recurrence's own (3 JR + 6 + QR a column, one
more for <z_c, z_s>)."""
import argparse
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trial_static import MIX_HEAD, alternate, fp64_valu, kept_block, mix_cells, row_loop_mix, sweep_asm, sweep_label, sweep_registers, sweep_symbol, with_block  # noqa: E402

FP64_PEAK = 78.6e12 / 2.0   # fp64 VALU instructions per lane and second
SHAPES = [(64, 4096, 8, 4096), (1, 4096, 8, 4096), (1024, 1024, 4, 1024), (64, 4096, 32, 512)]
TOOL = "tools/bench_kepler.py --static-only"
INSTANCES = ((4, 2), (8, 2), (16, 2), (32, 2), (8, 1), (8, 8), (16, 8))


def recurrence_fp64(jr, qr):
    """The fp64 VALU instructions of a lane-row that are not the solver's: per column fma, mul, fma a state element, three
    adds, the subtraction, z / d and <z, z>, one fma a Z0 column; one fma for <z_c, z_s>."""
    nc = 1 if jr == 32 else 2
    return nc * (3 * jr + 6 + qr) + 1


def instruction_table():
    asm = sweep_asm("keplerian")
    if asm is None:
        return None
    mix = lambda jr, qr: row_loop_mix(asm, sweep_symbol("keplerian", jr, qr))[0]
    lines = [MIX_HEAD + " solver's share of the fp64 VALU |", "|---|---|---|---|---|---|---|---|"]
    for jr, qr in INSTANCES:
        c = mix(jr, qr)
        lines.append("| `%s` | %s %.0f %% |" % (sweep_label("keplerian", jr, qr), mix_cells(c), 100.0 * (1.0 - recurrence_fp64(jr, qr) / fp64_valu(c))))
    lines += ["", "One row of one lane (one trial; at JR = 32 one of a trial's two columns): the solve has no branch, so this is the "
              "only path.  The solver's share: the row's fp64 VALU instructions less the recurrence's own (3 JR + 6 + QR a column, "
              "one for <z_c, z_s>).  fp64 VALU per lane-row, machine-readable: "
              + " ".join("JR%d=%d" % (jr, fp64_valu(mix(jr, 2))) for jr in (4, 8, 16, 32))]
    return "\n".join(lines)


def torch_columns(t, trials):
    """(cos nu, sin nu), each (B, N, K), in plain torch: the composed route's way to the two columns (torch.remainder, the
    same starter, four Danby steps with a fresh sine and cosine each)."""
    import torch

    w, e, tp = trials[:, None, :, 0], trials[:, None, :, 1], trials[:, None, :, 2]
    r = torch.remainder(w * (t[:, :, None] - tp) + math.pi, 2.0 * math.pi) - math.pi
    a = r.abs()
    sa = torch.sin(a)
    E = torch.minimum(a + e, a + e * sa / (1.0 - torch.sin(a + e) + sa))
    for _ in range(4):
        s, c = torch.sin(E), torch.cos(E)
        f, f1, f2, f3 = E - e * s - a, 1.0 - e * c, e * s, e * c
        d1 = -f / f1
        d2 = -f / (f1 + 0.5 * d1 * f2)
        E = E - f / (f1 + 0.5 * d2 * f2 + d2 * d2 * f3 / 6.0)
    s, c = torch.sin(E), torch.cos(E)
    g = 1.0 / (1.0 - e * c)
    return (c - e) * g, torch.copysign(torch.ones_like(r), r) * (torch.sqrt(1.0 - e * e) * s * g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--composed-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--static-only", action="store_true")
    a = ap.parse_args()
    old = open(a.out).read() if a.out and os.path.exists(a.out) else ""
    if a.static_only:
        text = with_block(old, "registers", sweep_registers("keplerian"), TOOL)
        text = with_block(text, "instructions", instruction_table(), TOOL)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import kepler as kp, ops, periodogram as pg, synth

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")
    per_row = dict((int(k), int(v)) for k, v in re.findall(r"JR(\d+)=(\d+)", kept_block(old, "instructions", TOOL) or ""))

    lines = ["# gp.keplerian_search's route beside ops.whitened_gram in chunks of 15 trials", "",
             "One process, steps alternating between the routes, %d timed steps each (composed: %d) after %d warm-up steps "
             "(composed: 1); ms: median (min .. max).  The routes' \"standard\" powers are compared before timing (neither is a "
             "reference: the worst distance in units of the standing criterion is listed under the table).  Share of the fp64 "
             "peak: lane-rows a second (B N K, twice that at J = 32, where a trial takes two lanes) times the fp64 VALU "
             "instructions of a lane-row (the table below) over 39.3e12." % (a.steps, a.composed_steps, a.warmup), "",
             "| B x N x J x K | route | ms | lane-rows / s | share of the vector fp64 peak | fused / composed |", "|---|---|---|---|---|---|"]
    agree = []
    for B, N, J, K in (SHAPES if not a.quick else [(8, 256, 8, 100), (4, 128, 32, 40)]):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, flag = ops.factor(t, c, av, U, V)
        span = (t[:, -1] - t[:, 0])[:, None]
        gen = torch.Generator(device="cpu").manual_seed(K)
        w = 2.0 * torch.pi / span * torch.linspace(1.0, N / 4.0, K, dtype=torch.float64, device=dev)[None, :]
        e = (0.9 * torch.rand((1, K), dtype=torch.float64, generator=gen)).to(dev).expand(B, K)
        tp = t[:, :1] + torch.rand((1, K), dtype=torch.float64, generator=gen).to(dev) * (2.0 * torch.pi / w)
        trials = torch.stack([w, e, tp], dim=-1).contiguous()
        Y0 = torch.stack([torch.ones_like(y), y], dim=-1).contiguous()
        Z0, T = torch.empty_like(Y0), torch.empty((B, K, 7), dtype=torch.float64, device=dev)
        ok = flag == 0
        chunks = [(lo, min(lo + 15, K)) for lo in range(0, K, 15)]
        T2 = torch.empty_like(T)
        A = torch.empty((B, N, 31), dtype=torch.float64, device=dev)
        S = torch.empty((B, 32, 32), dtype=torch.float64, device=dev)
        res = {}

        def fused():
            ops.solve_lower(t, c, U, W, Y0, Z=Z0)
            ops.whitened_keplerians(t, c, U, W, d, Z0, trials, out=T)
            res["fused"] = kp.finish(pg.null_products(Z0, d), T, N, ok=ok, trials=trials).power

        def kernel():
            ops.whitened_keplerians(t, c, U, W, d, Z0, trials, out=T)

        def composed():
            S0 = None
            for lo, hi in chunks:
                n = hi - lo
                Ac, Sc = (A, S) if n == 15 else (torch.empty((B, N, 1 + 2 * n), dtype=torch.float64, device=dev),
                                                 torch.empty((B, 2 + 2 * n, 2 + 2 * n), dtype=torch.float64, device=dev))
                Ac[..., 0] = 1.0
                Ac[..., 1:1 + n], Ac[..., 1 + n:] = torch_columns(t, trials[:, lo:hi])
                ops.whitened_gram(t, c, U, W, d, Ac, y, S=Sc)
                k, q = torch.arange(1, 1 + n, device=dev), 1 + 2 * n
                T2[:, lo:hi, 0], T2[:, lo:hi, 1], T2[:, lo:hi, 2] = Sc[:, k, k], Sc[:, k, k + n], Sc[:, k + n, k + n]
                T2[:, lo:hi, 3], T2[:, lo:hi, 4] = Sc[:, k, 0], Sc[:, k, q]
                T2[:, lo:hi, 5], T2[:, lo:hi, 6] = Sc[:, k + n, 0], Sc[:, k + n, q]
                S0 = Sc[:, [0, q]][:, :, [0, q]]
            res["composed"] = kp.finish(S0, T2, N, ok=ok, trials=trials).power

        fused()
        composed()
        torch.cuda.synchronize()
        p1, p2 = res["fused"], res["composed"]
        fin = torch.isfinite(p2).all(dim=1) & ok
        tol = 1e-10 * p2.abs() + 1e-12 * p2.abs().amax(dim=1, keepdim=True)
        worst = float(((p1 - p2).abs() / tol)[fin].max())
        assert bool(torch.equal(torch.isnan(p1), torch.isnan(p2))) and worst < 1e4, "the two routes disagree: %g" % worst
        agree.append("%d x %d x %d x %d: %.3g (%d series not factored)" % (B, N, J, K, worst, int((~ok).sum())))
        out = alternate({"fused": (fused, None), "kernel": (kernel, None), "composed": (composed, a.composed_steps)}, a.steps, a.warmup)
        jr = 4 if J <= 4 else 8 if J <= 8 else 16 if J <= 16 else 32
        lane_rows = B * N * K * (2 if jr == 32 else 1)
        for op, st in out.items():
            rate = lane_rows / (st[0] * 1e-3)
            share = "%.1f %%" % (100.0 * rate * per_row[jr] / FP64_PEAK) if op == "kernel" and jr in per_row else ""
            lines.append("| %d x %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %s | %s | %s |"
                         % (B, N, J, K, op, st[0], st[1], st[2], "%.3g" % rate if op == "kernel" else "", share,
                            "%.4f" % (out["fused"][0] / out["composed"][0]) if op == "fused" else ""))
            print(lines[-1], flush=True)
        del t, c, av, U, V, y, d, W, trials, Y0, Z0, T, T2, A, S
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
