# -*- coding: utf-8 -*-
"""What the multi-harmonic periodogram under correlated noise costs (csrc/c2_harmonics.hip) beside the two routes there were
before it, on one device, in ONE fresh process:

    python tools/bench_harmonics.py [--steps 10] [--out profiles/harmonics.md] [--quick]
    python tools/bench_harmonics.py --static-only --out profiles/harmonics.md   # no GPU: registers and instruction mix

  whole       ops.solve_lower ([1 | y]) + ops.whitened_harmonics + harmonics.finish (torch): gp.periodogram(nterms=H)
  kernel      ops.whitened_harmonics alone
  sinusoids   (a) H calls of ops.whitened_sinusoids at h * freq: the same column work WITHOUT the products between
              harmonics -- the floor of the one-harmonic-per-lane form, not a route to the fit
  composed    (b) ops.whitened_gram on [1 | c_1 s_1 .. c_H s_H of n frequencies | y] in chunks of n = 30 // (2 H)
              frequencies (Q <= 32), the design matrices built with torch inside the timed region.  Timed on the first
              --composed-chunks chunks only and scaled to F (every chunk is the same work): at H = 4 the full grid of the
              first shape is 1366 launches a step.

for H = 2, 3, 4, alternating step by step at B x N x J x F = 64 x 4096 x 8 x 4096, 1 x 4096 x 8 x 4096, 1024 x 1024 x 4 x 1024
and 64 x 4096 x 32 x 512 (the shapes of profiles/periodogram.md), every step timed by its own pair of HIP events after a
warm-up.  The kernel's products are compared with the composed route's on the timed chunks before timing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trial_static import MIX_HEAD, alternate, kept_block, kernel_asm, mix_cells, register_table, row_loop_mix, with_block  # noqa: E402

SHAPES = [(64, 4096, 8, 4096), (1, 4096, 8, 4096), (1024, 1024, 4, 1024), (64, 4096, 32, 512)]
TOOL = "tools/bench_harmonics.py --static-only"
REGISTER_NOTE = (" (`k_harmonic_sweep<GH, JR, QR>`: GH the lanes a trial's harmonics are rounded to, 2 for H = 2 and 4 for H = 3, 4; J "
                 "rounded up to 4, 8, 16 or 32, Q0 to 1, 2, 4 or 8).  About 80 of each instance's registers hold the double-precision "
                 "constants of the sine and cosine, which the compiler keeps in vector registers across the row loop.")


def symbol(gh, jr, qr):
    return "_ZN2c29harmonics16k_harmonic_sweepILi%dELi%dELi%dEE" % (gh, jr, qr)


def instruction_table():
    """The row loop's instruction mix, without the forward-skipped regions that hold the device library's large-argument
    reduction (v_trig_preop_f64)."""
    asm = kernel_asm("c2_harmonics.hip")
    if asm is None:
        return None
    lines = [MIX_HEAD, "|---|---|---|---|---|---|---|"]
    for gh, jr, qr in ((2, 4, 2), (4, 4, 2), (2, 8, 2), (4, 8, 2), (2, 16, 2), (4, 16, 2), (2, 32, 2), (4, 32, 2)):
        mix = row_loop_mix(asm, symbol(gh, jr, qr), "v_trig_preop_f64")[0]
        dpp = sum(v for k, v in mix.items() if k.startswith("v_mov_b32_dpp") or k.endswith("_dpp"))
        lines.append("| `k_harmonic_sweep<%d, %d, %d>` | %s %d DPP moves among the other VALU" % (gh, jr, qr, mix_cells(mix), dpp))
    lines += ["", "One row of one lane (one harmonic of one frequency; at JR = 32 one of a harmonic's two columns), the path a wavefront "
              "takes when every phase is below kSincosFastMax."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--composed-steps", type=int, default=2)
    ap.add_argument("--composed-chunks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--static-only", action="store_true")
    a = ap.parse_args()
    old = open(a.out).read() if a.out and os.path.exists(a.out) else ""
    if a.static_only:
        text = with_block(old, "registers", register_table("c2_harmonics.o", REGISTER_NOTE, "k_harmonic_sweep"), TOOL)
        text = with_block(text, "instructions", instruction_table(), TOOL)
        if a.out:
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import harmonics as hm, ops, synth

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")
    lines = ["# gp.periodogram(nterms=H)'s sweep beside H one-term sweeps and beside ops.whitened_gram in chunks", "",
             "One process, steps alternating between the routes, %d timed steps each (composed: %d) after %d warm-up steps "
             "(composed: 1); ms: median (min .. max).  `sinusoids` (a) is H calls of the one-term sweep at h * freq: the same "
             "column work without the products between harmonics.  `composed` (b) is timed on its first %d chunks of "
             "30 // (2 H) frequencies and scaled to the grid.  The kernel's products are compared with the composed route's "
             "on those chunks before timing (worst distance in units of the standing criterion under the table)."
             % (a.steps, a.composed_steps, a.warmup, a.composed_chunks), "",
             "| B x N x J x F | H | route | ms | kernel / (a) | kernel / (b) | whole / (b) |", "|---|---|---|---|---|---|---|"]
    agree = []
    for B, N, J, F in (SHAPES if not a.quick else [(8, 256, 8, 100), (4, 128, 32, 40)]):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, flag = ops.factor(t, c, av, U, V)
        ok = flag == 0
        span = (t[:, -1] - t[:, 0])[:, None]
        for H in (2, 3, 4):
            # the top harmonic stays below the sampling rate
            freq = (2.0 * torch.pi / span * torch.linspace(1.0, N / (4.0 * H), F, dtype=torch.float64, device=dev)[None, :]).contiguous()
            fh = [(float(h) * freq).contiguous() for h in range(1, H + 1)]
            Y0 = torch.stack([torch.ones_like(y), y], dim=-1).contiguous()
            NC, HEAD = 2 * H, H * (2 * H + 1)
            Z0, T = torch.empty_like(Y0), torch.empty((B, F, HEAD + NC * 2), dtype=torch.float64, device=dev)
            T1 = [torch.empty((B, F, 7), dtype=torch.float64, device=dev) for _ in range(H)]
            n = 30 // NC
            chunks = [(lo, min(lo + n, F)) for lo in range(0, F, n)]
            timed = [ch for ch in chunks if ch[1] - ch[0] == n][:a.composed_chunks]
            A = torch.empty((B, N, 1 + NC * n), dtype=torch.float64, device=dev)
            S = torch.empty((B, 2 + NC * n, 2 + NC * n), dtype=torch.float64, device=dev)
            T2 = torch.zeros((B, timed[-1][1], HEAD + NC * 2), dtype=torch.float64, device=dev)
            iu = [(i, j) for i in range(NC) for j in range(i, NC)]

            def whole():
                ops.solve_lower(t, c, U, W, Y0, Z=Z0)
                ops.whitened_harmonics(t, c, U, W, d, Z0, freq, H, out=T)
                return hm.finish(hm.null_products(Z0, d), T, N, H, ok=ok).power

            def kernel():
                ops.whitened_harmonics(t, c, U, W, d, Z0, freq, H, out=T)

            def sinusoids():
                for h in range(H):
                    ops.whitened_sinusoids(t, c, U, W, d, Z0, fh[h], out=T1[h])

            def composed():
                for lo, hi in timed:
                    A[..., 0] = 1.0
                    for h in range(H):       # column 1 + NC k + i: column i of frequency lo + k
                        x = fh[h][:, None, lo:hi] * t[:, :, None]
                        torch.cos(x, out=A[..., 1 + 2 * h::NC])
                        torch.sin(x, out=A[..., 2 + 2 * h::NC])
                    ops.whitened_gram(t, c, U, W, d, A, y, S=S)
                    k, q = 1 + NC * torch.arange(n, device=dev), 1 + NC * n
                    for m, (i, j) in enumerate(iu):
                        T2[:, lo:hi, m] = S[:, k + i, k + j]
                    for i in range(NC):
                        T2[:, lo:hi, HEAD + 2 * i], T2[:, lo:hi, HEAD + 2 * i + 1] = S[:, k + i, 0], S[:, k + i, q]

            whole()
            composed()
            torch.cuda.synchronize()
            got, ref = T[ok][:, :T2.shape[1]], T2[ok]
            tol = 1e-10 * ref.abs() + 1e-12 * ref.abs().amax(dim=(1, 2), keepdim=True)
            worst = float(((got - ref).abs() / tol).max())
            assert worst < 1e4, "the two routes disagree: %g" % worst
            agree.append("%d x %d x %d x %d, H = %d: %.3g" % (B, N, J, F, H, worst))
            out = alternate({"whole": (whole, None), "kernel": (kernel, None), "sinusoids": (sinusoids, None),
                             "composed": (composed, a.composed_steps)}, a.steps, a.warmup)
            scale = F / float(timed[-1][1])
            out["composed"] = tuple(v * scale for v in out["composed"])
            for op, st in out.items():
                lines.append("| %d x %d x %d x %d | %d | %s | %.3f (%.3f .. %.3f) | %s | %s | %s |"
                             % (B, N, J, F, H, op + (" (scaled x %.0f)" % scale if op == "composed" else ""), st[0], st[1], st[2],
                                "%.2f" % (out["kernel"][0] / out["sinusoids"][0]) if op == "kernel" else "",
                                "%.4f" % (out["kernel"][0] / out["composed"][0]) if op == "kernel" else "",
                                "%.4f" % (out["whole"][0] / out["composed"][0]) if op == "whole" else ""))
                print(lines[-1], flush=True)
            del freq, fh, Y0, Z0, T, T1, A, S, T2
            torch.cuda.empty_cache()
        del t, c, av, U, V, y, d, W
        torch.cuda.empty_cache()
    lines += ["", "Worst |kernel - composed| product in units of the standing criterion: " + "; ".join(agree) + "."]
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
