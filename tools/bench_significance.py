# -*- coding: utf-8 -*-
"""What the Monte-Carlo false-alarm probability of the three searches costs (csrc/c2_trial_project.hip,
gp.search_significance) beside the only route there was before it -- one call of the search entry point per draw -- on one
device, in ONE fresh process:

    python tools/bench_significance.py [--steps 5] [--out profiles/significance.md] [--quick]
    python tools/bench_significance.py --static-only --out profiles/significance.md    # no GPU: the register table

  kernel   ops.trial_projections alone on all draws (the figure the share of the fp64 rate is taken from)
  fused    gp.search_significance with given normals: the search's own sweep once, one solve_upper with `draws` columns,
           ops.trial_projections, significance.null_statistics (torch) and the maximum over the trials
  loop     for each draw y_r = mean + gp.dot_tril(n_r), gp.periodogram / transit_search / keplerian_search, nanmax: timed on
           --loop-draws draws a step and scaled to `draws` (every draw is one independent call: the cost is linear)

alternating step by step at B x N x J x K = 1 x 4096 x 8 x 4096 and 64 x 4096 x 8 x 4096 with 128 and 1024 draws, for each
kind, every step timed by its own pair of HIP events after a warm-up.  The two routes' maxima over the looped draws are
compared before timing.

The kernel's yardstick is the vector fp64 rate of tools/bench_periodogram.py, 39.3e12 fp64 instructions per lane and second:
its B K N R C multiply-adds, each what one lane of a v_fma_f64 does, over the time and over that rate.  The matrix pipe's own
ceiling is another matter: see the note the profile carries."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trial_static import kept_block, register_table, with_block  # noqa: E402

FP64_PEAK = 78.6e12 / 2.0   # fp64 VALU instructions per lane and second
SHAPES = [(1, 4096, 8, 4096), (64, 4096, 8, 4096)]
DRAWS = (128, 1024)
TOOL = "tools/bench_significance.py --static-only"
KINDS = ("periodogram", "transit", "keplerian")


def registers():
    table = register_table("c2_trial_project.o")
    if table is None:
        return None
    # (register_table's closing line describes the sweeps' template parameters: this kernel has its own)
    return table.rsplit("\n\n", 1)[0] + "\n\n`k_project<Column, NQ>`: Column the kind's column source (csrc/c2_trial_columns.hpp); NQ = RB / 16 " \
        "tiles of 16 draws a wavefront.  No scratch and no spilled register at any instantiation."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--loop-draws", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--static-only", action="store_true")
    a = ap.parse_args()
    old = open(a.out).read() if a.out and os.path.exists(a.out) else ""
    if a.static_only:
        text = with_block(old, "registers", registers(), TOOL)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import gp as G, ops, synth, transit as tr

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")

    class Matrices:   # a kernel that hands the synthetic celerite matrices to GaussianProcess.compute
        def __init__(self, c, a, U, V):
            self.m = (c, a, U, V)

        def get_celerite_matrices(self, t, diag):
            return self.m

    def stats(ms):
        ms = sorted(ms)
        return ms[len(ms) // 2], ms[0], ms[-1]

    def alternate(runs, steps):
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for k in runs}
        torch.cuda.synchronize()
        for i in range(steps):
            for k, fn in runs.items():
                ev[k][i][0].record()
                fn()
                ev[k][i][1].record()
        torch.cuda.synchronize()
        return {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}

    lines = ["# gp.search_significance beside one search call per draw", "",
             "One process, steps alternating between the routes, %d timed steps each after %d warm-up; ms: median (min .. max).  "
             "loop: timed on %d draws a step and scaled to the draw count (one independent call per draw).  The routes' per-draw "
             "maxima are compared before timing (worst distance in units of the standing criterion under the table).  Share of "
             "the vector fp64 rate: B K N R C multiply-adds over the kernel's time over 39.3e12 a second.  At B = 64 the fused "
             "route takes the trials in blocks of 1024 (`max_trials`), which bounds its (B, K, C, R) and (B, K, R) arrays."
             % (a.steps, a.warmup, a.loop_draws), "",
             "| kind | B x N x J x K | draws | kernel ms | share of the vector fp64 rate | fused ms | loop ms (scaled) | loop / fused |",
             "|---|---|---|---|---|---|---|---|"]
    agree = []
    for B, N, J, K in (SHAPES if not a.quick else [(2, 256, 8, 100)]):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        gp = G.GaussianProcess(Matrices(c, av, U, V), mean=0.0)
        gp.compute(t, diag=torch.ones((B, N), dtype=torch.float64, device=dev), check_sorted=False, quiet=True)
        span = (t[:, -1] - t[:, 0])[:, None]
        gen = torch.Generator(device="cpu").manual_seed(K)
        w = 2.0 * torch.pi / span * torch.linspace(1.0, N / 4.0, K, dtype=torch.float64, device=dev)[None, :]
        e = (0.9 * torch.rand((1, K), dtype=torch.float64, generator=gen)).to(dev).expand(B, K)
        tp = t[:, :1] + torch.rand((1, K), dtype=torch.float64, generator=gen).to(dev) * (2.0 * torch.pi / w)
        dur = span / 50.0 * (1.0 + torch.rand((1, K), dtype=torch.float64, generator=gen).to(dev))
        trials = {"periodogram": w.contiguous(), "keplerian": torch.stack([w, e, tp], dim=-1).contiguous(),
                  "transit": torch.stack([2.0 * torch.pi / w + dur, tp, dur, 0.25 * dur], dim=-1).contiguous()}
        assert bool(tr.in_domain(trials["transit"]).all())
        search = {"periodogram": gp.periodogram, "transit": gp.transit_search, "keplerian": gp.keplerian_search}
        nm = {"periodogram": dict(normalization="chi2"), "transit": {}, "keplerian": dict(normalization="chi2")}
        for draws in (DRAWS if not a.quick else (40,)):
            normals = torch.randn((B, N, draws), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(draws))
            alpha = ops.solve_upper(gp._t, gp._c, gp._U, gp._W, (normals * torch.rsqrt(gp._d)[..., None]).contiguous())
            for kind in KINDS:
                C = ops.TRIAL_KINDS[kind][2]
                P = torch.empty((B, K, C, draws), dtype=torch.float64, device=dev)
                kw = dict(normalization="chi2", normals=normals, max_trials=1024 if B > 1 else None)
                res = {}

                def kernel():
                    ops.trial_projections(kind, gp._t, alpha, trials[kind], out=P)

                def fused():
                    res["fused"] = gp.search_significance(kind, y, trials[kind], **kw).null_maxima

                def loop():
                    top = []
                    for r in range(a.loop_draws):
                        yr = gp.dot_tril(normals[..., r].contiguous())
                        s = search[kind](yr, trials[kind], **nm[kind])
                        top.append(torch.where(torch.isnan(s), torch.full_like(s, -float("inf")), s).amax(dim=1))
                    res["loop"] = torch.stack(top, dim=1)

                fused()
                loop()
                torch.cuda.synchronize()
                p1, p2 = res["fused"][:, :a.loop_draws], res["loop"]
                ok = (gp._flag == 0)[:, None].expand_as(p2)
                tol = 1e-10 * p2.abs() + 1e-12 * p2.abs().amax(dim=1, keepdim=True)
                worst = float(((p1 - p2).abs() / tol)[ok].max())
                assert worst < 1e4, "the two routes disagree: %g" % worst
                agree.append("%s %d x %d: %.3g" % (kind, B, draws, worst))
                out = alternate({"kernel": kernel, "fused": fused, "loop": loop}, a.steps)
                scaled = out["loop"][0] * draws / a.loop_draws
                share = 100.0 * (B * K * N * draws * C / (out["kernel"][0] * 1e-3)) / FP64_PEAK
                lines.append("| %s | %d x %d x %d x %d | %d | %.3f (%.3f .. %.3f) | %.1f %% | %.2f (%.2f .. %.2f) | %.1f | %.1f |"
                             % (kind, B, N, J, K, draws, *out["kernel"], share, *out["fused"], scaled, scaled / out["fused"][0]))
                print(lines[-1], flush=True)
                del P
            del normals, alpha
            torch.cuda.empty_cache()
    lines += ["", "Worst |fused - loop| per-draw maximum in units of the standing criterion (kind B x draws): " + "; ".join(agree) + "."]
    text = "\n".join(lines) + "\n"
    text = with_block(text, "registers", kept_block(old, "registers", TOOL), TOOL)
    if "<!-- notes -->" in old:   # whatever follows the generated part of an earlier file (hand-written notes) is kept
        text += "\n<!-- notes -->" + old.split("<!-- notes -->", 1)[1]
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
