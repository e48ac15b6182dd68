# -*- coding: utf-8 -*-
"""What the tabulated-shape search under correlated noise costs (csrc/c2_shapes.hip, csrc/c2_trial_project.hip) beside the
box sweep it is modelled on and beside the only route there was before it, on one device, in ONE fresh process:

    python tools/bench_shapes.py [--steps 10] [--out profiles/shape_search.md] [--quick]
    python tools/bench_shapes.py --static-only --out profiles/shape_search.md   # no GPU: registers, occupancy, instruction mix

  transits    ops.whitened_transits with tau = 0 on the same trials: the existing kernel, the yardstick, timed in this process
  box         ops.whitened_shapes with the all-ones S = 2 bank (the same column, through the table)
  limb        ops.whitened_shapes with shapes.limb_darkened at S = 65
  composed    ops.whitened_gram on [1 | b_k ... | y] in chunks of at most 30 trials (Q <= 32), the limb-darkened columns built
              by torch interpolation inside the timed region, then shapes.finish on the blocks of S

alternating step by step at B x N x J x K = 64 x 4096 x 8 x 4096, 1 x 4096 x 8 x 4096, 1024 x 1024 x 4 x 1024 and
64 x 4096 x 32 x 512 on folded trials, every step timed by its own pair of HIP events after a warm-up; the composed route
takes hundreds of launches a step and is given fewer steps (--composed-steps).  Then, at the two 4096 x 8 x 4096 shapes,

  significance  gp.shape_search_significance with 128 and 1024 given normals
  loop          one gp.shape_search per draw y_r = mean + gp.dot_tril(n_r), timed on --loop-draws draws and scaled

No ratio is set in advance.  The static part needs the built objects and the compiler, not a device."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trial_static import (MIX_HEAD, alternate, fp64_valu, kept_block, mix_cells, register_table, row_loop_mix, short_name, sorted_rows,  # noqa: E402
                          sweep_asm, sweep_label, sweep_registers, sweep_symbol, with_block)

SHAPES = [(64, 4096, 8, 4096), (1, 4096, 8, 4096), (1024, 1024, 4, 1024), (64, 4096, 32, 512)]
DRAWS = (128, 1024)
CHUNK = 30
TOOL = "tools/bench_shapes.py --static-only"
VGPRS, LDS_CU, WAVES_MAX = 512, 160 * 1024, 8       # registers per lane and SIMD, LDS bytes per compute unit, wavefronts per SIMD
BANK_PAIRS = 16 * 1024                              # a bank at the cap staged as (value, difference) pairs


def occupancy_table():
    """Waves per SIMD that registers and LDS each allow for every k_trial_sweep<Shape, JR, QR>, and what a bank staged in
    LDS would have left: the figures behind reading the nodes through the vector cache."""
    rows = sorted_rows("c2_shapes.o", "k_trial_sweep")
    if not rows:
        return None
    lines = ["| kernel | registers | waves / SIMD by registers | LDS bytes | waves / SIMD by LDS | by LDS with a 16 KB bank staged |",
             "|---|---|---|---|---|---|"]
    hit = 0
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        by_reg = min(WAVES_MAX, VGPRS // (8 * ((vg + ag + 7) // 8)))
        by_lds, by_bank = (LDS_CU // lds) / 4.0, (LDS_CU // (lds + BANK_PAIRS)) / 4.0      # one-wave blocks, four SIMDs
        hit += by_bank < min(by_reg, by_lds)
        lines.append("| `%s` | %d | %d | %d | %.2f | %.2f |" % (short_name(name), vg + ag, by_reg, lds, min(WAVES_MAX, by_lds), by_bank))
    lines += ["", "512 registers per lane and SIMD in steps of 8, 160 KiB of LDS per compute unit shared by its four SIMDs, blocks of one "
              "wavefront.  As shipped (the bank read through the vector cache) registers set the occupancy at every instantiation; a bank at "
              "the cap staged in LDS would have set it, lower, at %d of %d." % (hit, len(rows))]
    return "\n".join(lines)


def registers():
    a = sweep_registers("shape")
    b = register_table("c2_trial_project.o", " (`k_project<Shape, NQ>`: NQ = C2_SHAPE_DRAWS / 16 tiles of 16 draws a wavefront).", "Shape")
    occ = occupancy_table()
    return None if a is None or b is None or occ is None else a + "\n\n" + b + "\n\n" + occ


def instruction_table():
    """The row loop's instruction mix per width beside the transit's; the forward-skipped region that holds the gather (the
    global loads of the two nodes) is counted apart."""
    lines = [MIX_HEAD + " the skipped block (all) |", "|---|---|---|---|---|---|---|---|"]
    per_row = {}
    for search, skip in (("shape", "global_load"), ("transit", "v_div_fmas_f64")):
        asm = sweep_asm(search)
        if asm is None:
            return None
        for jr, qr in ((4, 2), (8, 2), (16, 2), (32, 2)):
            c, skipped = row_loop_mix(asm, sweep_symbol(search, jr, qr), skip)
            per_row[(search, jr)] = fp64_valu(c)
            lines.append("| `%s` | %s %d |" % (sweep_label(search, jr, qr), mix_cells(c), sum(skipped.values())))
    lines += ["", "One row of one lane (one trial), the path a wavefront takes when no lane needs the skipped block: for the shape the "
              "two node loads (entered when any lane is in an event), for the transit the ramp's division.  fp64 VALU per lane-row, "
              "machine-readable: " + " ".join("%s:JR%d=%d" % (k[0], k[1], v) for k, v in sorted(per_row.items()))]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--composed-steps", type=int, default=3)
    ap.add_argument("--loop-draws", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--static-only", action="store_true")
    a = ap.parse_args()
    old = open(a.out).read() if a.out and os.path.exists(a.out) else ""
    if a.static_only:
        text = with_block(old, "registers", registers(), TOOL)
        text = with_block(text, "instructions", instruction_table(), TOOL)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import gp as G, ops, periodogram as pg, shapes as sh, synth

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")

    class Matrices:   # a kernel that hands the synthetic celerite matrices to GaussianProcess.compute
        def __init__(self, c, a, U, V):
            self.m = (c, a, U, V)

        def get_celerite_matrices(self, t, diag):
            return self.m

    S = 65
    limb = sh.stack(sh.limb_darkened(0.1, 0.3, 0.4, 0.3, S)).to(dev)
    ones = sh.stack(sh.box()).to(dev)
    lines = ["# gp.shape_search's sweep beside ops.whitened_transits and beside ops.whitened_gram in chunks of %d trials" % CHUNK, "",
             "One process, steps alternating between the routes, %d timed steps each (composed: %d) after %d warm-up steps "
             "(composed: 1); ms: median (min .. max).  Trials: folded (periods from a fiftieth to a third of the baseline, widths "
             "2 %% of the period, epochs uniform over the baseline), shared by the batch; `transits` is ops.whitened_transits with "
             "tau = 0 on the same trials, the yardstick; `box` and `limb` are ops.whitened_shapes with the all-ones S = 2 bank and with "
             "shapes.limb_darkened at S = %d; `composed` builds the limb-darkened columns by torch interpolation and runs "
             "ops.whitened_gram.  The routes' delta_chi2 are compared before timing (worst distance in units of the standing "
             "criterion under the table)." % (a.steps, a.composed_steps, a.warmup, S), "",
             "| B x N x J x K | route | ms | over transits | composed / limb |", "|---|---|---|---|---|"]
    sig_lines = ["", "## gp.shape_search_significance beside one gp.shape_search per draw", "",
                 "The limb-darkened bank; loop: timed on %d draws a step and scaled to the draw count; `projection` is "
                 "ops.shape_projections alone on all draws.  At B = 64 the fused route takes the trials in blocks of 1024 "
                 "(`max_trials`)." % a.loop_draws, "",
                 "| B x N x J x K | draws | projection ms | significance ms | loop ms (scaled) | loop / significance |", "|---|---|---|---|---|---|"]
    agree, sig_agree = [], []
    for si, (B, N, J, K) in enumerate(SHAPES if not a.quick else [(8, 256, 8, 100), (4, 128, 32, 40)]):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        d, W, flag = ops.factor(t, c, av, U, V)
        t_lo, span = float(t.min()), float(t.max() - t.min())
        gen = torch.Generator(device="cpu").manual_seed(1)
        P = span / torch.linspace(3.0, 50.0, K, dtype=torch.float64)
        trials = torch.stack([P, t_lo + span * torch.rand(K, dtype=torch.float64, generator=gen), 0.02 * P, torch.zeros_like(P)], dim=1)
        trials = trials.to(dev).contiguous()
        Y0 = torch.stack([torch.ones_like(y), y], dim=-1).contiguous()
        Z0 = ops.solve_lower(t, c, U, W, Y0)
        T, Tb, Tt = [torch.empty((B, K, 3), dtype=torch.float64, device=dev) for _ in range(3)]
        ok = flag == 0
        chunks = [(lo, min(lo + CHUNK, K)) for lo in range(0, K, CHUNK)]
        T2 = torch.empty_like(T)
        A = torch.empty((B, N, 1 + CHUNK), dtype=torch.float64, device=dev)
        Sg = torch.empty((B, 2 + CHUNK, 2 + CHUNK), dtype=torch.float64, device=dev)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        flat = limb.reshape(-1)
        res = {}

        def transits():
            ops.whitened_transits(t, c, U, W, d, Z0, trials, out=Tt)

        def box():
            ops.whitened_shapes(t, c, U, W, d, Z0, trials, ones, out=Tb)

        def limb_():
            ops.whitened_shapes(t, c, U, W, d, Z0, trials, limb, out=T)

        def composed():
            S0 = None
            for lo, hi in chunks:
                n = hi - lo
                Pc, t0, w, s = [trials[lo:hi, i] for i in range(4)]
                x = t[:, :, None] - t0
                phi = x - torch.round(x * torch.where(Pc != 0, 1.0 / Pc, zero)) * Pc
                u = 0.5 * w - phi.abs()
                g = torch.clamp((phi + 0.5 * w) * ((S - 1.0) / w), 0.0, S - 1.0)
                i = torch.clamp(torch.floor(g), max=S - 2.0)
                idx = (s * S + i).long()
                lo_v, hi_v = flat[idx], flat[idx + 1]
                Ac, Sc = (A, Sg) if n == CHUNK else (torch.empty((B, N, 1 + n), dtype=torch.float64, device=dev),
                                                     torch.empty((B, 2 + n, 2 + n), dtype=torch.float64, device=dev))
                Ac[..., 0] = 1.0
                Ac[..., 1:] = torch.where(u < 0, zero, lo_v + (g - i) * (hi_v - lo_v))
                ops.whitened_gram(t, c, U, W, d, Ac, y, S=Sc)
                k, q = torch.arange(1, 1 + n, device=dev), 1 + n
                T2[:, lo:hi, 0], T2[:, lo:hi, 1], T2[:, lo:hi, 2] = Sc[:, k, k], Sc[:, k, 0], Sc[:, k, q]
                S0 = Sc[:, [0, q]][:, :, [0, q]]
            res["composed"] = sh.finish(S0, T2, N, ok=ok, trials=trials, n_shapes=1).delta_chi2

        transits(); box(); limb_(); composed()
        torch.cuda.synchronize()
        p1 = sh.finish(pg.null_products(Z0, d), T, N, ok=ok, trials=trials, n_shapes=1).delta_chi2
        p2 = res["composed"]
        fin = torch.isfinite(p2) & ok[:, None]
        tol = 1e-10 * p2.abs() + 1e-12 * torch.nan_to_num(p2).abs().amax(dim=1, keepdim=True)
        worst = float(((p1 - p2).abs() / tol)[fin].max())
        assert bool(torch.equal(torch.isnan(p1), torch.isnan(p2))) and worst < 1e4, "the two routes disagree: %g" % worst
        agree.append("%d x %d x %d x %d: %.3g (box bank bit-identical to whitened_transits: %s)" % (B, N, J, K, worst, bool(torch.equal(Tb, Tt))))
        out = alternate({"transits": (transits, None), "box": (box, None), "limb": (limb_, None), "composed": (composed, a.composed_steps)},
                        a.steps, a.warmup)
        for op, st in out.items():
            lines.append("| %d x %d x %d x %d | %s | %.3f (%.3f .. %.3f) | %s | %s |"
                         % (B, N, J, K, op, st[0], st[1], st[2], "%.3f" % (st[0] / out["transits"][0]) if op in ("box", "limb") else "",
                            "%.1f" % (out["composed"][0] / out["limb"][0]) if op == "composed" else ""))
            print(lines[-1], flush=True)
        del A, Sg, T2
        if si < 2:                                            # the two 4096 x 8 x 4096 shapes: the significance route
            gp = G.GaussianProcess(Matrices(c, av, U, V), mean=0.0)
            gp.compute(t, diag=torch.ones((B, N), dtype=torch.float64, device=dev), check_sorted=False, quiet=True)
            for draws in (DRAWS if not a.quick else (40,)):
                normals = torch.randn((B, N, draws), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(draws))
                alpha = ops.solve_upper(gp._t, gp._c, gp._U, gp._W, (normals * torch.rsqrt(gp._d)[..., None]).contiguous())
                Pj = torch.empty((B, K, 1, draws), dtype=torch.float64, device=dev)
                kw = dict(normalization="chi2", normals=normals, max_trials=1024 if B > 1 else None)

                def projection():
                    ops.shape_projections(gp._t, alpha, trials, limb, out=Pj)

                def significance():
                    res["sig"] = gp.shape_search_significance(y, trials, limb, **kw).null_maxima

                def loop():
                    top = []
                    for r in range(a.loop_draws):
                        sr = gp.shape_search(gp.dot_tril(normals[..., r].contiguous()), trials, limb)
                        top.append(torch.where(torch.isnan(sr), torch.full_like(sr, -float("inf")), sr).amax(dim=1))
                    res["loop"] = torch.stack(top, dim=1)

                significance(); loop()
                torch.cuda.synchronize()
                q1, q2 = res["sig"][:, :a.loop_draws], res["loop"]
                okk = (gp._flag == 0)[:, None].expand_as(q2)
                tol = 1e-10 * q2.abs() + 1e-12 * q2.abs().amax(dim=1, keepdim=True)
                worst = float(((q1 - q2).abs() / tol)[okk].max())
                assert worst < 1e4, "the two routes disagree: %g" % worst
                sig_agree.append("%d x %d: %.3g" % (B, draws, worst))
                o2 = alternate({"projection": (projection, None), "significance": (significance, None), "loop": (loop, None)}, max(3, a.steps // 2), a.warmup)
                scaled = o2["loop"][0] * draws / a.loop_draws
                sig_lines.append("| %d x %d x %d x %d | %d | %.3f (%.3f .. %.3f) | %.2f (%.2f .. %.2f) | %.1f | %.1f |"
                                 % (B, N, J, K, draws, *o2["projection"], *o2["significance"], scaled, scaled / o2["significance"][0]))
                print(sig_lines[-1], flush=True)
                del normals, alpha, Pj
            del gp
        del t, c, av, U, V, y, d, W, trials, Y0, Z0, T, Tb, Tt
        torch.cuda.empty_cache()
    lines += ["", "Worst |limb - composed| delta_chi2 in units of the standing criterion: " + "; ".join(agree) + "."]
    sig_lines += ["", "Worst |significance - loop| per-draw maximum in units of the standing criterion (B x draws): " + "; ".join(sig_agree) + "."]
    text = "\n".join(lines + sig_lines) + "\n"
    for key in ("registers", "instructions"):
        text = with_block(text, key, kept_block(old, key, TOOL), TOOL)
    if "<!-- notes -->" in old:   # whatever follows the generated part of an earlier file (hand-written notes) is kept
        text += "\n<!-- notes -->" + old.split("<!-- notes -->", 1)[1]
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
