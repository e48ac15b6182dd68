# -*- coding: utf-8 -*-
"""What the Monte-Carlo false-alarm probability of the multi-harmonic periodogram costs (csrc/c2_harmonic_trials.hip,
gp.search_significance(..., nterms=H)) beside the two routes there were before it, on one device, in ONE fresh process:

    python tools/bench_harmonic_significance.py [--steps 3] [--out profiles/harmonic_significance.md] [--quick]
    python tools/bench_harmonic_significance.py --static-only --out profiles/harmonic_significance.md   # no GPU: the registers

  kernel    ops.harmonic_null_chi2 alone on all draws, D (B, F, R) caller-owned
  fused     gp.search_significance("periodogram", nterms=H) with given normals: the harmonic sweep once, one solve_upper with
            `draws` columns, ops.harmonic_null_chi2, the normalisation and the maximum over the frequencies
  composed  (a) the same call with the per-draw statistic composed from what there was: H calls of
            ops.trial_projections("periodogram") at h * freq, the permuting copy to (B, F, 2 H, R), harmonics.null_statistics
            (torch), the maximum
  loop      (b) for each draw y_r = mean + gp.dot_tril(n_r), gp.periodogram(nterms=H), nanmax: timed on --loop-draws draws a
            step and scaled to `draws` (every draw is one independent call: the cost is linear)

alternating step by step at the shapes of profiles/harmonics.md with 128 and 1024 draws, every step timed by its own pair of
HIP events after a warm-up.  fused and composed take the frequencies in the same blocks (`max_trials`), sized so that the
composed route's (B, F, 2 H, R) block stays at 1 GiB.  The routes' maxima are compared before timing."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from trial_static import kept_block, marks, register_table, short_name  # noqa: E402

SHAPES = [(64, 4096, 8, 4096), (1, 4096, 8, 4096), (1024, 1024, 4, 1024), (64, 4096, 32, 512)]
DRAWS = (128, 1024)
TOOL = "tools/bench_harmonic_significance.py --static-only"
LLVM = "/opt/rocm/lib/llvm/bin"
HEAD = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]


def shipped():
    table = register_table("c2_harmonic_trials.o")
    if table is None:
        return None
    return table.rsplit("\n\n", 1)[0] + "\n\n`k_project<Harmonics<H>, NQ>` (c2_harmonic_projections) and `k_harmonic_null<H, NQ>` " \
        "(c2_harmonic_null_chi2): NQ = C2_HARMONIC_DRAWS_H / 16 tiles of 16 draws a wavefront.  No scratch and no spilled register at " \
        "any instantiation; above 256 registers a SIMD holds one wavefront."


def candidates():
    """The registers of every candidate NQ (tools/ubench/harmonic_null_candidates.hip), compiled with the build's flags; None
    without the compiler."""
    from celerite2_amd import build

    if not (os.path.exists(build.HIPCC) and os.path.exists(LLVM + "/llvm-readelf")):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "candidates.o")
        flags = [f for f in build.HIPFLAGS if f != "-shared"]
        subprocess.run([build.HIPCC] + flags + ["-c", os.path.join(ROOT, "tools", "ubench", "harmonic_null_candidates.hip"), "-o", obj],
                       check=True)
        # (llvm-objdump --offloading writes the bundle's members next to its input)
        subprocess.run([LLVM + "/llvm-objdump", "--offloading", obj], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", glob.glob(obj + ".*hipv4-amdgcn*")[0]], capture_output=True, text=True).stdout
    rows = []
    for b in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        f = lambda key: int(re.search(r"\.%s:\s*(\d+)" % key, b).group(1))
        rows.append([re.search(r"\.name:\s*(\S+)", b).group(1), f("vgpr_count"), int(b.split("\n")[0].strip()), f("sgpr_count"),
                     f("group_segment_fixed_size"), f("private_segment_fixed_size"), f("vgpr_spill_count")])
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    rows = sorted((short_name(n),) + tuple(r[1:]) for r, n in zip(rows, names))
    return "\n".join(HEAD + ["| `%s` | %d (%d) | %d | %d | %d | %d |" % r for r in rows])


def block(text, key, title, table):
    """`text` with the marked block `key` replaced by (or, under `title`, appended as) `table`."""
    begin, end = marks(key, TOOL)
    table = table or "(neither the built objects nor the compiler are on this machine: run `python %s --out <this file>` where the library was built)" % TOOL
    body = begin + "\n" + table + "\n" + end
    if begin in text and end in text:
        head, rest = text.split(begin, 1)
        return head + body + rest.split(end, 1)[1]
    return text + "\n## %s\n\n" % title + body + "\n"


def static_blocks(text, fresh):
    shipped_t, cand_t = (shipped(), candidates()) if fresh else (kept_block(text[1], "registers", TOOL), kept_block(text[1], "candidates", TOOL))
    out = block(text[0], "registers", "Registers of the shipped kernels (gfx950, from the built objects)", shipped_t)
    return block(out, "candidates", "Registers of every candidate NQ (gfx950, tools/ubench/harmonic_null_candidates.hip)", cand_t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--loop-draws", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--kernel-only", action="store_true", help="time ops.harmonic_null_chi2 alone (the A/B of two builds' draw tiles)")
    ap.add_argument("--static-only", action="store_true")
    a = ap.parse_args()
    old = open(a.out).read() if a.out and os.path.exists(a.out) else ""
    if a.static_only:
        text = static_blocks((old, old), True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(text)
        print(text)
        return

    import torch
    from celerite2_amd import gp as G, harmonics as hm, ops, synth
    from trial_static import alternate

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")

    class Matrices:   # a kernel that hands the synthetic celerite matrices to GaussianProcess.compute
        def __init__(self, c, a, U, V):
            self.m = (c, a, U, V)

        def get_celerite_matrices(self, t, diag):
            return self.m

    def nanmax(s):
        return torch.where(torch.isnan(s), torch.full_like(s, -float("inf")), s).amax(dim=1)

    def distance(p1, p2, ok):
        tol = 1e-10 * p2.abs() + 1e-12 * p2.abs().amax(dim=1, keepdim=True)
        return float(((p1 - p2).abs() / tol)[ok.expand_as(p2)].max())

    lines = ["# gp.search_significance(nterms=H) beside the composed route and beside one periodogram call per draw", "",
             "One process, steps alternating between the routes, %d timed steps each after %d warm-up; ms: median (min .. max).  "
             "composed (a): H one-term projections at h * freq, the permuting copy, `harmonics.null_statistics`.  loop (b): timed on "
             "%d draws a step and scaled to the draw count.  fused and composed take the frequencies in the same blocks (the column "
             "`block`).  The routes' per-draw maxima are compared before timing (worst distance in units of the standing criterion "
             "under the table)." % (a.steps, a.warmup, a.loop_draws), "",
             "| B x N x J x F | H | draws | block | kernel ms | fused ms | composed ms (a) | loop ms (b, scaled) | (a) / fused | (b) / fused |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    agree = []
    for B, N, J, F in (SHAPES if not a.quick else [(2, 256, 8, 100)]):
        t, c, av, U, V, y = synth.device_batch_fast(0, B, N, J, dev)
        gp = G.GaussianProcess(Matrices(c, av, U, V), mean=0.0)
        gp.compute(t, diag=torch.ones((B, N), dtype=torch.float64, device=dev), check_sorted=False, quiet=True)
        span = (t[:, -1] - t[:, 0])[:, None]
        w = (2.0 * torch.pi / span * torch.linspace(1.0, N / 16.0, F, dtype=torch.float64, device=dev)[None, :]).contiguous()
        ok = (gp._flag == 0)[:, None]
        for draws in (DRAWS if not a.quick else (40,)):
            normals = torch.randn((B, N, draws), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(draws))
            scaled_n = (normals * torch.rsqrt(gp._d)[..., None]).contiguous()
            alpha = ops.solve_upper(gp._t, gp._c, gp._U, gp._W, scaled_n)
            for H in (2, 3, 4):
                step = max(16, min(F, 2 ** 30 // (B * 2 * H * draws * 8)))
                Z0 = gp._whitened_columns(y, "mean")
                S0 = hm.null_products(Z0, gp._d)
                T = ops.whitened_harmonics(gp._t, gp._c, gp._U, gp._W, gp._d, Z0, w, H)
                fac = hm.null_factors(S0, T, N, H, gp._flag == 0)
                s_yy, G0Y = (normals * normals).sum(dim=1), torch.matmul(Z0[..., :-1].transpose(1, 2), scaled_n)
                Vd, _ = hm.null_draws(fac, G0Y, s_yy)
                D = torch.empty((B, F, draws), dtype=torch.float64, device=dev)
                res = {}

                def kernel():
                    ops.harmonic_null_chi2(gp._t, alpha, w, H, fac.Lm, fac.Xt, Vd, out=D)

                def fused():
                    res["fused"] = gp.search_significance("periodogram", y, w, normalization="chi2", normals=normals, nterms=H,
                                                          max_trials=step).null_maxima

                def composed():   # gp.search_significance's steps with the per-draw statistic from the one-term pieces
                    Zc = gp._whitened_columns(y, "mean")
                    Sc = hm.null_products(Zc, gp._d)
                    Tc = ops.whitened_harmonics(gp._t, gp._c, gp._U, gp._W, gp._d, Zc, w, H)
                    hm.finish(Sc, Tc, N, H, "chi2", ok=gp._flag == 0)
                    sc = (normals * torch.rsqrt(gp._d)[..., None]).contiguous()
                    syy, g0y = (normals * normals).sum(dim=1), torch.matmul(Zc[..., :-1].transpose(1, 2), sc)
                    al = ops.solve_upper(gp._t, gp._c, gp._U, gp._W, sc)
                    best = torch.full((B, draws), -float("inf"), dtype=torch.float64, device=dev)
                    for k0 in range(0, F, step):
                        wk = w[:, k0:k0 + step].contiguous()
                        P = torch.stack([ops.trial_projections("periodogram", gp._t, al, (h * wk).contiguous()) for h in range(1, H + 1)], dim=2)
                        P = P.reshape(B, wk.shape[1], 2 * H, draws).contiguous()
                        s = hm.null_statistics(Sc, Tc[:, k0:k0 + step], g0y, syy, P, N, H, normalization="chi2", ok=gp._flag == 0)
                        best = torch.maximum(best, nanmax(s))
                        del P, s
                    res["composed"] = best

                def loop():
                    top = []
                    for r in range(a.loop_draws):
                        yr = gp.dot_tril(normals[..., r].contiguous())
                        top.append(nanmax(gp.periodogram(yr, w, normalization="chi2", nterms=H)))
                    res["loop"] = torch.stack(top, dim=1)

                runs = {"kernel": (kernel, None)}
                if not a.kernel_only:
                    fused(), composed(), loop()
                    torch.cuda.synchronize()
                    wa, wb = distance(res["fused"], res["composed"], ok), distance(res["fused"][:, :a.loop_draws], res["loop"], ok)
                    assert max(wa, wb) < 1e4, "the routes disagree: %g, %g" % (wa, wb)
                    agree.append("%d x %d x %d x %d, H = %d, %d draws: %.3g (a), %.3g (b)" % (B, N, J, F, H, draws, wa, wb))
                    runs.update(fused=(fused, None), composed=(composed, None), loop=(loop, None))
                out = alternate(runs, a.steps, a.warmup)
                cell = lambda k: "%.2f (%.2f .. %.2f)" % out[k] if k in out else ""
                ratio = lambda x: "%.2f" % (x / out["fused"][0]) if "fused" in out else ""
                lp = out["loop"][0] * draws / a.loop_draws if "loop" in out else None
                lines.append("| %d x %d x %d x %d | %d | %d | %d | %s | %s | %s | %s | %s | %s |"
                             % (B, N, J, F, H, draws, step, cell("kernel"), cell("fused"), cell("composed"), "%.1f" % lp if lp else "",
                                ratio(out["composed"][0]) if "composed" in out else "", ratio(lp) if lp else ""))
                print(lines[-1], flush=True)
                del D, T, fac, Vd
                res.clear()
                torch.cuda.empty_cache()
            del normals, alpha, scaled_n
            torch.cuda.empty_cache()
    lines += ["", "Worst |fused - other route| per-draw maximum in units of the standing criterion: " + "; ".join(agree) + "."]
    text = static_blocks(("\n".join(lines) + "\n", old), False)
    if "<!-- notes -->" in old:   # whatever follows the generated part of an earlier file (hand-written notes) is kept
        text += "\n<!-- notes -->" + old.split("<!-- notes -->", 1)[1]
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
