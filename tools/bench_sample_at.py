# -*- coding: utf-8 -*-
"""What draws at new times cost in linear time (csrc/c2_priordraw.hip), on one device, in ONE fresh process:

    python tools/bench_sample_at.py [--steps 20] [--out profiles/sample_at.md] [--quick]
    python tools/bench_sample_at.py --regs-only --out profiles/sample_at.md     # no GPU: refresh the register table

  (a) ops.prior_draw at 8192 and 65536 x N = 4096 x J = 8 with M = 256 and M = 4096 queries and K = 1 and K = 8 draws; beside
      it, in the same process and alternating step by step, ops.factor (the same J x J state) and ops.dot_tril with K
      right-hand sides (the same J x K state).
  (b) gp.sample_at against the existing gp.condition(y, t).sample at 64 and 16 x 4096 x 8 with M = 256 (size 1 and 8);
      sample_at alone at 64 x 4096 x 8 with M = 4096 if the old path cannot allocate there, and at 8192 x 4096 x 8 with
      M = 4096, where the old path would need 268 MB per series.

Every step is timed by its own pair of HIP events after a warm-up, the steps enqueued back to back; the tables give the
median (min .. max) of --steps steps.  Algorithmic bytes per series:

    prior_draw   N (8 + 16 J + 16 K)  t, U, V, nt in; ft out   +  M (8 + 16 J + 16 K)  ts, Us, Vs, ns in; fs out
                 (K <= 8: one block of draws; each further block of 8 reads the rows again: + (N + M) (8 + 16 J))
    factor       N (24 + 24 J)        t, a, U, V in; d, W out
    dot_tril     N (16 + 16 J + 16 K) t, d, U, W, Y in; Z out

as a fraction of the 8 TB/s roofline.  The register table comes from tools/kernel_regs.py (the built object,
celerite2_amd/build)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_sample_at.py --regs-only) -->", "<!-- registers:end -->"
NOT_MEASURED = "# gp.sample_at / ops.prior_draw\n\nNo measurement has been taken: the tables of tools/bench_sample_at.py are not in this file yet.\n"


def register_table():
    """Registers, LDS and scratch of the kernels of c2_priordraw.o, from tools/kernel_regs.py (None if the object is not on
    this machine)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_priordraw.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::priordraw::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_priordraw<lanes per series, draws per register block>`)."
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or "(the built objects are not on this machine: run `python tools/bench_sample_at.py --regs-only --out <this file>` where the library was built)"
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def pd_bytes(N, M, J, K):
    blocks = (K + 7) // 8
    return (N + M) * (8 + 16 * J) * blocks + (N + M) * 16 * K


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
    from celerite2_amd import gp as G, ops, terms as T

    assert torch.cuda.is_available(), "this measures the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")
    kernel = T.SHOTerm(S0=1.0, w0=3.0, Q=2.0) + T.SHOTerm(S0=0.5, w0=1.0, Q=1.5) + T.SHOTerm(S0=0.3, w0=0.3, Q=0.8) \
        + T.SHOTerm(S0=0.2, w0=6.0, Q=4.0)   # J = 8

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

    def series(B, N, seed):
        """Per-series sorted times (mean spacing 0.1), data, and the factored GP."""
        gen = torch.Generator(device=dev).manual_seed(seed)
        x = torch.cumsum(0.02 + 0.16 * torch.rand((B, N), dtype=torch.float64, device=dev, generator=gen), dim=1)
        y = torch.sin(x) + 0.1 * torch.randn((B, N), dtype=torch.float64, device=dev, generator=gen)
        gp = G.GaussianProcess(kernel, x, diag=torch.full((B, N), 0.1, dtype=torch.float64, device=dev))
        return x, y, gp, gen

    def grid(x, M, gen):
        """M sorted query times per series over the span of its data and a little beyond on both sides."""
        lo, hi = x[:, :1] - 1.0, x[:, -1:] + 1.0
        return torch.sort(lo + (hi - lo) * torch.rand((x.shape[0], M), dtype=torch.float64, device=dev, generator=gen), dim=1).values

    randn = lambda gen, *s: torch.randn(s, dtype=torch.float64, device=dev, generator=gen)

    # (a) the op beside factor and dot_tril
    N = 4096 if not a.quick else 512
    lines = ["# ops.prior_draw beside factor and dot_tril", "",
             "One process, steps alternating between the ops, %d timed steps each after %d warm-up steps; ms: median (min .. max)."
             % (a.steps, a.warmup), "",
             "| B x N x J | M | K | op | ms | algorithmic bytes per series | GB/s | of the 8 TB/s roofline | time / (factor + dot_tril) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for B in ((8192, 65536) if not a.quick else (256,)):
        x, y, gp, gen = series(B, N, 7)
        J = gp._U.shape[-1]
        d, W = torch.empty_like(gp._d), torch.empty_like(gp._W)
        for M in ((256, 4096) if not a.quick else (64, 512)):
            ts = grid(x, M, gen)
            _, _, Us, Vs = kernel.get_celerite_matrices(ts, torch.zeros_like(ts))
            for K in (1, 8):
                nt, ns = randn(gen, B, N, K), randn(gen, B, M, K)
                ft, fs, Z = torch.empty_like(nt), torch.empty_like(ns), torch.empty_like(nt)
                runs = {"factor": lambda: ops.factor(gp._t, gp._c, gp._a, gp._U, gp._V, d=d, W=W),
                        "dot_tril": lambda: ops.dot_tril(gp._t, gp._c, gp._U, gp._W, gp._d, nt, Z=Z),
                        "prior_draw": lambda: ops.prior_draw(gp._t, ts, gp._c, gp._U, gp._V, Us, Vs, nt, ns, ft=ft, fs=fs)}
                res = alternate(runs, a.steps)
                both = res["factor"][0] + res["dot_tril"][0]
                for op, st in res.items():
                    nb = {"factor": N * (24 + 24 * J), "dot_tril": N * (16 + 16 * J + 16 * K), "prior_draw": pd_bytes(N, M, J, K)}[op]
                    rate = nb * B / (st[0] * 1e-3)
                    lines.append("| %d x %d x %d | %d | %d | %s | %.3f (%.3f .. %.3f) | %d | %.0f | %.1f %% | %.2f |"
                                 % (B, N, J, M, K, op, st[0], st[1], st[2], nb, rate / 1e9, 100 * rate / PEAK, st[0] / both))
                    print(lines[-1], flush=True)
                del nt, ns, ft, fs, Z, runs
            del ts, Us, Vs
        del x, y, gp, d, W
        torch.cuda.empty_cache()

    # (b) the frontend against the existing path through the M x M conditional covariance and its dense Cholesky factor
    lines += ["", "# gp.sample_at against gp.condition(y, t).sample", "",
              "| B x N x J | M | size | sample_at: ms per call | condition(y, t).sample: ms per call | old / new |",
              "|---|---|---|---|---|---|"]
    shapes = ((64, 256, 1), (64, 256, 8), (16, 256, 1), (16, 256, 8), (64, 4096, 8)) if not a.quick else ((4, 64, 1), (4, 64, 8))
    for B, M, size in shapes:
        x, y, gp, gen = series(B, N, 11)
        ts = grid(x, M, gen)
        runs = {"new": lambda: gp.sample_at(y, ts, size=size, generator=gen, check_sorted=False)}
        old = "not run"
        try:
            gp.condition(y, ts).sample(size=size, generator=gen)
            runs["old"] = lambda: gp.condition(y, ts).sample(size=size, generator=gen)
        except torch.OutOfMemoryError:
            old = "cannot allocate (%.1f GB of N x M and M x M arrays)" % (8.0 * B * (N * M + M * M) / 1e9)
            torch.cuda.empty_cache()
        except RuntimeError as exc:   # (a covariance that is not positive definite in floating point has no Cholesky factor)
            old = "fails: %s" % str(exc).split("\n")[0][:80]
        res = alternate(runs, max(5, a.steps // 4))
        if "old" in res:
            lines.append("| %d x %d x %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f |"
                         % ((B, N, gp._U.shape[-1], M, size) + res["new"] + res["old"] + (res["old"][0] / res["new"][0],)))
        else:
            lines.append("| %d x %d x %d | %d | %d | %.3f (%.3f .. %.3f) | %s | |" % ((B, N, gp._U.shape[-1], M, size) + res["new"] + (old,)))
        print(lines[-1], flush=True)
        del x, y, gp, ts, runs
        torch.cuda.empty_cache()
    if not a.quick:
        B, M, size = 8192, 4096, 1
        x, y, gp, gen = series(B, N, 13)
        ts = grid(x, M, gen)
        st = alternate({"big": lambda: gp.sample_at(y, ts, size=size, generator=gen, check_sorted=False)}, max(3, a.steps // 4))["big"]
        lines += ["", "gp.sample_at at %d x %d x %d with M = %d, one draw, completes: %.2f ms (%.2f .. %.2f) per call (the normals, the queries' "
                  "U and V rows, prior_draw, the two solves and the two general products); the old path would need %.0f GB of "
                  "cross- and conditional covariance there." % ((B, N, gp._U.shape[-1], M) + st + (8.0 * B * (N * M + M * M) / 1e9,))]
        print(lines[-1], flush=True)
    text = with_registers("\n".join(lines) + "\n")
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
