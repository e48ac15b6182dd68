# -*- coding: utf-8 -*-
"""What the term algebra costs (csrc/c2_term_expr.hip), on one device, in ONE fresh process:

    python tools/term_algebra_time.py [--B 65536] [--N 4096] [--steps 20] [--out profiles/term_algebra.md]

  (a) the two coefficient kernels alone (ops.term_coefficients / term_coefficients_rev on an ops.TermExpr) at B series for
      three expressions: sho * sho2 (width 4), (sho * real) * sho2 + real (width 5), TermConvolution(sho * real + mat, delta)
      (width 4) -- next to the flat kernels on the width-4 SUM sho + sho2 (ops.TermProgram);
  (b) ops.loglik_kernel_grad at B x N for the width-4 PRODUCT sho * sho2 (the expression chain: coefficients -> shift apply ->
      likelihood -> shift reverse -> coefficients reverse) against the width-4 SUM sho + sho2 on the flat program's chain --
      the path that existed before the algebra -- alternating step by step in the same process, caller-owned buffers.
Every step is timed by its own pair of HIP events after a warm-up; the table gives median, min and max, the ratio of the
medians, and the run-to-run spread (max - min) / median of the flat path the ratio is to be read against."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from celerite2_amd import ops, terms as T

    B, N = a.B, a.N
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    u = lambda lo, hi, *sh: lo + (hi - lo) * torch.rand(sh, dtype=torch.float64, device=dev, generator=gen)

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(ms):
        ms = sorted(ms)
        return ms[len(ms) // 2], ms[0], ms[-1]

    sho = lambda: T.SHOTerm(S0=u(0.2, 1.0, B), w0=u(0.3, 1.0, B), Q=u(1.0, 8.0, B), regime="under")
    sho2 = lambda: T.SHOTerm(sigma=u(0.5, 1.5, B), rho=u(2.0, 4.0, B), Q=u(1.0, 4.0, B), regime="under")
    real = lambda: T.RealTerm(a=u(0.5, 1.5, B), c=u(0.05, 0.4, B))
    mat = lambda: T.Matern32Term(sigma=u(0.3, 1.0, B), rho=u(1.0, 4.0, B))
    kernels = {"sum sho + sho2 (flat program)": sho() + sho2(), "prod_sho_sho: sho * sho2": sho() * sho2(),
               "nested: (sho * real) * sho2 + real": (sho() * real()) * sho2() + real(),
               "conv_prod: TermConvolution(sho * real + mat, 0.02)": T.TermConvolution(sho() * real() + mat(), 0.02)}
    lines = ["## (a) the coefficient kernels alone, B = %d, %d timed steps each after %d warm-up steps" % (B, a.steps, a.warmup), "",
             "| kernel | width | registers (real, complex) | forward ms: median (min .. max) | reverse ms: median (min .. max) |",
             "|---|---|---|---|---|"]
    for name, k in kernels.items():
        prog, P = k.program, k.parameter_matrix(B).contiguous()
        is_expr = isinstance(prog, ops.TermExpr)
        work = prog.workspace(B, dev) if is_expr else None
        kw = dict(work=work) if is_expr else {}
        res = ops.term_coefficients(prog, P, B, **kw)
        coefs, flag = res[0], res[1]
        assert int(flag.abs().sum()) == 0
        cots = [torch.ones_like(c) for c in coefs]
        bP = torch.empty((B, prog.NP), dtype=torch.float64, device=dev)
        if is_expr:
            kw_r = dict(work=work, bshift=torch.ones(B, dtype=torch.float64, device=dev))
            fkw = dict(work=work, shift=res[2])
        else:
            kw_r, fkw = {}, {}
        fwd = lambda: ops.term_coefficients(prog, P, B, out=list(coefs), flag=flag, **fkw)
        rev = lambda: ops.term_coefficients_rev(prog, P, cots, out=bP, **kw_r)
        for _ in range(a.warmup):
            fwd(); rev()
        tf = stats([one(fwd) for _ in range(a.steps)])
        tr = stats([one(rev) for _ in range(a.steps)])
        regs = "(%d, %d)" % (prog._c.NR, prog._c.NC) if is_expr else "(%d, %d) in place" % (prog.Jr, prog.Jc)
        lines.append("| %s | %d | %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) |" % ((name, prog.width, regs) + tf + tr))
        print(lines[-1], flush=True)

    # (b) the whole chain, product (expression) against sum (flat program), alternating
    x = torch.cumsum(u(0.02, 0.18, B, N), dim=1)
    yerr = torch.sqrt(u(0.1, 0.3, B, N))
    y = torch.sin(x) + 0.1 * torch.randn((B, N), dtype=torch.float64, device=dev, generator=gen)
    jitter, mean = u(0.05, 0.3, B), u(-0.2, 0.2, B)
    runs = {}
    for tag, name in (("sum", "sum sho + sho2 (flat program)"), ("product", "prod_sho_sho: sho * sho2")):
        k = kernels[name]
        prog, P = k.program, k.parameter_matrix(B).contiguous()
        work = ops.loglik_kernel_workspace(prog, B, N, dev)
        ll, out, flag = ops.loglik_kernel_grad(prog, P, x, yerr, jitter, mean, y, work=work)
        assert int(flag.abs().sum()) == 0, tag
        runs[tag] = (lambda prog=prog, P=P, work=work, out=out: ops.loglik_kernel_grad(prog, P, x, yerr, jitter, mean, y, work=work, out=out))
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    ms = {tag: [] for tag in runs}
    for _ in range(a.steps):          # alternating: sum, product, sum, product, ...
        for tag, fn in runs.items():
            ms[tag].append(one(fn))
    s, p = stats(ms["sum"]), stats(ms["product"])
    lines += ["", "## (b) ops.loglik_kernel_grad, %d x %d, width 4: product (expression chain) against sum (flat chain), alternating, "
              "%d timed steps each" % (B, N, a.steps), "",
              "| path | ms per step: median (min .. max) |", "|---|---|",
              "| sum sho + sho2: noise_mean_apply -> term_coefficients -> loglik_terms_grad -> term_coefficients_rev / noise_mean_rev | %.3f (%.3f .. %.3f) |" % s,
              "| product sho * sho2: term_expr_coefficients -> noise_mean_shift_apply -> loglik_terms_grad -> noise_mean_shift_rev -> term_expr_coefficients_rev | %.3f (%.3f .. %.3f) |" % p,
              "", "ratio of the medians product / sum: %.4f; run-to-run spread of the sum path (max - min) / median: %.4f"
              % (p[0] / s[0], (s[2] - s[1]) / s[0])]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
