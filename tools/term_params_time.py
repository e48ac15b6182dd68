# -*- coding: utf-8 -*-
"""What the hyper-parameter layer costs on top of the coefficient-level gradient, at the bench shape: four SHO terms
(regime="under", width 8), per-series S0, w0, Q, jitter and mean, B series x 4096 points.

    python tools/term_params_time.py [--sizes 8192,16384,32768,65536] [--steps 20] [--reps 2] [--parent-lib PATH] [--out FILE]

For every size, in a FRESH process each and alternating (process-to-process spread is part of the answer):
  (a)  ops.loglik_terms_grad alone, on precomputed coefficients, diag and residuals -- with this build's library and, when
       --parent-lib names a build of the parent commit's libcelerite2_amd.so, with that one too (C2_LIB_PATH);
  (b)  the full ops.loglik_kernel_grad: noise_mean_apply -> term_coefficients -> loglik_terms_grad ->
       term_coefficients_rev / noise_mean_rev;
  added the four kernels of this layer alone, on the same buffers (in the process of (b));
  copy a plain device copy moving the bytes the two (B, N) passes move (4 + 2 arrays: 3 arrays copied = 3 read + 3 written).
Times are HIP events over `--steps` steps after a warm-up; caller-owned buffers throughout.  Prints a markdown table
(and writes it to --out).  A child is `--child MODE B`; it prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def child(mode, B, steps):
    import torch

    sys.path.insert(0, ROOT)
    from celerite2_amd import ops

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1234)
    u = lambda lo, hi, *sh: lo + (hi - lo) * torch.rand(sh, dtype=torch.float64, device=dev, generator=gen)
    x = torch.cumsum(u(0.02, 0.18, B, N), dim=1)
    yerr = torch.sqrt(u(0.1, 0.3, B, N))
    y = torch.sin(x) + 0.1 * torch.randn((B, N), dtype=torch.float64, device=dev, generator=gen)
    jitter, mean = u(0.05, 0.3, B), u(-0.2, 0.2, B)
    cols = []
    for k in range(4):
        cols += [u(0.2, 1.0, B), u(0.3 + 0.8 * k, 1.0 + 0.8 * k, B), u(1.0, 8.0, B)]
    P = torch.stack(cols, dim=1).contiguous()

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    row = {"mode": mode, "B": B, "lib": os.environ.get("C2_LIB_PATH", "this build")}
    if mode == "a":
        # coefficients by torch (set-up, untimed; the same numbers for either library): terms.py:658-691, Q > 1/2
        S0, w0, Q = P[:, 0::3], P[:, 1::3], P[:, 2::3]
        f = torch.sqrt(4 * Q * Q - 1)
        ac, cc = S0 * w0 * Q, 0.5 * w0 / Q
        coefs = [torch.zeros((B, 0), dtype=torch.float64, device=dev)] * 2 + [v.contiguous() for v in (ac, ac / f, cc, cc * f)]
        diag, r = (yerr**2 + jitter[:, None] ** 2).contiguous(), (y - mean[:, None]).contiguous()
        del yerr, y
        work = ops.loglik_terms_workspace(B, N, 0, 4, dev)
        ll, out, flag = ops.loglik_terms_grad(*coefs, x, diag, r, work=work)
        assert int(flag.abs().sum()) == 0
        row["ms"] = timed(lambda: ops.loglik_terms_grad(*coefs, x, diag, r, work=work, out=out))
    elif mode == "b":
        prog = ops.TermProgram([dict(kind="sho", cols=(3 * k, 3 * k + 1, 3 * k + 2), regime="under") for k in range(4)], 12)
        work = ops.loglik_kernel_workspace(prog, B, N, dev)
        ll, out, flag = ops.loglik_kernel_grad(prog, P, x, yerr, jitter, mean, y, work=work)
        assert int(flag.abs().sum()) == 0
        row["ms"] = timed(lambda: ops.loglik_kernel_grad(prog, P, x, yerr, jitter, mean, y, work=work, out=out))

        def added():   # the four kernels this layer adds, on the same buffers, without the likelihood between them
            ops.noise_mean_apply(yerr, jitter, mean, y, out=(work["diag"], work["r"]))
            ops.term_coefficients(prog, P, B, out=work["coefs"], flag=work["tflag"])
            ops.term_coefficients_rev(prog, P, work["cots"], tflag=work["tflag"], lflag=flag, out=out[0])
            ops.noise_mean_rev(jitter, out[4], out[5], flag=flag, out=(out[1], out[2]))

        row["added_ms"] = timed(added)
    else:
        src, dst = torch.stack([x, yerr, y]), torch.empty((3, B, N), dtype=torch.float64, device=dev)
        row["ms"] = timed(lambda: dst.copy_(src))
        row["GB"] = 6 * B * N * 8 / 1e9
    row["ll_sum"] = float(ll.sum()) if mode != "copy" else None
    print(json.dumps(row), flush=True)


def run_child(mode, B, steps, lib=None):
    env = dict(os.environ)
    env.pop("C2_LIB_PATH", None)
    if lib:
        env["C2_LIB_PATH"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, str(B), "--steps", str(steps)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:   # stop here: nothing more is started on the device after a failed child
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit("child %s B=%d failed with status %d" % (mode, B, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,16384,32768,65536")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.steps)
    lines = ["| series | (a) parent ms | (a) this build ms | (b) full ms | (b) - (a) ms | the four added kernels alone ms | copy of the same bytes ms (GB) | ll sums agree |",
             "|---|---|---|---|---|---|---|---|"]
    fmt = lambda v: " / ".join("%.3f" % x for x in v) if v else "not measured"
    for B in [int(s) for s in a.sizes.split(",")]:
        ap_, at, b, ad, cp, sums = [], [], [], [], [], set()
        for _ in range(a.reps):   # alternating: parent, this build, full, copy
            if a.parent_lib:
                r = run_child("a", B, a.steps, a.parent_lib); ap_.append(r["ms"]); sums.add(r["ll_sum"])
            r = run_child("a", B, a.steps); at.append(r["ms"]); sums.add(r["ll_sum"])
            r = run_child("b", B, a.steps); b.append(r["ms"]); ad.append(r["added_ms"]); llb = r["ll_sum"]
            r = run_child("copy", B, a.steps); cp.append(r["ms"]); gb = r["GB"]
        s0 = sorted(sums)[0]
        agree = "(a): %s; (b) vs (a): %.1e rel" % ("identical" if len(sums) == 1 else "DIFFER", abs(llb - s0) / abs(s0))
        lines.append("| %d | %s | %s | %s | %.3f | %s | %s (%.1f) | %s |" % (B, fmt(ap_), fmt(at), fmt(b), min(b) - min(at), fmt(ad), fmt(cp), gb, agree))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
