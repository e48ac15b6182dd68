# -*- coding: utf-8 -*-
"""What the log-likelihood and gradient of a RAGGED batch cost (celerite2_amd/packed.py, csrc/c2_packed.hip), on one device, in
ONE fresh process:

    python tools/bench_packed.py [--steps 7] [--out profiles/packed.md] [--quick]
    python tools/bench_packed.py --regs-only --out profiles/packed.md      # no GPU: the register table

Shapes: J in {2, 8}, B in {8192, 65536} where memory allows, the lengths all 4096 or drawn uniformly from 256 .. 4096 with a
fixed seed.  Routes, alternating step by step in the same process, every step timed by its own pair of HIP events after a
warm-up, the table giving the median (min .. max) of --steps steps:

  (a) packed.loglik_grad on caller-owned work and out: with the default order, with the series in descending length
      (pk.order), in descending length inside windows of 1024 neighbours (sorted, but neighbours in memory) and as stored;
  (b) the exact route there was before: ops.filter_init -> ops.filter_append with `count` on arrays padded to N_max ->
      ops.filter_append_rev with the cotangent -1/2 on the two sums of the state;
  (c) ops.loglik_grad on the rectangle -- the tuned yardstick at equal lengths, the time of the WRONG answer (the padding
      rows enter the likelihood) at ragged ones.

Conditions set in advance: the median of (a) is not above the median of (b) at any measured shape, and (a)'s workspace is
below (b)'s ws.  Recorded without a bar: (a) / (c), the achieved bytes per second of (a) against the 8 TB/s roofline (bytes
counted from the shapes: what the two kernels must move, the ring of replayed states not included), what `order` buys.  A
route that cannot allocate is written down as that."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8.0e12   # bytes / s
REG_BEGIN, REG_END = "<!-- registers:begin (tools/bench_packed.py --regs-only) -->", "<!-- registers:end -->"
TITLE = "# packed.loglik_grad beside the padded routes"
NOT_MEASURED = TITLE + "\n\nNot measured yet: run `python tools/bench_packed.py --out profiles/packed.md` on an MI355X.\n"


def register_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    rows = kernel_rows("c2_packed.o")
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        name = re.sub(r"\(.*", "", name).replace("void ", "").replace("c2::packed::", "")
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (name, vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, most spilled registers %d over %d kernels (`k_packed_fwd<lanes per series, records and "
              "checkpoints>`, `k_packed_rev<lanes per series>`)." % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows))]
    return "\n".join(lines)


def with_registers(text):
    table = register_table() or ("(the built objects are not on this machine: run `python tools/bench_packed.py --regs-only "
                                 "--out <this file>` where the library was built)")
    block = REG_BEGIN + "\n" + table + "\n" + REG_END
    if REG_BEGIN in text and REG_END in text:
        head, rest = text.split(REG_BEGIN, 1)
        return head + block + rest.split(REG_END, 1)[1]
    return text + "\n## Registers (gfx950, from the built object)\n\n" + block + "\n"


def packed_bytes(R, J):
    """What the two kernels of packed.loglik_grad must move, per call: forward t, a, y, U, V in and d, z, W out; replay t, d, z,
    W in; backward t, d, z, U, W in and bt, ba, by, bU, bV out.  (Checkpoints: 1 / C of a row's J^2 + J, left out with the ring.)"""
    return 8 * R * ((3 + 2 * J) + (J + 2) + (J + 3) + (2 * J + 3) + (2 * J + 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes only (a rehearsal of the script, not a measurement)")
    ap.add_argument("--regs-only", action="store_true")
    args = ap.parse_args()
    if args.regs_only:
        text = open(args.out).read() if args.out and os.path.exists(args.out) else NOT_MEASURED
        text = with_registers(text)
        if args.out:
            open(args.out, "w").write(text)
        else:
            print(text)
        return
    if args.steps < 5:
        ap.error("--steps: at least 5 (the medians are of that many alternating steps)")

    import numpy as np
    import torch

    from celerite2_amd import ops, packed

    dev = torch.device("cuda")
    f64 = dict(dtype=torch.float64, device=dev)

    def inputs(B, lengths, J):
        """A positive-definite ragged batch made on the device: J / 2 complex terms with b = 0 per series (exp(-c tau) cos(d tau)
        is a covariance), a white diagonal of 0.1 .. 0.3, times with gaps of 0.01 .. 0.21."""
        g = torch.Generator(device=dev).manual_seed(1234)
        R = int(lengths.sum())
        gaps = 0.01 + 0.2 * torch.rand(R, generator=g, **f64)
        t = torch.cumsum(gaps, 0)
        pk0 = packed.Packed(t, lengths, check_sorted=False)
        start = torch.zeros(B, **f64)
        nz = torch.from_numpy(lengths > 0).to(dev)
        start[nz] = t[pk0.offsets[:-1][nz]]
        t = (t - start[pk0.seg]).contiguous()
        del gaps, start
        pk = packed.Packed(t, lengths)
        Jc = J // 2
        u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, Jc, generator=g, **f64)
        e = torch.zeros(B, 0, **f64)
        coefs = (e, e, u(0.3, 1.0), torch.zeros(B, Jc, **f64), u(0.05, 1.0), u(0.5, 3.0))
        diag = 0.1 + 0.2 * torch.rand(R, generator=g, **f64)
        a, U, V = torch.empty(R, **f64), torch.empty(R, J, **f64), torch.empty(R, J, **f64)
        off = pk.offsets.tolist()
        for b0, b1 in slabs(B):   # (in slabs of series: no torch kernel sees 2^31 elements)
            r0, r1 = off[b0], off[b1]
            sub = packed.Packed(t[r0:r1], lengths[b0:b1], check_sorted=False)
            cs, a[r0:r1], U[r0:r1], V[r0:r1] = packed.celerite_rows([v[b0:b1] for v in coefs], sub, diag[r0:r1])
        c = torch.cat([coefs[1], coefs[4].repeat_interleave(2, dim=1)], dim=1).contiguous()
        y = torch.sin(t) + 0.1 * torch.randn(R, generator=g, **f64)
        return pk, [c, a, U, V, y]

    def slabs(B, n=4096):
        return [(b0, min(b0 + n, B)) for b0 in range(0, B, n)]

    def padded(pk, x, fill=0.0):
        """pk.to_padded in slabs of series."""
        out = torch.empty((pk.B, pk.n_max) + tuple(x.shape[1:]), **f64)
        off = pk.offsets.tolist()
        for b0, b1 in slabs(pk.B):
            r0, r1 = off[b0], off[b1]
            sub = packed.Packed(pk.t[r0:r1], pk.lengths[b0:b1], check_sorted=False)
            part = sub.to_padded(x[r0:r1], fill)
            out[b0:b1, :part.shape[1]] = part
            if part.shape[1] < pk.n_max:
                out[b0:b1, part.shape[1]:] = fill
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def stats(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2], xs[0], xs[-1]

    def fmt(s):
        return "—" if s is None else (s if isinstance(s, str) else "%.2f (%.2f .. %.2f)" % s)

    shapes = [(J, B, kind) for J in (2, 8) for B in (8192, 65536) for kind in ("equal", "ragged")]
    nlo, nhi = 256, 4096
    if args.quick:
        shapes, nlo, nhi = [(J, 256, kind) for J in (2, 8) for kind in ("equal", "ragged")], 16, 256
    rows, verdict = [], []
    for J, B, kind in shapes:
        lengths = np.full(B, nhi, dtype=np.int64) if kind == "equal" else np.random.default_rng(7).integers(nlo, nhi + 1, B)
        routes, notes, made = {}, [], {}
        try:
            pk, (c, a, U, V, y) = inputs(B, lengths, J)
        except RuntimeError as err:
            rows.append((J, B, kind, 0, None, None, None, None, "the inputs cannot be allocated (%s)" % str(err).split("\n")[0][:60], 0, 0))
            torch.cuda.empty_cache()
            continue
        R, N = pk.R, pk.n_max
        work_a = packed.workspace(pk, J)
        out_a = tuple(torch.empty(s, **f64) for s in ((R,), (B, J), (R,), (R, J), (R, J), (R,)))
        routes["a"] = lambda: packed.loglik_grad(pk, c, a, U, V, y, work=work_a, out=out_a)   # the default order
        routes["a_sorted"] = lambda: packed.loglik_grad(pk, c, a, U, V, y, work=work_a, out=out_a, order="sorted")
        routes["a_plain"] = lambda: packed.loglik_grad(pk, c, a, U, V, y, work=work_a, out=out_a, order=None)
        idx = np.arange(B)   # (a negative result kept reproducible: by length inside windows of 1024 neighbours)
        windowed = torch.from_numpy(np.lexsort((idx, -lengths, idx // 1024)).astype(np.int32)).to(dev)
        routes["a_window"] = lambda: packed.loglik_grad(pk, c, a, U, V, y, work=work_a, out=out_a, order=windowed)
        ll_a, _, flag_a = routes["a"]()
        assert not bool(flag_a.any()), "the draw is not positive definite"
        ws_b = 8 * B * N * (J + J * J)
        try:   # the padded rectangle of (b) and (c)
            tp = padded(pk, pk.t, 1.0e9); ap_ = padded(pk, a, 1.0); yp = padded(pk, y)
            Up = padded(pk, U); Vp = padded(pk, V)
            made["pad"] = True
        except RuntimeError:
            notes.append("the padded arrays cannot be allocated")
            torch.cuda.empty_cache()
        if made.get("pad"):
            try:
                count = torch.from_numpy(lengths.astype(np.int32)).to(dev)
                st0 = ops.filter_init(B, J, dev)
                bst = torch.zeros_like(st0); bst[:, 2] = -0.5; bst[:, 3] = -0.5
                ws = torch.empty((B, N, J + J * J), **f64)
                st1 = torch.empty_like(st0)
                d_, W_, z_ = torch.empty_like(ap_), torch.empty_like(Up), torch.empty_like(ap_)
                out_b = tuple(torch.empty(s, **f64) for s in ((B, 4 + J + J * J), (B, N), (B, J), (B, N), (B, N, J), (B, N, J), (B, N)))

                def route_b():
                    _, d, W, z, flag = ops.filter_append(st0, tp, c, ap_, Up, Vp, yp, count=count, out=st1, d=d_, W=W_, z=z_)
                    ops.filter_append_rev(st0, tp, c, Up, W, d, z, flag, bst, count=count, ws=ws, out=out_b)

                route_b()
                torch.cuda.synchronize()
                ll_b = -0.5 * (st1[:, 2] + st1[:, 3] + st1[:, 1] * 1.8378770664093453)
                assert torch.allclose(ll_b, ll_a, rtol=1e-9, atol=1e-6), "routes (a) and (b) disagree"
                routes["b"] = route_b
            except RuntimeError as err:
                notes.append("(b) cannot allocate its %.1f GB of ws beside its arrays" % (ws_b / 1e9))
                ws = d_ = W_ = z_ = out_b = None
                torch.cuda.empty_cache()
            if "b" not in routes:
                ws = d_ = W_ = z_ = out_b = None
                torch.cuda.empty_cache()
            try:
                work_c = ops.loglik_grad_workspace(B, N, J, dev)
                out_c = tuple(torch.empty(s, **f64) for s in ((B, N), (B, J), (B, N), (B, N, J), (B, N, J), (B, N)))
                routes["c"] = lambda: ops.loglik_grad(tp, c, ap_, Up, Vp, yp, work=work_c, out=out_c)
                routes["c"]()
                torch.cuda.synchronize()
            except RuntimeError:
                notes.append("(c) cannot allocate its workspace")
                routes.pop("c", None)
                work_c = out_c = None
                torch.cuda.empty_cache()
        times = {k: [] for k in routes}
        for step in range(args.warmup + args.steps):
            for k, fn in routes.items():
                ms = timed(fn)
                if step >= args.warmup:
                    times[k].append(ms)
        st = {k: stats(v) for k, v in times.items()}
        nbytes = packed_bytes(R, J)
        rows.append((J, B, kind, R, (st["a"], st["a_sorted"], st["a_window"]), st.get("a_plain"), st.get("b"), st.get("c"), "; ".join(notes),
                     work_a.numel() * 8, ws_b, nbytes))
        if "b" in st:
            ok = st["a"][0] <= st["b"][0] and work_a.numel() * 8 < ws_b
            verdict.append((J, B, kind, ok))
        print(rows[-1], flush=True)
        del routes, work_a, out_a, pk, c, a, U, V, y
        tp = ap_ = yp = Up = Vp = ws = d_ = W_ = z_ = out_b = work_c = out_c = st0 = st1 = bst = None
        torch.cuda.empty_cache()

    L = [TITLE, "", "`python tools/bench_packed.py --steps %d%s` on %s, torch %s.  Milliseconds per call, median (min .. max) of %d "
         "alternating steps after %d warm-up steps, each step between its own pair of HIP events.  Lengths: all %d, or uniform in "
         "%d .. %d (seed 7).  (a) packed.loglik_grad; (b) filter_append with `count` + filter_append_rev on arrays padded to N_max; "
         "(c) ops.loglik_grad on the padded rectangle (at ragged lengths: the time of the wrong answer)."
         % (args.steps, " --quick" if args.quick else "", torch.cuda.get_device_name(0), torch.__version__, args.steps, args.warmup,
            nhi, nlo, nhi), "",
         "| J | B | lengths | rows R | (a) default order | (a) sorted | (a) sorted in windows of 1024 | (a) no order | (b) append + reverse | "
         "(c) rectangle | (a) / (b) | (a) / (c) | (a) of 8 TB/s | work of (a) | ws of (b) | notes |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r[4] is None:
            L.append("| %d | %d | %s | — | — | — | — | — | — | — | — | — | — | — | — | %s |" % (r[0], r[1], r[2], r[8]))
            continue
        J, B, kind, R, (sa, ss, sw), sp, sb, sc, note, wa, wb, nb = r
        ratio = lambda x: "—" if x is None else "%.2f" % (sa[0] / x[0])
        L.append("| %d | %d | %s | %d | %s | %s | %s | %s | %s | %s | %s | %s | %.1f %% | %.2f GB | %.2f GB | %s |"
                 % (J, B, kind, R, fmt(sa), fmt(ss), fmt(sw), fmt(sp), fmt(sb), fmt(sc), ratio(sb), ratio(sc), 100.0 * nb / (sa[0] * 1e-3) / PEAK,
                    wa / 1e9, wb / 1e9, note))
    L += ["", "Conditions set in advance -- median of (a) not above the median of (b), work of (a) below the ws of (b) -- at the "
          "shapes where (b) ran: " + (", ".join("%d x %d %s: %s" % (J, B, k, "met" if ok else "MISSED") for J, B, k, ok in verdict)
                                     or "none ran") + "."]
    text = with_registers("\n".join(L) + "\n")
    if args.out:
        open(args.out, "w").write(text)
    print(text)
    if not all(ok for *_, ok in verdict):
        sys.exit(1)


if __name__ == "__main__":
    main()
