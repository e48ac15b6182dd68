# -*- coding: utf-8 -*-
"""The static tables of the one-lane-per-trial sweep (trial::k_trial_sweep<Column, JR, QR>, csrc/c2_trial_sweep.hpp, instantiated
by csrc/c2_periodogram.hip, c2_transit.hip, c2_kepler.hip and c2_shapes.hip), shared by tools/bench_periodogram.py,
tools/bench_transit.py, tools/bench_kepler.py and tools/bench_shapes.py: the register table from the built objects, the row
loop's instruction mix from the compiler's assembly, and the marked blocks of a profile that hold them.  No GPU."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TITLES = {"registers": "Registers (gfx950, from the built objects)", "instructions": "The row loop (gfx950, from the compiler's assembly)"}


# search -> (the source that instantiates the sweep for it, its column source of csrc/c2_trial_columns.hpp)
SWEEPS = {"periodogram": ("c2_periodogram", "Sinusoid"), "transit": ("c2_transit", "Transit"), "keplerian": ("c2_kepler", "Keplerian"),
          "shape": ("c2_shapes", "Shape")}


def sweep_label(search, jr, qr):
    return "k_trial_sweep<%s, %d, %d>" % (SWEEPS[search][1], jr, qr)


def sweep_symbol(search, jr, qr):
    """The mangled name of c2::trial::k_trial_sweep<c2::trial::<Column>, jr, qr>, up to its arguments."""
    column = SWEEPS[search][1]
    return "_ZN2c25trial13k_trial_sweepINS0_%d%sELi%dELi%dEE" % (len(column), column, jr, qr)


def sweep_asm(search):
    return kernel_asm(SWEEPS[search][0] + ".hip")


def sweep_registers(search, note=""):
    return register_table(SWEEPS[search][0] + ".o", " (`k_trial_sweep<Column, JR, QR>`: J rounded up to 4, 8, 16 or 32, Q0 to 1, 2, 4 or 8)." + note)


def marks(key, tool):
    return "<!-- %s:begin (%s) -->" % (key, tool), "<!-- %s:end -->" % key


def with_block(text, key, table, tool):
    """`text` with the block `key` replaced by (or, with its title, appended as) `table`; `tool`: the command that makes it."""
    begin, end = marks(key, tool)
    table = table or "(neither the built objects nor the compiler are on this machine: run `python %s --out <this file>` where the library was built)" % tool
    block = begin + "\n" + table + "\n" + end
    if begin in text and end in text:
        head, rest = text.split(begin, 1)
        return head + block + rest.split(end, 1)[1]
    return text + "\n## %s\n\n" % TITLES[key] + block + "\n"


def kept_block(text, key, tool):
    begin, end = marks(key, tool)
    return text.split(begin, 1)[1].split(end, 1)[0].strip("\n") if begin in text and end in text else None


def sorted_rows(obj, kernel=""):
    """kernel_regs.kernel_rows of the built object `obj` whose name holds `kernel`, by their last two template arguments."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_regs import kernel_rows

    return sorted((r for r in kernel_rows(obj) if kernel in r[1]), key=lambda r: [int(v) for v in re.findall(r"\d+", re.sub(r"\(.*", "", r[1]))[-2:]])


def short_name(name):
    """A demangled kernel name without its arguments, `void` and the project's namespaces."""
    return re.sub(r"c2::\w+::", "", re.sub(r"\(.*", "", name).replace("void ", ""))


def register_table(obj, note=".", kernel=""):
    """The registers, LDS and scratch of every kernel of the built object `obj`, e.g. "c2_trial_project.o", whose name holds
    `kernel`; None where the objects are not on this machine."""
    rows = sorted_rows(obj, kernel)
    if not rows:
        return None
    lines = ["| kernel | registers (of them accumulation) | SGPRs | LDS bytes | scratch bytes | spilled registers |", "|---|---|---|---|---|---|"]
    for _, name, vg, ag, scratch, lds, spill, sg in rows:
        lines.append("| `%s` | %d (%d) | %d | %d | %d | %d |" % (short_name(name), vg, ag, sg, lds, scratch, spill))
    lines += ["", "Largest scratch %d bytes, %d spilled registers over %d kernels%s"
              % (max(r[4] for r in rows), max(r[6] for r in rows), len(rows), note)]
    return "\n".join(lines)


def kernel_asm(source):
    """The gfx950 assembly of csrc/`source` from a device-only compile with the build's own flags; None without the compiler."""
    from celerite2_amd import build

    if not os.path.exists(build.HIPCC):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, source[:-4] + ".s")
        flags = [f for f in build.HIPFLAGS if f not in ("-shared", "-fPIC")]
        subprocess.run([build.HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, source), "-o", out], check=True)
        return open(out).read()


def row_loop_mix(asm, name, skip=None):
    """(Counter of the instructions one row of one lane issues in the kernel with the mangled name `name`, Counter of what is
    left out): the innermost loop with an LDS read in the compiler's assembly.  Left out, with `skip` a mnemonic: the
    regions inside the loop that a forward conditional branch jumps over and that hold `skip` -- code a wavefront enters only
    when a lane needs it."""
    i = asm.index("\n" + name) + 1
    lines = asm[i:asm.index(".Lfunc_end", i)].split("\n")
    labels = {m.group(1): k for k, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l.strip())] if m}
    loops = []
    for k, l in enumerate(lines):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), k) < k:
            loops.append((labels[m.group(1)], k))
    a = max(lp[0] for lp in loops if any("ds_read" in l for l in lines[lp[0]:lp[1]]))   # the innermost header ...
    b = max(lp[1] for lp in loops if lp[0] == a)                                        # ... and its last back edge
    out = set()
    for k in range(a, b + 1) if skip else ():
        m = re.search(r"s_cbranch_(?:execz|scc[01]|vccn?z)\s+(\.LBB\d+_\d+)", lines[k])
        if m and k < labels[m.group(1)] <= b and any(skip in l for l in lines[k:labels[m.group(1)]]):
            out.update(range(k + 1, labels[m.group(1)]))
        # (the compiler may rotate the loop instead: the row's body first, a conditional branch back to the body when no
        # lane needs the region, and the region falling through to an unconditional branch back)
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", lines[k])
        if m and labels[m.group(1)] == a and k < b and any(skip in l for l in lines[k:b + 1]):
            out.update(range(k + 1, b + 1))
    is_ins = lambda l: l.strip() and not l.strip().startswith((";", ".")) and not l.strip().endswith(":")
    row = collections.Counter(lines[k].split()[0] for k in range(a, b + 1) if k not in out and is_ins(lines[k]))
    return row, collections.Counter(lines[k].split()[0] for k in sorted(out) if is_ins(lines[k]))


def fp64_valu(c):
    return sum(v for k, v in c.items() if k.startswith("v_") and "_f64" in k)


MIX_HEAD = "| kernel | instructions a row | fp64 VALU | of them fma / mul / add / other | other VALU | LDS reads (b128 / b64 / other) | scalar |"


def mix_cells(c):
    """The cells of one Counter under MIX_HEAD, after the kernel's name."""
    f64 = {k: v for k, v in c.items() if k.startswith("v_") and "_f64" in k}
    fma = sum(v for k, v in f64.items() if "fma" in k)
    mul, add = sum(v for k, v in f64.items() if k.startswith("v_mul")), sum(v for k, v in f64.items() if k.startswith("v_add"))
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    lds = sum(v for k, v in c.items() if k.startswith("ds_"))
    return "%d | %d | %d / %d / %d / %d | %d | %d / %d / %d | %d |" % (
        sum(c.values()), sum(f64.values()), fma, mul, add, sum(f64.values()) - fma - mul - add, valu - sum(f64.values()),
        c.get("ds_read_b128", 0), c.get("ds_read_b64", 0), lds - c.get("ds_read_b128", 0) - c.get("ds_read_b64", 0),
        sum(v for k, v in c.items() if k.startswith("s_")))


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def alternate(runs, steps, warmup):
    """{name: (median, min, max) ms} of the functions `runs`: name -> (fn, its own number of steps or None for `steps`), step by
    step in turn, every step timed by its own pair of HIP events after `warmup` calls (one for a run with its own count)."""
    import torch

    for k, (fn, n) in runs.items():
        for _ in range(warmup if n is None else 1):
            fn()
    # events made beforehand and ONE synchronise at the end: the device never idles between steps
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n or steps)]
          for k, (fn, n) in runs.items()}
    torch.cuda.synchronize()
    for i in range(steps):
        for k, (fn, n) in runs.items():
            if i < len(ev[k]):
                ev[k][i][0].record()
                fn()
                ev[k][i][1].record()
    torch.cuda.synchronize()
    return {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}
