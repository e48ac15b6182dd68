"""Registers and scratch of every kernel in the built objects (celerite2_amd/build/*.o): lists the kernels that use more than 256
registers (arch + accumulation: ONE wavefront per SIMD) or any scratch -- intended for the fused log-likelihood pairs
(__launch_bounds__(64, 1)), an accident anywhere else (round 6: k_cols_walk<.., 0> at 442 registers, profiles/r06_large_nrhs.md).
Usage: python tools/kernel_regs.py [min registers, default 257]
kernel_rows() is the one parser of the objects' notes (tools/bench_inverse_diag.py takes its register table from it)."""
import glob, os, re, shutil, subprocess, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
llvm = "/opt/rocm/lib/llvm/bin"


def kernel_rows(pattern="c2_*.o"):
    """[(object, demangled kernel, registers, of them accumulation, scratch bytes, LDS bytes, spilled registers, SGPRs)] of the
    built objects matching `pattern`; [] where the objects or the llvm tools are not on this machine."""
    rows = []
    if not os.path.exists(llvm + "/llvm-readelf"):
        return rows
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(glob.glob(os.path.join(root, "celerite2_amd", "build", pattern))):
            if re.search(r"_[a-z0-9]+\.o$", os.path.basename(o)) and not os.path.exists(os.path.join(root, "celerite2_amd", "csrc", os.path.basename(o)[:-2] + ".hip")):
                continue   # objects of A/B builds
            # (llvm-objdump --offloading writes the bundle's members next to its input: work on a copy)
            cp = os.path.join(tmp, os.path.basename(o))
            shutil.copy(o, cp)
            subprocess.run([llvm + "/llvm-objdump", "--offloading", cp], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            cos = glob.glob(cp + ".*hipv4-amdgcn*")
            if not cos: continue   # (host code only)
            co = cos[0]
            out = subprocess.run([llvm + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for b in re.split(r"\n\s*- \.agpr_count:", out)[1:]:
                f = lambda key: int(re.search(r"\.%s:\s*(\d+)" % key, b).group(1))
                rows.append([os.path.basename(o)[:-2], re.search(r"\.name:\s*(\S+)", b).group(1), f("vgpr_count"), int(b.split("\n")[0].strip()),
                             f("private_segment_fixed_size"), f("group_segment_fixed_size"), f("vgpr_spill_count"), f("sgpr_count")])
    names = subprocess.run(["c++filt"], input="\n".join(r[1] for r in rows), capture_output=True, text=True).stdout.split("\n")
    for r, n in zip(rows, names):
        r[1] = n
    return [tuple(r) for r in rows]


if __name__ == "__main__":
    lim = int(sys.argv[1]) if len(sys.argv) > 1 else 257
    rows = kernel_rows()
    print(len(rows), "kernels; those with >= %d registers or scratch:" % lim)
    for r in sorted(rows, key=lambda x: (x[0], -x[2])):
        if r[2] >= lim or r[4] > 0:
            print("%-20s %-110s registers %4d (accumulation %3d) scratch %d B" % (r[0], r[1].split("(")[0].replace("void ", "")[:110], r[2], r[3], r[4]))
