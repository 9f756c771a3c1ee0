#!/usr/bin/env python3
"""Per-kernel VGPR / AGPR / scratch / occupancy / LDS of the library build (hipcc -Rpass-analysis=kernel-resource-usage), for
both translation units, compiled with the flags of gencomm_amd._lib.build (HIP_FLAGS).
Usage: python tools/resource_usage.py [--csrc DIR] [--insts] [substring ...]   (no GPU needed)
  --csrc DIR   compile DIR/gencomm_abi*.hip instead of the tree's (DIR/../../include/gencomm_hip.h must exist): another checkout
  --insts      one more column: the kernel's instruction count in the assembly that --save-temps leaves"""
import argparse, os, re, subprocess, sys, tempfile
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gencomm_amd import _lib  # noqa: E402


def instruction_counts(asm):
    """{mangled kernel name: instructions between its label and its end label}"""
    counts, name = {}, None
    for line in open(asm):
        if name is None:
            if (m := re.match(r"(_Z\w+):", line)):
                name, n = m.group(1), 0
        elif line.startswith(".Lfunc_end"):
            counts[name], name = n, None
        elif re.match(r"\s+[a-z]", line):   # directives begin with '.', comments with ';', labels in column 0
            n += 1
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=_lib.CSRC_DIR)
    ap.add_argument("--insts", action="store_true")
    ap.add_argument("pats", nargs="*")
    a = ap.parse_args()
    srcs = [os.path.join(os.path.abspath(a.csrc), os.path.basename(s)) for s in _lib.hip_sources()]
    with tempfile.TemporaryDirectory() as d:
        cmds = [["/opt/rocm/bin/hipcc", *_lib.HIP_FLAGS, "-Rpass-analysis=kernel-resource-usage", *(["--save-temps"] if a.insts else []),
                 "-c", s, "-o", os.path.join(d, os.path.basename(s) + ".o")] for s in srcs]
        procs = [subprocess.Popen(c, cwd=d, stderr=subprocess.PIPE, text=True) for c in cmds]   # one pipe each: the remarks do not interleave
        errs = [p.communicate()[1] for p in procs]
        if any(p.returncode for p in procs):
            sys.exit("\n".join(errs))
        sys.stderr.write("".join(l for e in errs for l in e.splitlines(True) if "warning:" in l))   # the build's -Wall, not lost among the remarks
        insts = {}
        for f in os.listdir(d) if a.insts else []:
            if f.endswith(".s") and "amdgcn" in f:
                insts.update(instruction_counts(os.path.join(d, f)))
    blocks = [b for e in errs for b in re.split(r"remark: [^\n]*Function Name: ", e)[1:]]
    names = [b.split()[0] for b in blocks]   # the mangled name; the remark's own flag follows it
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    print(f"{'VGPR':>5} {'AGPR':>5} {'scratch':>8} {'occ':>4} {'LDS':>7} " + (f"{'insts':>6} " if a.insts else "") + " kernel")
    for b, mangled, n in zip(blocks, names, dem):
        if a.pats and not any(p in n for p in a.pats):
            continue
        g = lambda k: int(m.group(1)) if (m := re.search(k + r": (\d+)", b)) else -1
        vals = (g("VGPRs"), g("AGPRs"), g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]"))
        print("%5d %5d %8d %4d %7d " % vals + ("%6d " % insts.get(mangled, -1) if a.insts else "") + " " + n[:140])


if __name__ == "__main__":
    main()
