#!/usr/bin/env python3
"""Do two builds hold the same device code?  Compares, function by function, the gfx950 assembly of two source trees (each
gencomm_amd/csrc/*.hip compiled with gencomm_amd._lib.HIP_FLAGS --cuda-device-only -S, both trees concurrently), of two .s files or
of two built .so files (disassembled).  Comments, blank lines and the numbers of compiler-local labels are dropped, and only functions are
read, so the __hip_cuid_<hash> object that hipcc derives from the source text is ignored: a refactor that moves no instruction compares equal.
Usage: python tools/code_object_diff.py OLD NEW        (no GPU needed; exit status 1 when a function was added, removed or changed)"""
import os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gencomm_amd import _lib  # noqa: E402
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def functions(asm):
    """{name: normalised body} of `.type NAME,@function` ... `.size NAME,` in compiler output"""
    asm = re.sub(r";.*", "", asm)
    asm = re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", asm)   # .LBB<function>_<block>: the function's number goes, the block's stays
    asm = re.sub(r"\.(Lfunc_begin|Lfunc_end|Ltmp)\d+", r".\1", asm)
    out = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\s*\.size\s+\1,", asm, re.S | re.M):
        out[m.group(1)] = "\n".join(l.rstrip() for l in m.group(2).split("\n") if l.strip())
    return out


def disassembled(so, tmp):
    """the same of a built library: its gfx950 code objects, `<NAME>:` ... in llvm-objdump -d (addresses and encodings dropped)"""
    os.makedirs(tmp)
    so = shutil.copy(so, os.path.join(tmp, "lib.so"))   # --offloading writes the code objects next to its input
    subprocess.run([OBJDUMP, "--offloading", so], check=True, capture_output=True, cwd=tmp)
    out = {}
    for o in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
        dis = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, o)], check=True, capture_output=True, text=True).stdout
        # where a function lies shows in two places that are no change of its code: the pc-relative literal behind s_getpc_b64 (the
        # distance to a callee or a table) and the padding behind the last function of a section
        dis = re.sub(r"(s_getpc_b64 [^\n]*\n\s*s_add_u32 [^\n]*, )(0x[0-9a-f]+|-?\d+)", r"\1<pcrel>", re.sub(r"\s*//.*", "", dis))
        parts = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", dis)
        for n, b in zip(parts[1::2], parts[2::2]):
            out[n] = re.sub(r"(\n\t(s_nop 0|s_code_end|\t\.\.\.))+$", "", "\n".join(l for l in b.split("\n") if l.startswith("\t")))
    return out


def compile_unit(src, out):
    subprocess.run(["/opt/rocm/bin/hipcc", *_lib.HIP_FLAGS, "--cuda-device-only", "-S", src, "-o", out], check=True)
    return functions(open(out).read())


def load(pool, path, tmp):
    """{unit: future of {function: body}} of a tree, a .s file or a .so file"""
    if path.endswith(".s"):
        return {"": pool.submit(lambda: functions(open(path).read()))}
    if path.endswith(".so"):
        return {"": pool.submit(disassembled, path, tmp)}
    csrc = os.path.join(path, "gencomm_amd", "csrc")
    os.makedirs(tmp)
    return {f: pool.submit(compile_unit, os.path.join(csrc, f), os.path.join(tmp, f + ".s")) for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(16) as pool:
        old, new = (load(pool, p, os.path.join(d, side)) for side, p in zip(("old", "new"), sys.argv[1:]))
        differences = 0
        for unit in sorted(set(old) | set(new)):
            a, b = (side[unit].result() if unit in side else {} for side in (old, new))
            if not a and not b:
                sys.exit(f"{unit or 'code object'}: no function found on either side")
            diff = [("removed", n) for n in sorted(set(a) - set(b))] + [("added", n) for n in sorted(set(b) - set(a))] + \
                   [("changed", n) for n in sorted(set(a) & set(b)) if a[n] != b[n]]
            print(f"{unit or 'code object'}: {len(a)} -> {len(b)} functions, {len(diff)} differ")
            dem = subprocess.run(["c++filt"], input="\n".join(n for _, n in diff), capture_output=True, text=True).stdout.split("\n")
            for (what, _), n in zip(diff, dem):
                print(f"  {what:8} {n[:160]}")
            differences += len(diff)
    sys.exit(1 if differences else 0)


if __name__ == "__main__":
    main()
