"""The C-ABI library loads and exports every symbol include/gencomm_hip.h declares; host-side
plan queries (no GPU compute) behave. CPU only."""
import ctypes
import os
import re

import pytest

from gencomm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    txt = open(os.path.join(REPO, "include", "gencomm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gencomm_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def test_header_and_binding_agree():
    assert _declared_symbols() == sorted(_lib.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in _declared_symbols():
        assert hasattr(raw, sym), sym
    assert lib.gencomm_abi_version() == _lib.ABI_VERSION


def test_unet_param_table_matches_module(lib):
    from gencomm_amd import GenComm, synth
    for C in (8, 16, 64, 128):
        gen = GenComm(synth.default_gencomm_cfg(C, 3))
        named = dict(gen.denoiser.named_parameters())
        table = _lib.unet_param_table(C, 2, 2, 0)
        assert sorted(n for n, _, _ in table) == sorted(named)  # every UNet parameter is consumed
        off = 0
        for name, numel, o in table:
            assert named[name].numel() == numel and o == off
            off += numel
        assert off == lib.gencomm_unet_raw_floats(C, 2, 2, 0)
        assert lib.gencomm_unet_prepared_floats(C, 2, 2, 0, 3) > off


def test_enhancer_param_table_matches_module(lib):
    from gencomm_amd import Enhancer
    enh = Enhancer(64, [8, 8], 4)
    named = dict(enh.named_parameters())
    table = _lib.enhancer_param_table(64)
    live = {n for n, _, _ in table}
    assert live == {k for k in named if k.startswith(("block_1.norm", "block_1.mlp", "split_attn"))}
    for name, numel, _ in table:
        assert named[name].numel() == numel


def test_argument_errors_are_status_codes_not_exits(lib):
    assert lib.gencomm_unet_raw_floats(7, 2, 2, 0) == -1
    assert b"multiple of 8" in lib.gencomm_last_error()
    assert lib.gencomm_denoise_workspace_bytes(4, 64, 201, 704, 2, 2, 0) == -1  # odd H with a downsample
    assert b"even" in lib.gencomm_last_error()
    assert lib.gencomm_denoise_workspace_bytes(4, 64, 200, 704, 2, 2, 0) > 0
    # null pointers are rejected before anything is launched
    assert lib.gencomm_unet_fwd(None, None, None, None, 0, 1, 64, 16, 16, 2, 2, 0, 3, None, 0, None) == 1
    assert lib.gencomm_warp_attfuse_fwd(None, None, None, None, 1, 1, 8, 4, 4, None) == 1
    assert lib.gencomm_head_loss(None, None, None, None, None, None, None, None, None, None, 2, 2, 64, 128, 2, None, 0.7853,
                                 2.0, 2.0, 0.25, 2.0, 3.0, 2.0, 0.2, 2, None) == 1
    assert b"null pointer" in lib.gencomm_last_error()


def test_cpu_tensors_fail_loudly():
    import torch
    from gencomm_amd import AttFusion, Enhancer, GenComm, synth
    gen = GenComm(synth.default_gencomm_cfg(16, 3)).eval()
    with pytest.raises(_lib.GenCommHipError):
        with torch.no_grad():
            gen(torch.zeros(2, 16, 8, 8), torch.zeros(2, 2, 8, 8), torch.tensor([2]))
    with pytest.raises(_lib.GenCommHipError):
        with torch.no_grad():
            Enhancer(16, [8, 8], 4)(torch.zeros(2, 16, 8, 8), None, torch.tensor([2]))
    with pytest.raises(_lib.GenCommHipError):
        with torch.no_grad():
            AttFusion(16)(torch.zeros(2, 16, 8, 8), torch.tensor([2]), torch.zeros(1, 5, 5, 2, 3))


def test_attnblock_params_are_enumerated_when_present(lib):
    from gencomm_amd import GenComm, synth
    cfg = synth.default_gencomm_cfg(8, 3)
    cfg["model"]["attn_resolutions"] = [64]  # nominal 128 -> 64 at level 1
    gen = GenComm(cfg)
    assert gen.denoiser.attn_mask == 0b10
    named = dict(gen.denoiser.named_parameters())
    table = _lib.unet_param_table(8, 2, 2, 0b10)
    assert sorted(n for n, _, _ in table) == sorted(named)
    assert lib.gencomm_unet_raw_floats(8, 2, 2, 0b100) == -1  # bit beyond the number of levels


def test_integration_md_example_matches_the_binding():
    """INTEGRATION.md section 2 shows a maintainer how to call the C ABI: every `lib.<fn>(...)` call and every `argtypes`
    list in it must have exactly as many entries as the binding the package itself uses (a stale example shifts arguments
    and corrupts the call)."""
    import re
    from gencomm_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    block = text[text.index("```python\nimport ctypes as C, torch"):]
    block = block[:block.index("```", 10)]
    assert f"gencomm_abi_version() == {_lib.ABI_VERSION}" in block

    def top_level_args(s):
        depth, n, seen = 0, 0, False
        for ch in s:
            if ch in "([":
                depth += 1
            elif ch in ")]":
                depth -= 1
            elif ch == "," and depth == 0:
                n += 1
            if not ch.isspace():
                seen = True
        return n + 1 if seen else 0

    checked = 0
    for m in re.finditer(r"lib\.(gencomm_\w+)\.argtypes = \[([^\]]*)\]", block):
        assert top_level_args(m.group(2)) == len(_lib._SIGNATURES[m.group(1)][1]), m.group(1)
        checked += 1
    for m in re.finditer(r"lib\.(gencomm_\w+)\(", block):
        name, start = m.group(1), m.end()
        if name == "gencomm_abi_version" or name == "gencomm_last_error":
            continue
        depth, i = 1, start
        while depth:
            depth += {"(": 1, ")": -1}.get(block[i], 0)
            i += 1
        nargs = top_level_args(block[start:i - 1])
        want = len(_lib._SIGNATURES[name][1])
        if name == "gencomm_unet_num_params" or nargs == want:
            assert nargs == want, (name, nargs, want)
            checked += 1
        else:
            raise AssertionError((name, nargs, want))
    assert checked >= 8


def test_code_object_has_no_packed_fp32_instructions(tmp_path):
    """Disassemble the gfx950 code object of the built library: no v_pk_{fma,mul,add}_f32 anywhere (see gencomm_build_info
    in include/gencomm_hip.h), and the matrix-core instructions the design rests on are there."""
    import shutil, subprocess
    from gencomm_amd import _lib
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("llvm-objdump or the built library is not available")
    assert b"-packed-fp32-ops" in _lib.lib().gencomm_build_info()
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    objs = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert objs, os.listdir(tmp_path)
    asm = "\n".join(subprocess.run([objdump, "-d", str(tmp_path / o)], check=True, capture_output=True, text=True).stdout for o in sorted(objs))
    import re
    assert not re.search(r"v_pk_(fma|mul|add)_f32", asm)
    assert "v_mfma_f32_16x16x32_f16" in asm and "v_mfma_f32_4x4x1" in asm
    # the step noise is ONE field in every kernel: no kernel that runs Box-Muller (v_sin_f32) may round the product straight
    # to fp16 (v_fma_mix{lo,hi}_f16 = a single rounding; the other kernels round to fp32 first) -- csrc/common.h bm_pair
    parts = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", asm)
    noisy = [(n, b) for n, b in zip(parts[1::2], parts[2::2]) if "v_sin_f32" in b and ("latent_step" in n or "conv_out" in n or "step_noise" in n)]
    assert len(noisy) >= 6, [n for n, _ in noisy]
    for n, b in noisy:
        assert "v_fma_mixlo_f16" not in b and "v_fma_mixhi_f16" not in b, n


def _mfma_hazard_violations(asm):
    """gfx950 / ROCm 7.2: a matrix instruction that accumulates onto the result of a matrix instruction of ANOTHER input type
    (bf8 <-> f16) reads a stale half of the accumulator when it issues fewer than 6 wait states later; hipcc assumes SrcC
    forwarding and places such pairs back to back (tools/probes/mfma_mixed_dep_probe.hip). Returns the offending pairs: a
    dependent pair of different types with fewer than two other matrix instructions (>= 8 issue cycles) in between."""
    import re
    # Only the 16x16x32 forms (4 passes): the 32x32x16 forms (8 passes: enh_front_h_kernel, the general convolution) give exact results at
    # 0 wait states in both directions, alone and with 12 waves per SIMD (round 3: tools/probes/mfma32_mixed_dep_probe.hip,
    # profiles/r3_mfma32_probe.txt; re-confirmed in round 5: tools/probes/mfma_mixed_dep32_probe.hip, profiles/r5_mfma_mixed_dep32_probe.txt)
    pat = re.compile(r"^\s*(v_mfma_f32_16x16x32_(bf8_bf8|f16|bf16|fp8_fp8|bf8_fp8|fp8_bf8))\s+([av]\[\d+:\d+\]),\s*\S+,\s*\S+,\s*([av]\[\d+:\d+\]|0)")
    bad = []
    for name, body in zip(*(lambda p: (p[1::2], p[2::2]))(re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", asm))):
        recent = []   # (type, dst) of the matrix instructions issued so far, newest last; cleared by anything that waits long
        for line in body.split("\n"):
            m = pat.match(line)
            if m is None:
                continue
            typ, dst, srcc = ("8" if "8" in m.group(2) else "16"), m.group(3), m.group(4)
            for age, (t0, d0) in enumerate(reversed(recent[-2:])):
                if d0 == srcc and t0 != typ:
                    bad.append((name, line.strip(), age))
            recent.append((typ, dst))
    return bad


def test_code_object_keeps_mixed_type_matrix_instructions_apart(tmp_path):
    import shutil, subprocess
    from gencomm_amd import _lib
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump) or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("llvm-objdump or the built library is not available")
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    objs = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    asm = "\n".join(subprocess.run([objdump, "-d", str(tmp_path / o)], check=True, capture_output=True, text=True).stdout for o in sorted(objs))
    assert "v_mfma_f32_16x16x32_bf8_bf8" in asm          # the third-term instruction of the three-term products is there
    assert "v_mfma_f32_32x32x16_bf8_bf8" in asm          # ... and of the general convolution / wide weight gradient
    bad = _mfma_hazard_violations(asm)
    assert not bad, bad[:5]
    # the detector itself: the pair hipcc produced before the order was pinned
    sample = "\n0000 <k>:\n\tv_mfma_f32_16x16x32_bf8_bf8 v[18:21], v[22:23], v[18:19], v[2:5]\n\tv_mfma_f32_16x16x32_f16 v[18:21], v[36:39], v[58:61], v[18:21]\n"
    assert len(_mfma_hazard_violations(sample)) == 1


def _contract_violations(text):
    """File-scope `#pragma clang fp contract(...)` stays in force across #include boundaries until the next one, and the target has no
    push / pop: so every file-scope `off` must be answered by `fast` (the build's default) in the same file, with no #include in
    between. A file may open by stating `fast`. Pragmas inside a function body end with their block and are not looked at; namespace and
    extern "C" braces count as file scope. Returns what breaks the rule."""
    bad, state, seen, scopes = [], "fast", 0, []   # scopes: one entry per open brace, True for a namespace / linkage brace
    for no, line in enumerate(re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S).split("\n"), 1):
        if re.match(r"\s*#\s*include\b", line):
            if state == "off":
                bad.append(f"line {no}: #include while contraction is off")
            continue
        line = re.sub(r"//.*", "", re.sub(r'"(\\.|[^"\\])*"|\'(\\.|[^\'\\])\'', "", line))
        m = re.match(r"\s*#\s*pragma\s+clang\s+fp\s+contract\s*\((\w+)\)", line)
        if m and not any(not ns for ns in scopes):
            mode, seen = m.group(1), seen + 1
            if mode not in ("off", "fast") or (mode == state and not (mode == "fast" and seen == 1)):
                bad.append(f"line {no}: contract({mode}) while contraction is {state}")
            state = mode
        for i, ch in enumerate(line):
            if ch == "{":
                scopes.append(re.search(r"(namespace(\s+\w+)?|extern)\s*$", line[:i]) is not None)
            elif ch == "}" and scopes:
                scopes.pop()
    if state != "fast":
        bad.append("contraction is still off at the end of the file")
    return bad


def test_fp_contraction_is_a_property_of_each_file():
    """No file under csrc/ hands a contraction mode other than the build's default to whatever is parsed after it, so no kernel's
    rounding depends on the order of the #include lines -- which both translation units therefore keep sorted."""
    from gencomm_amd import _lib
    files = sorted(os.listdir(_lib.CSRC_DIR))
    assert len(files) >= 50
    for f in files:
        assert _contract_violations(open(os.path.join(_lib.CSRC_DIR, f)).read()) == [], f
    for src in _lib.hip_sources():
        own = re.findall(r'^#include "(\w+\.h)"', open(src).read(), flags=re.M)   # not ../../include/gencomm_hip.h
        assert own[0] == "common.h" and own[1:] == sorted(own[1:]) and len(own) >= 10, (src, own)
    # the detector itself: a header that turns contraction off and never back on, as iou3d_kernels.h once did ...
    kernel = "__device__ float f(float a, float b) {\n  return a * b + a;   // { \"}\"\n}\n"
    assert _contract_violations("#pragma once\nnamespace gc {\n#pragma clang fp contract(off)\n" + kernel + "}  // namespace gc\n")
    assert not _contract_violations("#pragma once\nnamespace gc {\n#pragma clang fp contract(off)\n" + kernel + "#pragma clang fp contract(fast)\n}\n")
    # ... an #include inside the region, a region opened twice ...
    assert _contract_violations('#pragma clang fp contract(off)\n#include "common.h"\n#pragma clang fp contract(fast)\n')
    assert _contract_violations("#pragma clang fp contract(off)\n#pragma clang fp contract(off)\n#pragma clang fp contract(fast)\n")
    # ... and a pragma scoped to a function body, which is none of its business
    assert not _contract_violations("namespace gc {\n__device__ float f(float a, float b) {\n#pragma clang fp contract(off)\n  return a * b + a;\n}\n}\n")


_SPLIT_HOME = {   # text of the exact fp16 split -> the only files under csrc/ that may hold it
    r"typedef\s+_Float16\b[^;]*ext_vector_type": {"common.h"},              # the vector types (shared with the packed step noise)
    r"__builtin_amdgcn_cvt_pk_bf8_f32": {"split_f16.h"},
    r"__builtin_amdgcn_cvt_scalef32_pk_bf8_f32": {"split_f16.h"},
}
# the copies that went: sp_split8 too -- the sparse kernel forms its products under its own contraction and calls the shared split_pair
_SPLIT_GONE = r"\b(c1_split8|sp_split8|enh_bf8x4|ENH_TSCALE|hc_s2_t|c1h[28]_t|c1f2_t|sph[28]_t|spf2_t|eh[28]_t|ef2_t|nz_half2_t|nz_float2_t)\b"


def _split_strays(name, text):
    """What a file says of the split arithmetic that only its home may say, or that nobody may say any more."""
    bad = [pat for pat, home in _SPLIT_HOME.items() if name not in home and re.search(pat, text)]
    return bad + sorted(set(m.group(0) for m in re.finditer(_SPLIT_GONE, text)))


def test_the_fp16_split_has_one_home():
    """The operand splits, the bf8 conversions and their vector types are written once (split_f16.h; the types in common.h) and included,
    not copied under a new prefix by each layer that runs on this arithmetic."""
    from gencomm_amd import _lib
    files = sorted(os.listdir(_lib.CSRC_DIR))
    assert "split_f16.h" in files and len(files) >= 50
    text = {f: open(os.path.join(_lib.CSRC_DIR, f)).read() for f in files}
    for f in files:
        assert _split_strays(f, text[f]) == [], f
    for pat, home in _SPLIT_HOME.items():   # ... and the home does hold it
        assert all(re.search(pat, text[h]) for h in home), pat
    users = [f for f in files if f != "split_f16.h" and re.search(r'^#include "split_f16\.h"', text[f], flags=re.M)]
    assert len(users) >= 8 and re.search(r'^#include "common\.h"', text["split_f16.h"], flags=re.M), users
    # the detector itself: a layer that declares the types again under its own prefix and converts to bf8 by hand ...
    copy = "typedef _Float16 xh2_t __attribute__((ext_vector_type(2)));\nint v = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);\n"
    assert _split_strays("next_layer_kernels.h", copy) == list(_SPLIT_HOME)[:2]
    assert _split_strays("split_f16.h", copy) == list(_SPLIT_HOME)[:1] and _split_strays("common.h", copy) == list(_SPLIT_HOME)[1:2]
    # ... and one that calls the shared code, or names a retired copy
    assert _split_strays("next_layer_kernels.h", "half2_t h; split8(v, xs, hi, lo); bf8x4(a, b, c, d);") == []
    assert _split_strays("next_layer_kernels.h", "enh_bf8x4(a, b, c, d) * ENH_TSCALE; eh8_t x;") == ["ENH_TSCALE", "eh8_t", "enh_bf8x4"]
