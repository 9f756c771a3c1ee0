"""Training STAMP's adapter / reverter without a GPU: the restatement's autograd against the reference's gradients
(tests/golden/stamp_adapter_train_*.npz), the trainable switch, the ABI declarations of the block backward, its workspace budget, and the
LDS bank arithmetic of the matrix-operand reads of csrc/convnext_bwd_kernels.h.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stamp_adapter_restatement as R
import stamp_adapter_train_restatement as T
from test_lds_banks import B128_GROUPS, extra_cycles
from gencomm_amd import Adapter, Reverter, _lib

REPO = Path(__file__).resolve().parents[1]
CLASSES = {"Adapter": Adapter, "Reverter": Reverter}
HEADER = REPO / "gencomm_amd" / "csrc" / "convnext_bwd_kernels.h"
_cache = {}


def _case(name):
    """(fixture, {dtype: restatement gradients}) of one case, computed once."""
    if name not in _cache:
        g = T.load_fixture(name)
        seed = int(g["seed"])
        if name == "step":
            data = T.step_data(seed)
            l64, r64 = T.step_grads(data, torch.float64)
            _, r32 = T.step_grads(data, torch.float32)
            sums = (R.checksum(list(data[1].values()) + list(data[3].values())), R.checksum([data[4], data[5]]), None)
            assert abs(l64 - float(g["loss64"])) <= 1e-12 * abs(l64)
        else:
            cls, cfg, sd, x = R.case_data(name, seed)
            prefix = R.prefix_of(cls)
            with torch.no_grad():
                G = T.make_G(tuple(R.adapter_forward(cfg, sd, prefix, x).shape), seed + 2)
            r64, r32 = T.module_grads(cfg, sd, prefix, x, G, torch.float64), T.module_grads(cfg, sd, prefix, x, G, torch.float32)
            sums = (R.checksum(sd.values()), R.checksum([x]), R.checksum([G]))
        _cache[name] = (g, r64, r32, sums)
    return _cache[name]


@pytest.mark.parametrize("name", T.TRAIN_CASES + ("step",))
def test_restatement_autograd_is_the_reference_in_float64(name):
    g, r64, _, sums = _case(name)
    same = lambda a, b: abs(a - float(b)) <= 1e-12 * abs(float(b))      # a float64 sum: its last digit depends on the host's reduction order
    assert same(sums[0], g["checksum_params"]) and same(sums[1], g["checksum_x"])
    assert sums[2] is None or same(sums[2], g["checksum_G"])
    keys = [str(k) for k in g["keys"]]
    assert keys == sorted(r64)
    assert not [k for k in g if "smoothing" in k]
    for i, k in enumerate(keys):
        if f"grad64/{k}" in g:
            assert T.rel_rms(r64[k], torch.from_numpy(g[f"grad64/{k}"])) <= 1e-10, k
        else:
            assert r64[k].numel() > T.DIGEST_ABOVE
            ref, got = g[f"digest64/{k}"], T.digest(r64[k], int(g["seed"]), i)
            assert np.all(np.abs(got - ref) <= 1e-10 * np.sqrt(ref[1]) * np.array([np.sqrt(r64[k].numel()), np.sqrt(ref[1]), 3.0, 3.0])), k


@pytest.mark.parametrize("name", T.TRAIN_CASES + ("step",))
def test_float32_yardsticks_are_inside_the_criterion(name):
    """The stored yardstick is the reference's own float32 error; the float32 restatement (another float32 run of the same graph) meets
    the criterion built from it, and no yardstick is so large that the criterion would be empty."""
    g, _, r32, _ = _case(name)
    for i, k in enumerate(str(k) for k in g["keys"]):
        yard = float(g[f"yard/{k}"])
        assert 0.0 < yard < 1e-6, (k, yard)        # the 1e-6 floor or at most twice it is the operative bound everywhere
        if f"grad64/{k}" in g:
            T.check(k, r32[k], torch.from_numpy(g[f"grad64/{k}"]), yard)
        else:
            T.check_digest(k, r32[k], g[f"digest64/{k}"], yard, int(g["seed"]), i)


def test_no_fixture_file_outgrows_the_largest_committed_one():
    files = sorted((REPO / "tests" / "golden").glob("stamp_adapter_train_*.npz"))
    assert len(files) >= 5 and all(f.stat().st_size <= 1205138 for f in files)
    for f in files:
        with np.load(f) as z:
            assert not [k for k in z.files if k.startswith(("param", "weight"))]     # seeds, checksums, gradients, digests, yardsticks


@pytest.mark.parametrize("key", list(R.SHIPPED))
@pytest.mark.parametrize("cls", ["Adapter", "Reverter"])
def test_trainable_keeps_the_state_dict(key, cls):
    cfg = R.SHIPPED[key]
    mod, plain = CLASSES[cls](cfg, trainable=True), CLASSES[cls](cfg)
    assert len(mod.state_dict()) == 33
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == [(k, tuple(v.shape)) for k, v in plain.state_dict().items()]
    sd = R.make_params(cfg, R.prefix_of(cls), 5)
    mod.load_state_dict(sd, strict=True)
    assert all(torch.equal(mod.state_dict()[k], v) for k, v in sd.items())


@pytest.mark.parametrize("cls", ["Adapter", "Reverter"])
def test_trainable_reaches_the_device_check_and_the_default_still_refuses(cls):
    x = torch.zeros(1, 128, 4, 4)
    with pytest.raises(_lib.GenCommHipError):
        CLASSES[cls](R.SHIPPED["in128_dim64"], trainable=True)(x)
    with pytest.raises(_lib.GenCommHipError):
        CLASSES[cls](R.SHIPPED["in128_dim64"], trainable=True)(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError) as e:
        CLASSES[cls](R.SHIPPED["in128_dim64"])(x)
    assert str(e.value) == ("stamp adapter training is not implemented (the backward of the fused ConvNeXt block is missing): call under "
                            "torch.no_grad(), or freeze the parameters and detach the input")
    for other in ("adapterfc", "adapterdsa", "adapteratt"):
        with pytest.raises(NotImplementedError, match="not implemented"):
            CLASSES[cls]({"core_method": other, "args": R.base_args(128)}, trainable=True)


def test_header_declares_and_binding_matches():
    header = (REPO / "include" / "gencomm_hip.h").read_text()
    assert "#define GENCOMM_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    for name, res, count in (("gencomm_convnext_block_bwd_workspace_bytes", "long long", 6), ("gencomm_convnext_block_bwd", "int", 30)):
        m = re.search(res + r" " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        r, args = _lib._SIGNATURES[name]
        assert len(params) == len(args) == count, (name, len(params), len(args))
        assert r is (_lib._ll if res == "long long" else _lib._i)
        for p, a in zip(params, args):
            assert ("*" in p) == (a is _lib._p), (p, a)
            assert ("long long" in p) == (a is _lib._ll) or "*" in p, (p, a)
        assert name in _lib.EXPORTED_SYMBOLS
    assert '#include "convnext_bwd_kernels.h"' in (REPO / "gencomm_amd" / "csrc" / "gencomm_abi_aux.hip").read_text()


def test_launch_constants_are_the_headers():
    from gencomm_amd import convnext_bwd as B
    src = HEADER.read_text()
    m = re.search(r"constexpr int kCnxBwdLaunches = (\d+), kCnxBwdLaunchesDxOnly = (\d+);", src)
    assert m and (B.LAUNCHES, B.LAUNCHES_DX_ONLY) == (int(m.group(1)), int(m.group(2)))
    assert B.LAUNCHES_DX_ONLY < B.LAUNCHES <= 6
    assert src.count("GC_KLOG(") == 8     # two of the six launches have one instantiation per width


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("dx_only", [0, 1])
def test_workspace_grows_by_less_than_one_hidden_row_per_pixel(C, dx_only):
    q = _lib.lib().gencomm_convnext_block_bwd_workspace_bytes
    a, b = q(5, C, 128, 256, dx_only, 0), q(10, C, 128, 256, dx_only, 0)
    assert 0 < a < b
    assert (b - a) <= 3 * C * 4 * (5 * 128 * 256)
    assert q(1, C, 1, 1, dx_only, 0) > 0 and q(1, C, 19, 35, dx_only, 4) > 0
    for bad in ((0, C, 4, 4, dx_only, 0), (1, 32, 4, 4, dx_only, 0), (1, C, 4, 4, 2, 0), (1, C, 4, 4, dx_only, -1)):
        assert q(*bad) == -1


def test_no_module_named_after_the_shell_was_added():
    names = {p.stem for p in (REPO / "gencomm_amd").glob("*.py")}
    assert "convnext_bwd" in names
    assert not [n for n in names if ("stamp" in n and n != "stamp_adapter") or "adapter_loss" in n]


# ------------------------------------------------------------------------------------------------ LDS bank arithmetic
def _constants():
    fwd = (REPO / "gencomm_amd" / "csrc" / "convnext_kernels.h").read_text()
    src = HEADER.read_text()
    g = lambda pat: int(re.search(pat, fwd).group(1))
    # the operand patterns restated below, as the kernels write them
    assert src.count("constexpr int LD = C + kCnxPad, LH = kCnxChunk + kCnxPad") == 1 and "constexpr int LD = C + kCnxPad, R = kCnxRows, NC = C / 16;" in src
    assert src.count("cnx_mma<C, 1, LD>(ln + lr * LD + 4 * lk") == 2 and src.count("cnx_mma<C, 1, LD>(dyi + lr * LD + 4 * lk") == 2
    assert src.count("cnx_mma<kCnxChunk, NT, LH>(du + lr * LH + 4 * lk") == 1
    assert len(re.findall(r"cnx_mma<[^>]*>\(", src)) == 5      # every call is one of the five above
    assert "const int prow = (16 * rt + 4 * lk + e) * LD + lr;" in src and "dyi[prow + 16 * t]" in src and "ln[prow + 16 * t]" in src
    return dict(chunk=g(r"kCnxChunk = (\d+);"), pad=g(r"kCnxPad = (\d+);"))


def _a_operand_extra_cycles(ld, k):
    """cnx_mma's A operand: one ds_read_b128 per lane at [row lane % 16 of row tile rt][k0 + 4 (lane / 16)], `ld` floats per row."""
    extra = reads = 0
    for rt in range(4):
        for k0 in range(0, k, 16):
            addrs = [4 * ((16 * rt + (l & 15)) * ld + k0 + 4 * (l >> 4)) for l in range(64)]
            extra += extra_cycles(addrs, B128_GROUPS, 16)
            reads += 1
    return extra, reads


def test_matrix_operand_b128_reads_of_the_backward_are_conflict_free():
    c = _constants()
    for dim in (64, 128):      # u = ln W1^T and dh = dy W2G^T, in the pixel pass and in the weight pass: images of C + pad floats per row
        extra, reads = _a_operand_extra_cycles(dim + c["pad"], dim)
        assert extra == 0, f"{extra} extra LDS cycles over {reads} ds_read_b128 at C = {dim}"
    extra, reads = _a_operand_extra_cycles(c["chunk"] + c["pad"], c["chunk"])     # dln += du W1T^T reads the du image
    assert extra == 0, f"{extra} extra LDS cycles over {reads} ds_read_b128 of the du image"


def test_weight_pass_dword_operand_conflict_is_the_pinned_two_way_one():
    """The B operand of the two weight-gradient products is ONE dword per lane at [pixel 16 rt + 4 lk + e][16 t + lr]: ds_read_b32 is
    served in lane groups {0-31}, {32-63} on 32 banks, and 4 (C + 8) = 0 mod 32 puts lk and lk + 1 on the same banks: one extra cycle
    per group, 2 per read, at both widths. Pinned, not fixed: a read feeds one 16x16x4 MFMA (32 cycles of matrix work); a row stride of
    4 mod 8 floats would remove it and break the conflict-free ds_read_b128 of the A operand above (the header says so)."""
    c = _constants()
    for dim in (64, 128):
        ld = dim + c["pad"]
        for rt in range(4):
            for e in range(4):
                for t in range(dim // 16):
                    addrs = [(16 * rt + 4 * (l >> 4) + e) * ld + 16 * t + (l & 15) for l in range(64)]
                    extra = 0
                    for grp in (range(0, 32), range(32, 64)):
                        per_bank = {}
                        for l in grp:
                            per_bank.setdefault(addrs[l] % 32, set()).add(addrs[l])
                        extra += max(len(v) for v in per_bank.values()) - 1
                    assert extra == 2
    assert "2-way conflict" in HEADER.read_text()
