"""STAMP's adapter / reverter without a GPU: the restatement against the reference's float64 outputs (tests/golden/stamp_adapter.npz), the
module's state_dict against the reference's key lists, every refusal, the ABI declarations, and the LDS bank arithmetic of the fused
block kernel's matrix-operand reads.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import stamp_adapter_restatement as R
from test_lds_banks import B128_GROUPS, extra_cycles
from gencomm_amd import Adapter, Reverter, _lib

REPO = Path(__file__).resolve().parents[1]
GOLD = np.load(REPO / "tests" / "golden" / "stamp_adapter.npz")
CLASSES = {"Adapter": Adapter, "Reverter": Reverter}


def _case(name):
    return R.case_data(name, int(GOLD[f"{name}/seed"]))


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_the_reference_in_float64(name):
    cls, cfg, sd, x = _case(name)
    assert R.checksum(sd.values()) == float(GOLD[f"{name}/checksum_params"]) and R.checksum([x]) == float(GOLD[f"{name}/checksum_x"])
    ref = torch.from_numpy(GOLD[f"{name}/out64"])
    got = R.adapter_forward(cfg, sd, R.prefix_of(cls), x, torch.float64)
    assert got.shape == ref.shape and got.dtype == torch.float64
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_fixture_reference_float32_is_inside_the_tolerance():
    for name in R.CASES:
        assert float(GOLD[f"{name}/ref32_ratio"]) < 1.0


def test_the_chain_case_is_inside_the_tolerance_in_the_restatements_own_float32():
    c = R.chain_data(int(GOLD["cnx64/seed"]), int(GOLD["rev64/seed"]))
    ok, worst = R.within(R.chain_forward(*c, torch.float32), R.chain_forward(*c, torch.float64))
    assert ok and worst < 0.5, worst


@pytest.mark.parametrize("name", ["cnx64", "cnx128", "rev64"])
def test_every_block_of_the_fixture_is_visible_next_to_its_residual(name):
    """gamma is random, not the reference's 1e-6: what a block adds is more than a tenth of its output, in the median."""
    cls, cfg, sd, x = _case(name)
    trace = []
    R.adapter_forward(cfg, sd, R.prefix_of(cls), x, torch.float64, trace)
    shares = [R.branch_share(a, b) for a, b in trace]
    assert len(shares) == 3 and all(s > R.MIN_BRANCH_SHARE for s in shares), shares
    assert np.allclose(shares, GOLD[f"{name}/branch_shares"], rtol=1e-9)
    gammas = [v for k, v in sd.items() if k.endswith(".gamma")]
    assert len(gammas) == 3 and all(float(g.abs().median()) > 0.05 for g in gammas)


@pytest.mark.parametrize("key", list(R.SHIPPED))
@pytest.mark.parametrize("cls", ["Adapter", "Reverter"])
def test_state_dict_keys_and_shapes_are_the_references(key, cls):
    mod = CLASSES[cls](R.SHIPPED[key])
    ours = [f"{k} {list(v.shape)}" for k, v in mod.state_dict().items()]
    assert len(ours) == 33 and ours == list(GOLD[f"keys/{key}/{cls}"])
    assert list(R.param_shapes(R.SHIPPED[key], R.prefix_of(cls))) == list(mod.state_dict())


def test_a_reference_shaped_state_dict_loads_strictly():
    for cls in ("Adapter", "Reverter"):
        cfg = R.SHIPPED["in128_dim64"]
        sd = R.make_params(cfg, R.prefix_of(cls), 11)
        mod = CLASSES[cls](cfg)
        mod.load_state_dict(sd, strict=True)
        assert torch.equal(mod.state_dict()[f"{R.prefix_of(cls)}.conv.model.2.gamma"], sd[f"{R.prefix_of(cls)}.conv.model.2.gamma"])
    _, cfg, sd, _ = _case("conv")
    Adapter(cfg).load_state_dict(sd, strict=True)
    assert len(Adapter(R.CASES["identity"][1]).state_dict()) == 0


def test_pad_arithmetic_is_base_adapters():
    cfg = R.CASES["conv"][1]
    assert Adapter(cfg).adapter.pad == (2, 2, 2, 2) == R.pad_of(cfg["args"])[1]
    assert Adapter(R.SHIPPED["in128_dim64"]).adapter.pad == (0, 0, 0, 0)


def _sub(**kw):
    return R.shipped(128, 64, **kw)


@pytest.mark.parametrize("cfg,needle", [
    (_sub(kernel_size=3), "kernel_size"),
    (_sub(deform=True), "deform"),
    ({"core_method": "adapterconvnext", "args": R.base_args(128, sub=dict(num_of_blocks=3, dim=32))}, "dim"),
    ({"core_method": "adapterfc", "args": R.base_args(128)}, "adapterfc"),
    ({"core_method": "adapterdsa", "args": R.base_args(128)}, "adapterdsa"),
    ({"core_method": "adapteratt", "args": R.base_args(128)}, "adapteratt"),
    ({"core_method": "nonsense", "args": R.base_args(128)}, "nonsense"),
    ({"core_method": "adapterconvnext", "args": R.base_args(128, sub=dict(num_of_blocks=3, dim=64), out_shape=(256, 512))}, "in_feature_shape/out_feature_shape"),
    ({"core_method": "adapterconv", "args": R.base_args(128, out_shape=(64, 128))}, "in_feature_shape/out_feature_shape"),
    ({"core_method": "identity", "args": R.base_args(128, out_shape=(64, 128))}, "in_feature_shape/out_feature_shape"),
    ({"core_method": "identity", "args": R.base_args(128, 64)}, "in_channels"),
])
@pytest.mark.parametrize("cls", ["Adapter", "Reverter"])
def test_refusals_name_their_key(cfg, needle, cls):
    with pytest.raises(NotImplementedError, match=re.escape(needle)):
        CLASSES[cls](cfg)


@pytest.mark.parametrize("cls", ["Adapter", "Reverter"])
def test_a_grad_enabled_call_is_refused(cls):
    mod = CLASSES[cls](R.SHIPPED["in128_dim64"])
    x = torch.zeros(1, 128, 4, 4)
    with pytest.raises(NotImplementedError, match="stamp adapter training"):
        mod(x)                                     # trainable parameters
    for p in mod.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="stamp adapter training"):
        mod(x.clone().requires_grad_(True))        # trainable input
    with pytest.raises(_lib.GenCommHipError):      # nothing to train: the call reaches the device check
        mod(x)


def test_header_declares_and_binding_matches():
    header = (REPO / "include" / "gencomm_hip.h").read_text()
    assert "#define GENCOMM_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    m = re.search(r"int gencomm_convnext_block_fwd\(([^;]*)\);", header)
    assert m, "gencomm_convnext_block_fwd is not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib._SIGNATURES["gencomm_convnext_block_fwd"]
    assert len(params) == len(args) == 16
    for p, a in zip(params, args):
        assert ("*" in p) == (a is _lib._p), (p, a)
    assert "feature_alignnet_modules.py:303-348" in header
    assert '#include "convnext_kernels.h"' in (REPO / "gencomm_amd" / "csrc" / "gencomm_abi_aux.hip").read_text()
    assert "gencomm_convnext_block_fwd" in _lib.EXPORTED_SYMBOLS


def test_no_baseline_shell_module_was_added():
    names = {p.stem for p in (REPO / "gencomm_amd").glob("*.py")}
    assert "stamp_adapter" in names
    assert not [n for n in names if "stamp" in n and n != "stamp_adapter"]
    assert "adapter_loss" not in names and not [n for n in names if n.startswith("heter_model_baseline_w_") and "gencomm" not in n]


def _kernel_constants():
    src = (REPO / "gencomm_amd" / "csrc" / "convnext_kernels.h").read_text()
    g = lambda pat: int(re.search(pat, src).group(1))
    assert "constexpr int LD = C + kCnxPad, LH = kCnxChunk + kCnxPad" in src, "the LDS row strides changed: restate them here"
    assert "cnx_mma<C, 1, LD>(ln + lr * LD + 4 * lk" in src and "cnx_mma<kCnxChunk, NT, LH>(h + lr * LH + 4 * lk" in src
    assert "aq[set][rt] = *reinterpret_cast<const float4*>(ap + rt * 16 * LDA + k0);" in src
    return dict(tile_h=g(r"kCnxTileH = (\d+)"), tile_w=g(r"kCnxTileW = (\d+)"), chunk=g(r"kCnxChunk = (\d+);"), pad=g(r"kCnxPad = (\d+);"))


def _a_operand_extra_cycles(ld, k):
    """The A operand of a matrix step: one ds_read_b128 per lane at [row lane % 16 of row tile rt][k0 + 4 (lane / 16)] of an image with
    `ld` floats per row."""
    extra = reads = 0
    for rt in range(4):
        for k0 in range(0, k, 16):
            addrs = [4 * ((16 * rt + (l & 15)) * ld + k0 + 4 * (l >> 4)) for l in range(64)]
            assert all(a % 16 == 0 for a in addrs)
            extra += extra_cycles(addrs, B128_GROUPS, 16)
            reads += 1
    return extra, reads


def test_matrix_operand_reads_are_bank_conflict_free():
    c = _kernel_constants()
    assert (c["tile_h"] * c["tile_w"], c["chunk"]) == (64, 64)
    for dim in (64, 128):
        extra, reads = _a_operand_extra_cycles(dim + c["pad"], dim)          # Linear1 reads the LayerNorm image
        assert extra == 0, f"{extra} extra LDS cycles over {reads} ds_read_b128 at C = {dim}"
    extra, reads = _a_operand_extra_cycles(c["chunk"] + c["pad"], c["chunk"])  # Linear2 reads the hidden chunk
    assert extra == 0, f"{extra} extra LDS cycles over {reads} ds_read_b128 of the hidden chunk"
    assert _a_operand_extra_cycles(64 + 4, 64)[0] > 0                          # the padding matters: 4 floats would conflict
