"""The fused ConvNeXt-block kernel (gencomm_convnext_block_fwd) and the STAMP adapter / reverter modules on the GPU.

The block against the float64 restatement (tests/stamp_adapter_restatement.py, pinned to the reference by tests/test_stamp_adapter.py),
elementwise |got - ref| <= 1e-5 + 1e-4 |ref| with no element left out, at the smallest shapes where it can go wrong: maps
smaller than the 7 x 7 window, batches, ragged tiles on both axes, several tiles per axis (from the kernel's own tile constants), both
instantiations, gamma absent.  The depthwise taps are random and asymmetric: a flipped or transposed window, or swapped axes, fails.
The modules against the reference's float64 outputs of tests/golden/stamp_adapter.npz.
"""
import os
import re

import numpy as np
import pytest
import torch

import stamp_adapter_restatement as R
from gencomm_amd import Adapter, Reverter, _lib
from gencomm_amd.runtime import ptr, stream_ptr
from gencomm_amd.stamp_adapter import convnext_block

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "stamp_adapter.npz"))
DEV = torch.device("cuda:0")
ORDER = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias", "gamma")
_cache = {}


def _tile():
    src = open(os.path.join(HERE, "..", "gencomm_amd", "csrc", "convnext_kernels.h")).read()
    return int(re.search(r"kCnxTileH = (\d+)", src).group(1)), int(re.search(r"kCnxTileW = (\d+)", src).group(1))


TILE_H, TILE_W = _tile()
BLOCK_SHAPES = [
    (64, 1, 1, 1), (64, 1, 3, 5), (64, 1, 6, 7),            # smaller than the window: every tap hits padding somewhere
    (64, 2, 8, 8), (64, 3, 9, 17),                          # batch stride, non-square, edges inside a tile on both axes
    (64, 1, 19, 35),
    (64, 1, TILE_H + 1, 2 * TILE_W + 1),                    # several tiles per axis, ragged last tile
    (128, 1, 3, 5), (128, 2, 9, 17),
]


def _block_case(C, n, H, W, gamma=True):
    """(params, x, float64 reference) of one block, computed once and shared. x has standard deviation 2, what channel_convert1 hands the
    first block in the fixture's cases: the LayerNorm inputs keep a channel variance of order 1 even on the 1 x 1 map."""
    key = (C, n, H, W, gamma)
    if key not in _cache:
        seed = 9000 + 131 * C + 17 * n + 5 * H + W
        p = R.make_block_params(C, seed)
        if not gamma:
            p["gamma"] = None
        x = 2.0 * R.make_x((n, C, H, W), seed + 1)
        _cache[key] = (p, x, R.convnext_block(p, x, torch.float64))
    return _cache[key]


def _run_block(p, x):
    xd = x.to(DEV)
    return xd, convnext_block(xd, *[None if p[k] is None else p[k].to(DEV) for k in ORDER])


@pytest.mark.parametrize("C,n,H,W", BLOCK_SHAPES)
def test_block_against_float64(C, n, H, W):
    p, x, ref = _block_case(C, n, H, W)
    _, y = _run_block(p, x)
    ok, worst = R.within(y.cpu(), ref)
    print(f"C {C} x [{n}, {C}, {H}, {W}]: worst |d| / (1e-5 + 1e-4 |ref|) = {worst:.3f}, max |ref| {float(ref.abs().max()):.2f}")
    assert ok, worst


def test_block_without_gamma():
    p, x, ref = _block_case(64, 2, 8, 8, gamma=False)
    _, y = _run_block(p, x)
    ok, worst = R.within(y.cpu(), ref)
    assert ok, worst
    assert float((ref - x.double()).abs().median()) > 0.1 * float(ref.abs().median())


def test_the_reference_would_catch_a_flipped_or_transposed_window():
    """The taps are asymmetric: the float64 block with its window flipped, transposed, or with H and W swapped is far outside the tolerance."""
    p, x, ref = _block_case(64, 3, 9, 17)
    for name, w in (("flipped", p["dwconv.weight"].flip(-1, -2)), ("transposed", p["dwconv.weight"].transpose(-1, -2))):
        bad = R.convnext_block(dict(p, **{"dwconv.weight": w}), x, torch.float64)
        assert R.within(bad, ref)[1] > 100.0, name
    swapped = R.convnext_block(p, x.transpose(-1, -2), torch.float64).transpose(-1, -2)
    assert R.within(swapped, ref)[1] > 100.0


def test_two_runs_are_bit_identical():
    for shape in ((64, 3, 9, 17), (128, 2, 9, 17)):
        p, x, _ = _block_case(*shape)
        assert torch.equal(_run_block(p, x)[1], _run_block(p, x)[1])


def _raw_call(x, y, p, C):
    n, _, H, W = x.shape
    return _lib.lib().gencomm_convnext_block_fwd(ptr(x), *[ptr(p[k]) for k in ORDER], ptr(y), n, C, H, W, stream_ptr(DEV))


def test_aliasing_output_is_refused_and_nothing_is_launched():
    p, x, _ = _block_case(64, 2, 8, 8)
    pd = {k: v.to(DEV) for k, v in p.items()}
    xd = x.to(DEV)
    before = xd.clone()
    with _lib.kernel_log() as kl:
        rc = _raw_call(xd, xd, pd, 64)
        rc_overlap = _raw_call(xd, xd.view(-1)[64:], pd, 64)      # a partial overlap is an alias too
    torch.cuda.synchronize()
    assert rc == 1 and rc_overlap == 1 and "alias" in _lib.lib().gencomm_last_error().decode()
    assert not kl.counts and torch.equal(xd, before)


def test_unsupported_width_is_refused():
    x = torch.zeros(1, 32, 4, 4, device=DEV)
    p = {k: torch.zeros(s, device=DEV) for k, s in R.block_shapes(32).items()}
    with _lib.kernel_log() as kl:
        rc = _raw_call(x, torch.empty_like(x), p, 32)
    assert rc == -1 and not kl.counts
    msg = _lib.lib().gencomm_last_error().decode()
    assert "C must be 64 or 128" in msg and "32" in msg


def _module(name):
    if ("module", name) not in _cache:
        cls, cfg, sd, x = R.case_data(name, int(GOLD[f"{name}/seed"]))
        mod = {"Adapter": Adapter, "Reverter": Reverter}[cls](cfg)
        mod.load_state_dict(sd, strict=True)
        _cache[("module", name)] = (mod.to(DEV).eval(), cfg, sd, x)
    return _cache[("module", name)]


@pytest.mark.parametrize("name", list(R.CASES))
def test_modules_against_the_references_float64(name):
    mod, cfg, sd, x = _module(name)
    ref = torch.from_numpy(GOLD[f"{name}/out64"])
    with torch.no_grad():
        y = mod(x.to(DEV))
    assert y.shape == ref.shape and y.dtype == torch.float32
    ok, worst = R.within(y.cpu(), ref)
    print(f"{name}: worst |d| / (1e-5 + 1e-4 |ref|) = {worst:.3f} (the reference's own float32: {float(GOLD[name + '/ref32_ratio']):.3f})")
    assert ok, worst


def test_adapterconvnext_launches():
    """1x1 convolution, one launch per block, 1x1 convolution; the module re-prepares when a parameter changes."""
    mod, cfg, sd, x = _module("cnx64")
    xd = x.to(DEV)
    with torch.no_grad():
        y0 = mod(xd)
        with _lib.kernel_log() as kl:
            mod(xd)
        assert kl.counts.get("convnext_block_kernel<64>") == 3
        gamma = mod.adapter.conv.model[0].gamma
        gamma.mul_(2.0)
        y1 = mod(xd)
        gamma.mul_(0.5)
        assert not torch.equal(y0, y1) and torch.equal(mod(xd), y0)


def test_adapter_then_reverter():
    """The adapter's output straight into a reverter (parameters at R.STD_CHAIN: see there), against the float64 chain."""
    a = _module("cnx64")[0]
    if "chain" not in _cache:
        c = R.chain_data(int(GOLD["cnx64/seed"]), int(GOLD["rev64/seed"]))
        r = Reverter(c[2])
        r.load_state_dict(c[3], strict=True)
        _cache["chain"] = (r.to(DEV).eval(), c[4], R.chain_forward(*c, torch.float64))
    r, x, ref = _cache["chain"]
    with torch.no_grad():
        y = r(a(x.to(DEV)))
    ok, worst = R.within(y.cpu(), ref)
    print(f"adapter -> reverter: worst |d| / (1e-5 + 1e-4 |ref|) = {worst:.3f}")
    assert ok, worst


def test_identity_returns_its_input():
    mod, _, _, x = _module("identity")
    xd = x.to(DEV)
    with torch.no_grad():
        y = mod(xd)
    assert torch.equal(y, xd) and torch.equal(y.cpu().double(), torch.from_numpy(GOLD["identity/out64"]))


def test_cpu_tensor_is_refused():
    for name in ("cnx64", "identity", "conv"):
        mod, _, _, x = _module(name)
        with torch.no_grad(), pytest.raises(_lib.GenCommHipError):
            mod(x)
