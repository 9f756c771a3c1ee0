"""HEAL's PyramidFusion, CPU side: the torch restatement (tests/pyramid_restatement.py) against the fixture the reference's OWN module
produced (tests/golden/pyramid.npz; tools/make_golden_pyramid.py), the checkpoint keys, the crop rectangles of the host against the
reference's mask, the refusals, the three C-ABI entries and the absence of a baseline shell."""
import ctypes
import json
import os
import pkgutil
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import pyramid_restatement as R
from helpers import GOLDEN, assert_close, load_case

REPO = os.path.dirname(os.path.dirname(GOLDEN))


@pytest.fixture(scope="module")
def g():
    return load_case("pyramid")


@pytest.fixture(scope="module")
def model64(g):
    assert int(g["seed"]) == R.SEED
    return R.fill_params_(R.PyramidRestatement(R.cfg()).double().eval())


def test_fixture_conditions(g):
    """The margin shares are conditions of the fixture: none in the strict case, at most 1e-3 anywhere; the stored masks are the rule's."""
    assert float(g["collab_share"]) == 0.0 and float(g["crop_share"]) <= R.MARGIN_CAP and float(g["fuse_share"]) <= R.MARGIN_CAP
    assert not any(g[f"collab_margin_{i}"].any() for i in range(3))
    fx, fs = R.fuse_inputs()
    assert np.array_equal(fx, g["fuse_x"]) and np.array_equal(fs, g["fuse_score"])
    assert np.array_equal(R.margin_mask(fs, R.FUSE["record_len"], g["collab_affine"]).numpy(), g["fuse_margin"])
    assert (fs[1:] == 0).any() and (fs > 0).any()
    # the cases the fixture must contain: a lone agent under a non-identity matrix, an agent entirely outside the map
    aff = g["collab_affine"]
    assert [int(v) for v in g["collab_record_len"]] == [1, 4]
    assert not np.array_equal(aff[0, 0, 0], np.array([[1.0, 0, 0], [0, 1.0, 0]])) and abs(aff[1, 0, 3, 0, 2]) > 4.0
    dark = (g["collab_level64_0"][0] == 0).all(0)
    assert 0 < dark.sum() < dark.size                                  # pixels nobody sees are exactly 0, the others are not
    assert g["collab_x"].dtype == np.float32 and g["collab_out64"].dtype == np.float64


def test_restatement_reproduces_the_reference(g, model64):
    aff = torch.from_numpy(g["collab_affine"])
    rl = [int(v) for v in g["collab_record_len"]]
    with torch.no_grad():
        levels = []
        out, occ = model64.forward_collab(torch.from_numpy(g["collab_x"]).double(), rl, aff, levels=levels)
        assert_close(out.numpy(), g["collab_out64"], 1e-11, 1e-12, "collab out")
        for i in range(3):
            assert_close(occ[i].numpy(), g[f"collab_occ64_{i}"], 1e-11, 1e-12, f"collab occ {i}")
            assert_close(levels[i][2].numpy(), g[f"collab_level64_{i}"], 1e-11, 1e-12, f"collab level {i}")
            assert np.array_equal(levels[i][2].numpy() == 0, g[f"collab_level64_{i}"] == 0)
        c = R.CROP
        out, occ = model64.forward_collab(torch.from_numpy(g["crop_x"]).double(), c["record_len"], torch.from_numpy(g["crop_affine"]),
                                          c["modalities"], c["info"])
        assert_close(out.numpy(), g["crop_out64"], 1e-11, 1e-12, "crop out")
        for i in range(3):
            assert_close(occ[i].numpy(), g[f"crop_occ64_{i}"], 1e-11, 1e-12, f"crop occ {i}")
        out, occ = model64.forward_single(torch.from_numpy(g["collab_x"][:1]).double())
        assert_close(out.numpy(), g["single_out64"], 1e-11, 1e-12, "single out")
        for i in range(3):
            assert_close(occ[i].numpy(), g[f"single_occ64_{i}"], 1e-11, 1e-12, f"single occ {i}")
        out = R.weighted_fuse(torch.from_numpy(g["fuse_x"]).double(), torch.from_numpy(g["fuse_score"]).double(), R.FUSE["record_len"], aff)
        assert_close(out.numpy(), g["fuse_out64"], 1e-12, 1e-13, "weighted_fuse")


def test_state_dict_keys_are_the_references():
    from gencomm_amd import PyramidFusion
    with open(os.path.join(GOLDEN, "pyramid_keys.json")) as f:
        want = json.load(f)
    assert want["model_cfg"] == R.cfg()
    for model in (PyramidFusion(R.cfg()), R.PyramidRestatement(R.cfg())):
        assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == want["state_dict"]
    m = PyramidFusion(R.cfg())
    assert m.num_levels == 3 and all(isinstance(getattr(m, f"single_head_{i}"), nn.Conv2d) for i in range(3))
    assert [m.resnet.layer0[0].conv2.groups, m.resnet.layer1[0].conv2.in_channels, m.resnet.layer2[0].conv2.in_channels] == [32, 256, 512]
    with pytest.raises(KeyError):                        # the reference indexes model_cfg["resnext"]
        PyramidFusion({k: v for k, v in R.cfg().items() if k != "resnext"})
    plain = PyramidFusion(R.cfg(resnext=False))
    assert [k for k, _ in plain.state_dict().items()] == [k for k, _ in R.PyramidRestatement(R.cfg(resnext=False)).state_dict().items()]
    assert "resnet.layer0.0.conv3.weight" not in plain.state_dict()


def _mask_of(rects, H, W):
    m = np.ones((len(rects), 1, H, W), bool)
    for j, (h0, h1, w0, w1) in enumerate(rects):
        if h0 < 0:
            continue
        m[j] = False
        m[j, :, h0:h1, w0:w1] = True
    return m


def test_crop_rectangles_equal_the_references_mask(g):
    from gencomm_amd.pyramid_fuse import NO_RECT, crop_rect, crop_rects
    c = R.CROP
    for i in range(3):
        ref = g[f"crop_mask_{i}"]
        H, W = ref.shape[2:]
        rects = crop_rects(H, W, c["modalities"], c["info"])
        assert rects[0] == NO_RECT and rects[3] == NO_RECT
        assert np.array_equal(_mask_of(rects, H, W), ref), i
        assert np.array_equal(R.crop_mask(H, W, c["modalities"], c["info"]).numpy(), ref), i
    assert g["crop_mask_0"][1].sum() == 4 and g["crop_mask_0"][2].sum() == 64 and g["crop_mask_2"][1:3].sum() == 0
    # Python's slice semantics, beyond what the fixture holds: a ratio below 1 makes the start negative (it counts from the end), an
    # odd size, an empty range; against the reference's own expression on a numpy array
    for H, W, rh, rw in ((8, 12, 0.5, 0.5), (9, 13, 0.7, 2), (16, 24, 2, 2), (5, 7, 1, 0.9), (100, 252, 2, 1), (2, 3, 1, 1), (32, 32, 0.25, 3)):
        info = {"m2": {"crop_ratio_H_m2": rh, "crop_ratio_W_m2": rw}}
        want = R.crop_mask(H, W, ["m2"], info).numpy()
        h0, h1, w0, w1 = crop_rect(H, W, rh, rw)
        assert 0 <= h0 <= h1 <= H and 0 <= w0 <= w1 <= W
        assert np.array_equal(_mask_of([(h0, h1, w0, w1)], H, W), want), (H, W, rh, rw)


def test_refusals_name_what_they_refuse():
    from gencomm_amd import PyramidFusion, weighted_fuse
    from gencomm_amd.bev_backbone import gconv3x3_check
    with pytest.raises(NotImplementedError, match="align_corners"):
        PyramidFusion(dict(R.cfg(), align_corners=True))
    with pytest.raises(NotImplementedError, match="align_corners"):
        weighted_fuse(torch.zeros(1, 2, 4, 4), torch.ones(1, 1, 4, 4), [1], torch.zeros(1, 1, 1, 2, 3), True)
    for groups, c in ((32, 64), (32, 1024), (16, 128), (4, 64)):
        with pytest.raises(NotImplementedError, match="unsupported group width"):
            gconv3x3_check(nn.Conv2d(c, c, 3, padding=1, groups=groups))
    assert [gconv3x3_check(nn.Conv2d(32 * k, 32 * k, 3, stride=s, padding=1, groups=32)) for k in (4, 8, 16) for s in (1, 2)] == [4, 4, 8, 8, 16, 16]
    with pytest.raises(NotImplementedError, match="dilation"):
        gconv3x3_check(nn.Conv2d(128, 128, 3, padding=2, dilation=2, groups=32))
    x, aff = torch.zeros(1, 64, 8, 12), torch.zeros(1, 1, 1, 2, 3, dtype=torch.float64)
    m = PyramidFusion(R.cfg())
    assert m.training
    for call in (lambda: m.forward_single(x), lambda: m.forward_collab(x, [1], aff)):
        with pytest.raises(NotImplementedError, match=r"train\(\)"):
            call()
    m.eval()
    for call in (lambda: m.forward_single(x), lambda: m.forward_collab(x, [1], aff)):
        with pytest.raises(NotImplementedError, match="pyramid training"):
            call()
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="pyramid training"):
        m.forward_single(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="pyramid training"):
        weighted_fuse(x.clone().requires_grad_(True), torch.ones(1, 1, 8, 12), [1], aff, False)


def test_entries_are_declared_and_exported():
    from gencomm_amd import _lib
    with open(os.path.join(REPO, "include", "gencomm_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    want = {"gencomm_gconv3x3_fwd": 13, "gencomm_pyramid_score_fwd": 11, "gencomm_warp_weightfuse_fwd": 11, "gencomm_gconv3x3_prepare": 4}
    for name, nargs in want.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert _lib.ABI_VERSION == 12                        # additive entries: the ABI version stays
    assert os.path.exists(os.path.join(_lib.CSRC_DIR, "pyramid_kernels.h"))


def test_no_baseline_shell_module():
    import gencomm_amd
    names = {m.name for m in pkgutil.iter_modules(gencomm_amd.__path__)}
    assert "pyramid_fuse" in names
    assert not names & {"heter_pyramid_collab", "heter_pyramid_single", "point_pillar_pyramid_loss"}
