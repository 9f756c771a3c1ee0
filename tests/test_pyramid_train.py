"""Training HEAL's PyramidFusion, the part that needs no GPU: the float64 restatement reproduces every number of the reference's step
(tests/golden/pyramid_train_*.npz) to 1e-10, the fixtures satisfy their own conditions (empty margin masks, file sizes, consistent
sample metadata), the trainable module keeps the reference's state_dict keys, the new entries are declared, and ``trainable=True``
objects on CPU tensors fail with the usual no-CPU-fallback error."""
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
import pyramid_train_restatement as TR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"gencomm_gconv3x3_prepare_t": 4, "gencomm_gconv3x3_dgrad": 13, "gencomm_gconv3x3_wgrad_fixed_scratch_floats": 5,
           "gencomm_gconv3x3_wgrad_fixed": 12, "gencomm_pyramid_score_bwd_scratch_floats": 4, "gencomm_pyramid_score_bwd": 16,
           "gencomm_warp_weightfuse_bwd_scratch_floats": 3, "gencomm_warp_weightfuse_bwd": 15}


@pytest.fixture(scope="module")
def steps():
    """One float64 restatement step per case, computed once."""
    return {name: TR.run_case(TR.restatement(), name, torch.float64) for name in TR.CASES}


@pytest.mark.parametrize("name", list(TR.CASES))
def test_restatement_reproduces_the_reference_step(name, steps):
    store, _ = TR.fixture(name)
    got = steps[name]
    worst = {"loss": abs(float(got["loss"]) - float(store["loss"])) / abs(float(store["loss"])), "dx": TR.check_summary(store, "dx", got["dx"])}
    for i, o in enumerate(got["occs"]):
        worst[f"occ_{i}"] = TR.check_summary(store, f"occ_{i}", o)
    stored_grads = {k[5:].split("#")[0] for k in store if k.startswith("grad/")}
    assert stored_grads == set(got["grads"]), (sorted(stored_grads ^ set(got["grads"])))
    for k, g in got["grads"].items():
        worst["grad/" + k] = TR.check_summary(store, "grad/" + k, g)
    for k in store:
        if k.startswith("stat/"):
            worst[k] = TR.check_summary(store, k, got["stats"][k[5:]])
    key = max(worst, key=worst.get)
    print(f"{name}: {len(worst)} tensors, worst {key}: {worst[key]:.2e}")
    assert worst[key] <= 1e-10, (key, worst[key])
    mode, frozen, _ = TR.CASES[name]
    assert frozen == (len(got["grads"]) == 0)
    assert (mode == "train") == any(k.startswith("stat/") for k in store)


@pytest.mark.parametrize("name", list(TR.CASES))
def test_fixture_conditions(name):
    store, paths = TR.fixture(name)
    for p in paths:
        assert os.path.getsize(p) <= TR.FILE_LIMIT <= os.path.getsize(os.path.join(TR.GOLDEN, "pyramid.npz")), p
    assert store["dx"].dtype == np.float64 and store["dx"].shape == TR.case_inputs(name)[0].shape
    for k in store:
        if k.endswith("#meta"):
            size, stride, total, norm = store[k]
            assert size > TR.SAMPLE_ABOVE and stride == size // TR.SAMPLES and store[k[:-5] + "#sample"].shape == (TR.SAMPLES,), k
            assert np.isfinite(total) and norm > 0, k
        if k.startswith("e32/"):
            assert 0 <= float(store[k]) < 1e-2, (k, float(store[k]))      # a float32 step (one crossed ReLU kink moves a tensor by ~1e-3), not a broken one
    if TR.CASES[name][2] == "collab":
        # the condition of the gradient cases, recomputed from the restatement's own float64 scores: no marked pixel at any level
        model = TR.restatement()
        if TR.CASES[name][0] == "train":
            for m in model.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.momentum = 0.0
        scores, rl, aff = TR.level_scores(model, name)
        for i, s in enumerate(scores):
            mask = R.margin_mask(s, rl, aff).numpy()
            assert not mask.any() and not store[f"margin_{i}"].any(), (name, i, int(mask.sum()))
        if name == "frozen":
            assert any(bool((s == 0).any()) for s in scores)              # the crop mask is on


@pytest.mark.parametrize("key,kw,shape", [("basic", dict(resnext=False), TR.SMALL), ("ego", dict(), TR.EGO)])
def test_steps_without_a_fixture_stay_clear_of_relu_kinks(key, kw, shape):
    """The condition of the two module steps the GPU tests compare without a fixture, from the float64 restatement alone."""
    with TR.relu_margin() as m:
        TR.run_case(TR.restatement(torch.float64, **kw), "train", torch.float64, **shape)
    print(f"{key}: smallest |ReLU input| / rms = {m.worst:.3e}")
    assert m.worst >= TR.KINK_MARGIN


def test_trainable_module_keeps_the_state_dict_keys():
    from gencomm_amd.bev_backbone_resnet import Bottleneck
    from gencomm_amd.pyramid_fuse import PyramidFusion
    with open(os.path.join(TR.GOLDEN, "pyramid_keys.json")) as f:
        want = json.load(f)
    model = PyramidFusion(want["model_cfg"], input_channels=64, trainable=True)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == want["state_dict"]
    blocks = [m for m in model.modules() if isinstance(m, Bottleneck)]
    assert blocks and all(m.trainable is True for m in blocks)
    assert all(m.trainable is False for m in PyramidFusion(want["model_cfg"]).modules() if isinstance(m, Bottleneck))
    with pytest.raises(NotImplementedError, match="align_corners"):
        PyramidFusion(dict(want["model_cfg"], align_corners=True), trainable=True)


def test_new_entries_are_declared_and_exported():
    from gencomm_amd import _lib
    with open(os.path.join(REPO, "include", "gencomm_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES.items():
        decl = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert _lib.ABI_VERSION == 12
    assert os.path.exists(os.path.join(_lib.CSRC_DIR, "pyramid_bwd_kernels.h"))


def test_entries_refuse_what_is_outside_their_domain():
    """Status codes before any launch: no device is needed to see them."""
    from gencomm_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert l.gencomm_gconv3x3_wgrad_fixed_scratch_floats(1, 5, 8, 8, 1) == -1 and b"group width" in l.gencomm_last_error()
    assert l.gencomm_gconv3x3_wgrad_fixed_scratch_floats(2, 16, 9, 35, 2) > 0
    assert l.gencomm_gconv3x3_dgrad(p, p, p, p, p + 64, None, 1, 128, 4, 8, 8, 2, None) == 1 and b"spread" in l.gencomm_last_error()
    assert l.gencomm_gconv3x3_dgrad(p, p, p, p, p, None, 1, 128, 4, 8, 8, 1, None) == 1 and b"alias" in l.gencomm_last_error()
    assert l.gencomm_gconv3x3_wgrad_fixed(p, p, p, 1, 128, 4, 8, 8, 1, p, 1, None) == 2 and b"scratch" in l.gencomm_last_error()
    assert l.gencomm_pyramid_score_bwd(p, p, p, None, None, None, p, None, None, 1, 4, 2, 2, None, 0, None) == 1 and b"d_occ" in l.gencomm_last_error()
    assert l.gencomm_pyramid_score_bwd(p, p, p, None, p, None, None, p, p, 1, 4, 2, 2, p, 1, None) == 2 and b"scratch" in l.gencomm_last_error()
    assert l.gencomm_warp_weightfuse_bwd(p, p, p, p, p, p, p, p, 1, 1, 1, 4, 2, 2, None) == 2 and b"scratch" in l.gencomm_last_error()
    assert l.gencomm_warp_weightfuse_bwd(p, p, p, p, p, p, None, p, 64, 1, 1, 4, 2, 2, None) == 1 and b"null" in l.gencomm_last_error()


def test_no_shell_or_loss_module_is_added():
    import gencomm_amd
    names = {m.name for m in pkgutil.iter_modules(gencomm_amd.__path__)}
    assert {"pyramid_fuse", "pyramid_bwd"} <= names
    assert not names & {"heter_pyramid_collab", "heter_pyramid_single", "point_pillar_pyramid_loss"}


def test_trainable_objects_need_a_gpu():
    """On CPU tensors the opt-in objects fail as everything else does (no CPU fallback), not with a refusal about training."""
    from gencomm_amd._lib import GenCommHipError
    from gencomm_amd.bev_backbone import gconv3x3_hip
    from gencomm_amd.pyramid_fuse import PyramidFusion, score_head, weighted_fuse
    x = torch.zeros(1, 128, 4, 4, requires_grad=True)
    conv, bn = nn.Conv2d(128, 128, 3, padding=1, groups=32, bias=False), nn.BatchNorm2d(128)
    with pytest.raises(GenCommHipError, match="no CPU fallback"):
        gconv3x3_hip(x, conv, bn, True, trainable=True)
    with pytest.raises(GenCommHipError, match="no CPU fallback"):
        score_head(torch.zeros(1, 64, 4, 4, requires_grad=True), nn.Conv2d(64, 1, 1), trainable=True)
    aff = torch.from_numpy(R.affine_of([[R.theta(4, 4)]], L=5))
    with pytest.raises(GenCommHipError, match="no CPU fallback"):
        weighted_fuse(torch.zeros(1, 8, 4, 4, requires_grad=True), torch.ones(1, 1, 4, 4), [1], aff, False, trainable=True)
    model = PyramidFusion(R.cfg(), trainable=True).train()
    with pytest.raises(GenCommHipError, match="no CPU fallback"):
        model.forward_single(torch.zeros(1, 64, 8, 8, requires_grad=True))
    with pytest.raises(NotImplementedError, match="pyramid training"):     # the default keeps its refusal
        weighted_fuse(torch.zeros(1, 8, 4, 4, requires_grad=True), torch.ones(1, 1, 4, 4), [1], aff, False)
