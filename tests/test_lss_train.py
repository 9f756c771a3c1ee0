"""Training the Lift-Splat-Shoot camera encoder, CPU side: the new entries of the C ABI and their argument checks, the depth term of the
criteria in its composed form against tests/golden/lss_train.npz (made by tools/make_golden_lss_train.py from the reference's own
LiftSplatShoot in .train() mode and its FocalLoss), the refusals, the resolver name of PointPillarDepthLoss, and the opt-in switch of
LiftSplatShoot. No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lss_restatement import small_args

from gencomm_amd import _lib, synth
from gencomm_amd.lift_splat_shoot import LiftSplatShoot
from gencomm_amd.point_pillar_gencomm_loss import PointPillarGencommLoss, depth_focal_loss, depth_term

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_ENTRIES = ("gencomm_lss_splat_bwd_workspace_bytes", "gencomm_lss_splat_bwd", "gencomm_maxpool3x3s2_bwd",
                 "gencomm_stem7x7_wgrad_scratch_floats", "gencomm_stem7x7_wgrad", "gencomm_depth_focal_loss")
LOSS_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz")


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lss.npz"))


@pytest.fixture(scope="module")
def gt(golden_dir):
    return np.load(os.path.join(golden_dir, "lss_train.npz"))


def test_training_entries_in_header_binding_and_library():
    txt = open(os.path.join(REPO, "include", "gencomm_hip.h")).read()
    raw = ctypes.CDLL(_lib.build())
    for name in TRAIN_ENTRIES:
        assert name + "(" in txt and name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert "#define GENCOMM_ABI_VERSION 12" in txt and _lib.ABI_VERSION == 12 and raw.gencomm_abi_version() == 12


def test_training_entries_reject_bad_arguments_with_status_codes():
    _lib.build()
    l = _lib.lib()
    err = lambda: l.gencomm_last_error()
    nx = (ctypes.c_int * 3)(256, 256, 1)
    p = ctypes.c_void_p(16)   # never dereferenced: the argument checks fail first
    # workspace size of the backward: the cell-major copy of grad_out
    assert l.gencomm_lss_splat_bwd_workspace_bytes(4, 128, nx) == 4 * 256 * 256 * 128 * 4
    assert l.gencomm_lss_splat_bwd_workspace_bytes(0, 128, nx) == -1 and b"bad B" in err()
    assert l.gencomm_lss_splat_bwd_workspace_bytes(4, 128, None) == -1
    assert l.gencomm_lss_splat_bwd_workspace_bytes(4, 128, (ctypes.c_int * 3)(256, 0, 1)) == -1
    # gencomm_lss_splat_bwd(grad_out, fwd_ws, fwd_ws_bytes, cell, nx3, B, N, D, fH, fW, C, d_logit, d_feat, ws, ws_bytes, stream)
    ok = [p, p, 1 << 40, p, nx, 1, 1, 48, 8, 16, 16, p, p, p, 1 << 40, None]
    for i in (0, 1, 3, 11, 12, 13):
        a = list(ok)
        a[i] = None
        assert l.gencomm_lss_splat_bwd(*a) == 1 and b"null pointer" in err(), i
    a = list(ok); a[4] = None
    assert l.gencomm_lss_splat_bwd(*a) == 1 and b"null pointer" in err()
    for i in (5, 6, 7, 10):   # B, N, D, C < 1
        a = list(ok)
        a[i] = 0
        assert l.gencomm_lss_splat_bwd(*a) == 1 and b"bad B" in err(), i
    a = list(ok); a[4] = (ctypes.c_int * 3)(256, 0, 1)
    assert l.gencomm_lss_splat_bwd(*a) == 1 and b"bad grid" in err()
    a = list(ok); a[7] = 257
    assert l.gencomm_lss_splat_bwd(*a) == 1 and b"256 depth bins" in err()
    a = list(ok); a[2] = 1024
    assert l.gencomm_lss_splat_bwd(*a) == 2 and b"forward workspace too small" in err()
    a = list(ok); a[14] = 1024
    assert l.gencomm_lss_splat_bwd(*a) == 2 and b"gencomm_lss_splat_bwd_workspace_bytes" in err()
    # max-pool backward
    assert l.gencomm_maxpool3x3s2_bwd(None, p, p, 1, 64, 32, 32, None) == 1 and b"null pointer" in err()
    assert l.gencomm_maxpool3x3s2_bwd(p, p, None, 1, 64, 32, 32, None) == 1
    assert l.gencomm_maxpool3x3s2_bwd(p, p, p, 1, 0, 32, 32, None) == 1 and b"bad dims" in err()
    # stem weight gradient
    assert l.gencomm_stem7x7_wgrad_scratch_floats(16, 3, 336, 448, 64) == 512 * 64 * 147
    assert l.gencomm_stem7x7_wgrad_scratch_floats(2, 3, 16, 20, 64) == ((2 * 8 * 10 + 31) // 32) * 64 * 147
    assert l.gencomm_stem7x7_wgrad_scratch_floats(2, 4, 16, 20, 64) == -1 and b"bad dims" in err()
    assert l.gencomm_stem7x7_wgrad_scratch_floats(2, 3, 16, 20, 48) == -1
    assert l.gencomm_stem7x7_wgrad(None, p, p, 2, 3, 16, 20, 64, p, 1 << 30, None) == 1 and b"null pointer" in err()
    assert l.gencomm_stem7x7_wgrad(p, p, p, 2, 3, 16, 20, 64, None, 1 << 30, None) == 1
    assert l.gencomm_stem7x7_wgrad(p, p, p, 2, 3, 0, 20, 64, p, 1 << 30, None) == 1 and b"bad dims" in err()
    assert l.gencomm_stem7x7_wgrad(p, p, p, 2, 3, 16, 20, 64, p, 10, None) == 1 and b"scratch smaller" in err()
    # depth focal loss
    assert l.gencomm_depth_focal_loss(None, p, p, p, 4, 48, 8, 16, 0.25, 2.0, 1.0, None) == 1 and b"null pointer" in err()
    assert l.gencomm_depth_focal_loss(p, p, p, None, 4, 48, 8, 16, 0.25, 2.0, 1.0, None) == 1
    assert l.gencomm_depth_focal_loss(p, p, p, p, 4, 0, 8, 16, 0.25, 2.0, 1.0, None) == 1 and b"bad dims" in err()
    assert l.gencomm_depth_focal_loss(p, p, p, p, 4, 48, 8, 16, 0.25, -1.0, 1.0, None) == 1 and b"gamma" in err()


def test_composed_depth_term_equals_the_reference_focal_loss(g, gt):
    """The composed form on CPU tensors is the reference's fp32 operator sequence: on the depth logits of lss.npz it gives the value and
    the gradient that the reference's own FocalLoss(alpha 0.25, gamma 2).mean() gave (focal_eval_* of lss_train.npz) at rtol 1e-5."""
    idx = torch.from_numpy(g["depth_gt_indices"])
    logit = torch.from_numpy(g["depth_logit"]).requires_grad_(True)
    total = depth_term({"depth_items": (logit, idx)}, "", {"weight": 1.0})
    total.backward()
    assert float(total.detach()) == pytest.approx(float(gt["focal_eval_loss"]), rel=1e-5)
    want = gt["focal_eval_grad"]
    np.testing.assert_allclose(logit.grad.numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()))
    # and the closed form of the issue, in float64: -alpha (1 - p_t)^2 log p_t at the target bin
    p = torch.softmax(logit.detach().double(), 1).gather(1, idx[:, None])[:, 0]
    assert float((-0.25 * (1 - p) ** 2 * p.log()).mean()) == pytest.approx(float(gt["focal_eval_loss"]), rel=1e-5)


def test_depth_term_sums_keys_weights_and_suffixes(g):
    idx = torch.from_numpy(g["depth_gt_indices"])
    logit = torch.from_numpy(g["depth_logit"])
    one = float(depth_focal_loss(logit, idx).mean())
    out = {"depth_items": (logit, idx), "depth_items_m4": (logit * 0.5, idx), "depth_items_single": (logit, idx), "cls_preds": None}
    two = float(depth_focal_loss(logit * 0.5, idx).mean())
    assert float(depth_term(out, "", {"weight": 3.0})) == pytest.approx(3.0 * (2 * one + two), rel=1e-6)      # every key with the prefix
    assert float(depth_term(out, "_single", {"weight": 1.0})) == pytest.approx(one, rel=1e-6)
    assert depth_term({"cls_preds": None}, "", {"weight": 1.0}) is None


def test_smooth_target_and_fg_mask_refusals_name_their_key(g):
    out = {"depth_items": (torch.from_numpy(g["depth_logit"]), torch.from_numpy(g["depth_gt_indices"]))}
    for key in ("smooth_target", "use_fg_mask"):
        with pytest.raises(NotImplementedError, match="depth." + key):
            depth_term(out, "", {"weight": 1.0, key: True})
        assert depth_term(out, "", {"weight": 1.0, key: False}) is not None


def _loss_inputs():
    gl = np.load(LOSS_GOLD)
    B, H, W, A, C = (int(v) for v in gl["dims"])
    t = {k: torch.from_numpy(v) for k, v in synth.make_loss_inputs(int(gl["data_seed"]), B, H, W, A, C).items()}
    out = {k: t[k] for k in ("cls_preds", "reg_preds", "dir_preds", "gt_feature", "pred_feature")}
    tgt = {k: t[k] for k in ("pos_equal_one", "neg_equal_one", "targets")}
    return gl, json.loads(str(gl["args"])), out, tgt


def test_gencomm_loss_without_depth_items_is_unchanged():
    """No depth key: head terms + generate_weight * MSE in the operation order of the parent commit, bit for bit, the same loss_dict
    keys, and the reference's values of loss.npz."""
    gl, args, out, tgt = _loss_inputs()
    crit = PointPillarGencommLoss(args)
    total = crit(dict(out), tgt)
    assert set(crit.loss_dict) == {"reg_loss", "cls_loss", "dir_loss", "generate_loss", "total_loss"}
    heads = PointPillarGencommLoss(args)._head_terms(dict(out), tgt, "")
    want = heads + args["generate_weight"] * F.mse_loss(out["gt_feature"], out["pred_feature"])
    assert torch.equal(total, want) and torch.equal(crit.loss_dict["total_loss"], want)
    assert float(total) == pytest.approx(float(gl["total"]), rel=2e-6)
    for k in ("reg_loss", "cls_loss", "dir_loss", "generate_loss"):
        assert float(crit.loss_dict[k]) == pytest.approx(float(gl[k]), rel=2e-6, abs=1e-7), k


def test_gencomm_loss_with_depth_items_adds_the_term_once(g):
    gl, args, out, tgt = _loss_inputs()
    item = (torch.from_numpy(g["depth_logit"]).requires_grad_(True), torch.from_numpy(g["depth_gt_indices"]))
    crit = PointPillarGencommLoss(dict(args, depth={"weight": 2.0}))
    total = crit(dict(out, depth_items=item), tgt)
    depth = 2.0 * float(depth_focal_loss(item[0].detach(), item[1]).mean())
    assert float(total) == pytest.approx(float(gl["total"]) + depth, rel=2e-6)
    assert float(crit.loss_dict["depth_loss"]) == pytest.approx(depth, rel=1e-6)
    assert float(crit.loss_dict["total_loss"]) == pytest.approx(float(total), rel=1e-7)   # the gencomm criterion re-logs the final total
    total.backward()
    assert item[0].grad is not None and float(item[0].grad.abs().max()) > 0
    d = crit.logging(0, 0, 1)
    assert d["depth_loss"] == pytest.approx(depth, rel=1e-6)


def test_point_pillar_depth_loss_resolves_by_name_and_omits_the_generation_term(g):
    import gencomm_amd
    import gencomm_amd.point_pillar_depth_loss as m
    # train_utils.create_loss: module `point_pillar_depth_loss`, class whose lower-cased name is the module name without underscores
    assert [n for n in dir(m) if n.lower() == "pointpillardepthloss"] == ["PointPillarDepthLoss"]
    assert gencomm_amd.PointPillarDepthLoss is m.PointPillarDepthLoss and "PointPillarDepthLoss" in gencomm_amd.__all__
    gl, args, out, tgt = _loss_inputs()
    args = {k: v for k, v in args.items() if k != "generate_weight"}
    with pytest.raises(KeyError):
        m.PointPillarDepthLoss({k: v for k, v in args.items() if k != "depth"})
    crit = m.PointPillarDepthLoss(dict(args, depth={"weight": 1.0}))
    item = (torch.from_numpy(g["depth_logit"]), torch.from_numpy(g["depth_gt_indices"]))
    heads_only = {k: v for k, v in out.items() if k not in ("gt_feature", "pred_feature")}
    total = crit(dict(heads_only, depth_items=item), tgt)
    heads = float(gl["reg_loss"]) + float(gl["cls_loss"]) + float(gl["dir_loss"])
    depth = float(depth_focal_loss(*item).mean())
    assert float(total) == pytest.approx(heads + depth, rel=2e-6)
    assert "generate_loss" not in crit.loss_dict
    assert float(crit.loss_dict["depth_loss"]) == pytest.approx(depth, rel=1e-6)
    assert float(crit.loss_dict["total_loss"]) == pytest.approx(heads, rel=2e-6)   # point_pillar_depth_loss.py:56-57: logged without the depth term
    assert crit.logging(0, 0, 1)["depth_loss"] == pytest.approx(depth, rel=1e-6)


def test_trainable_switch_on_cpu_inputs(g):
    inp = {k: torch.from_numpy(g[k].astype(np.float32)) for k in ("imgs", "rots", "trans", "intrins", "post_rots", "post_trans")}
    m = LiftSplatShoot(small_args(), trainable=True)
    with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):
        m({"inputs_m4": inp}, "m4")
    with pytest.raises(NotImplementedError, match="inference only"):
        LiftSplatShoot(small_args(), trainable=False)({"inputs_m4": inp}, "m4")
    # the constructor's refusals are those of the default
    for key, value, text in (("camera_encoder", "EfficientNet", "camera_encoder: EfficientNet"), ("use_depth_gt", True, "use_depth_gt")):
        with pytest.raises(NotImplementedError, match=text):
            LiftSplatShoot(dict(small_args(), **{key: value}), trainable=True)


def test_stem_input_gradient_refusal_names_the_layer():
    from gencomm_amd.bev_backbone import _conv_backward
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    with pytest.raises(NotImplementedError, match=r"7x7 stride-2 pad-3 stem \(Conv2d 3 -> 64"):
        _conv_backward(torch.zeros(1, 3, 16, 16), torch.zeros(1, 64, 8, 8), conv, None, True)


def test_fixture_holds_what_the_gpu_test_needs(gt):
    for k in ("loss_bev", "loss_depth", "d_depth_logit", "d_feat", "grad__conv1.weight", "grad__bn1.weight", "grad__layer1.0.conv2.weight",
              "grad__layer2.0.downsample.0.weight", "grad__layer2.3.bn3.bias", "grad__depth_head.weight", "grad__depth_head.bias",
              "grad__image_head.weight", "stat__bn1.running_mean", "stat__bn1.running_var", "stat__layer2.3.bn3.running_mean",
              "stat__layer2.3.bn3.running_var"):
        assert k in gt.files and "e_ref__" + k in gt.files and np.isfinite(gt[k]).all() and 0 <= float(gt["e_ref__" + k]) < 1e-2, k
    assert tuple(gt["d_depth_logit"].shape) == (4, 48, 8, 16) and tuple(gt["d_feat"].shape) == (4, 8, 8, 16)
