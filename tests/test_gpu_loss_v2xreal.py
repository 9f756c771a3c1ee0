"""V2X-Real training criteria on the GPU: the two-launch head terms of the library (gencomm_head_loss_mc, csrc/loss_kernels.h) against the
reference's own criteria (tests/golden/loss_v2xreal.npz), against the framework-operator composition on edge cases, for determinism,
and end to end behind a stage-1 shell with num_class 3 in train mode."""
import json
import math

import numpy as np
import pytest
import torch

from gencomm_amd import synth
from gencomm_amd.point_pillar_v2xreal_gencomm_loss import PointPillarV2XRealGenCommLoss
from gencomm_amd.point_pillar_v2xreal_loss import PointPillarV2XRealLoss
from test_loss_v2xreal import CASES, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARGS = {"cls_weight": 1.0, "reg": 2.0, "num_class": 3, "generate_weight": 1}


def _took_fused_path(total):
    """True when the autograd graph of `total` holds the library's Function."""
    todo, seen = [total.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if "HeadLossMcFn" in type(f).__name__:
            return True
        todo.extend(n for n, _ in f.next_functions)
    return False


@pytest.mark.parametrize("crit_name", ["stage2", "gencomm"])
@pytest.mark.parametrize("tag", CASES)
def test_fused_matches_the_reference_criteria(tag, crit_name):
    _, total = run_case(tag, crit_name, DEV, fuse=True)
    assert _took_fused_path(total)


def _inputs(case):
    B, H, W, R, K = 2, 64, 128, 2, 3
    if case == "k1":
        K = 1
    dtype = np.float32 if case == "float32" else np.float64
    t = synth.make_loss_inputs_v2xreal(11 + len(case), B, H, W, R, K, C=16, nan_frac=0.3 if case == "nan" else 0.0, dtype=dtype)
    lab = t["pos_equal_one"]
    if case == "all_ignored":
        lab[1] = -1
    if case == "no_positives":
        lab[0][lab[0] > 0] = 0
    if case == "label_not_block":   # class values that differ from the slot's class block
        pos = lab > 0
        lab[pos] = np.random.RandomState(5).randint(1, K + 1, int(pos.sum()))
        assert (lab[pos] != (np.nonzero(pos)[3] // R + 1)).mean() > 0.5
    t = {k: torch.from_numpy(v).to(DEV) for k, v in t.items()}
    if case == "noncontiguous":
        t["cls_preds"] = t["cls_preds"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # NHWC storage, NCHW view
        assert not t["cls_preds"].is_contiguous()
    return t, K


def _run(crit_cls, args, t, fused):
    crit = crit_cls(args)
    crit.fuse_heads = fused
    leaves = {k: t[k].detach().clone().requires_grad_(True) for k in ("cls_preds", "reg_preds", "pred_feature")}
    assert leaves["cls_preds"].stride() == t["cls_preds"].stride()   # clone keeps the storage order
    total = crit(dict(leaves, gt_feature=t["gt_feature"]), {"pos_equal_one": t["pos_equal_one"], "targets": t["targets"]})
    total.backward()
    assert _took_fused_path(total) == fused
    return total, {k: v for k, v in crit.loss_dict.items()}, {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("case", ["shipped", "all_ignored", "no_positives", "nan", "k1", "label_not_block", "float32", "noncontiguous"])
def test_fused_equals_the_operator_composition(case):
    """Bars of tests/test_loss.py::test_one_launch_head_loss_equals_the_operator_composition; the shipped stage-1 shape (2 x 64 x 128,
    S = 6, K = 3, float64 labels / targets) and its edge cases."""
    t, K = _inputs(case)
    args = dict(ARGS, num_class=K)
    res = {f: _run(PointPillarV2XRealGenCommLoss, args, t, f) for f in (True, False)}
    assert res[True][0].dtype == res[False][0].dtype == (torch.float32 if case == "float32" else torch.float64)
    assert float(res[True][0].detach()) == pytest.approx(float(res[False][0].detach()), rel=3e-6)
    assert set(res[True][1]) == set(res[False][1])
    for k, v in res[False][1].items():
        assert float(res[True][1][k]) == pytest.approx(float(v), rel=3e-6, abs=1e-7), k
    for k, gr in res[False][2].items():
        assert torch.isfinite(res[True][2][k]).all(), k
        scale = float(gr.abs().max()) + 1e-30
        assert float((res[True][2][k] - gr).abs().max()) <= 2e-5 * scale, k
    if case == "all_ignored":   # weight 0 everywhere in the ignored sample
        assert float(res[True][2]["cls_preds"][1].abs().max()) == 0.0 and float(res[True][2]["reg_preds"][1].abs().max()) == 0.0
    if case == "nan":           # a NaN target contributes neither loss nor gradient
        tgt = t["targets"]
        nan = torch.isnan(tgt) & (t["pos_equal_one"] > 0)[..., None]
        assert bool(nan.any())
        B, H, W, S, _ = tgt.shape
        g = res[True][2]["reg_preds"].view(B, S, 7, H, W).permute(0, 3, 4, 1, 2)
        assert float(g[nan].abs().max()) == 0.0


def test_gradients_are_bit_identical_over_two_runs():
    t, K = _inputs("shipped")
    a, b = (_run(PointPillarV2XRealLoss, ARGS, t, True) for _ in range(2))
    for k in ("cls_preds", "reg_preds"):
        assert torch.equal(a[2][k], b[2][k]), k


def test_stage1_shell_with_three_classes_trains_through_the_fused_criterion():
    """A stage-1 shell with num_class 3 at the V2X-Real lidar range in train mode: forward, the fused GenComm criterion, backward.
    The head-map gradients equal the composition's; every parameter except dir_head.* (no direction term, as in the reference) gets a
    finite gradient."""
    from gencomm_amd.heter_model_baseline_w_gencomm_stage1 import HeterModelBaselineWGenCommStage1
    lidar_range = [-102.4, -51.2, -15.0, 102.4, 51.2, 15.0]
    args = synth.stage1_model_args(T=3, lidar_range=lidar_range, C=256)
    args["m1"]["encoder_args"]["voxel_size"] = [0.4, 0.4, 30]
    args["num_class"] = 3
    model = HeterModelBaselineWGenCommStage1(args)
    synth.fill_params_(model, 21)
    synth.fill_bn_stats_(model, 22)
    model = model.to(DEV).train()
    rl = [3]
    pil = synth.make_pillars(3000, 3, 512, 256, 23, voxel_size=[0.4, 0.4, 30], pc_range=lidar_range)
    data = {"agent_modality_list": ["m1"] * 3, "record_len": torch.tensor(rl),
            "pairwise_t_matrix": torch.from_numpy(synth.make_pairwise_t_matrix(rl, 5, 24, max_shift=6.0)).to(DEV),
            "inputs_m1": {k: torch.from_numpy(pil[k]).to(DEV) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}}
    out = model(data)
    assert tuple(out["cls_preds"].shape) == (1, 18, 64, 128) and tuple(out["reg_preds"].shape) == (1, 42, 64, 128)
    out["cls_preds"].retain_grad()
    out["reg_preds"].retain_grad()
    lab = synth.make_loss_inputs_v2xreal(25, 1, 64, 128, 2, 3, C=1, feature_hw=(1, 1))
    tgt = {"pos_equal_one": torch.from_numpy(lab["pos_equal_one"]).to(DEV), "targets": torch.from_numpy(lab["targets"]).to(DEV)}
    crit = PointPillarV2XRealGenCommLoss(ARGS)
    total = crit(out, tgt)
    assert _took_fused_path(total) and total.dtype == torch.float64 and math.isfinite(float(total.detach()))
    total.backward()
    ref = PointPillarV2XRealGenCommLoss(ARGS)
    ref.fuse_heads = False
    leaves = {k: out[k].detach().clone().requires_grad_(True) for k in ("cls_preds", "reg_preds")}
    ref_total = ref(dict(leaves, gt_feature=out["gt_feature"].detach(), pred_feature=out["pred_feature"].detach()), tgt)
    ref_total.backward()
    assert float(total.detach()) == pytest.approx(float(ref_total.detach()), rel=3e-6)
    for k, leaf in leaves.items():
        scale = float(leaf.grad.abs().max()) + 1e-30
        assert float((out[k].grad - leaf.grad).abs().max()) <= 2e-5 * scale, k
    def without_grad():
        return {n for n, p in model.named_parameters() if p.requires_grad and p.grad is None}
    missing = without_grad()
    bad = [n for n, p in model.named_parameters() if p.grad is not None and not torch.isfinite(p.grad).all()]
    assert not bad, bad
    # parameters that no output reaches (the Enhancer's inactive block) stay without gradient under any loss: a probe through every
    # output of a second forward finds them; what the criterion leaves out beyond those is exactly dir_head.*
    model.zero_grad(set_to_none=True)
    out = model(data)
    sum(out[k].square().mean() for k in ("cls_preds", "reg_preds", "dir_preds", "gt_feature", "pred_feature")).backward()
    unreachable = without_grad()
    assert missing - unreachable == {"dir_head.weight", "dir_head.bias"}, sorted(missing - unreachable)
    print(f"stage-1 shell, 3 classes, train mode: total {float(total.detach()):.4f}; without gradient: dir_head + {len(unreachable)} unreachable")
