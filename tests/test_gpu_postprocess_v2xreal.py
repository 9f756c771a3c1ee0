"""V2X-Real multi-class detection tail on the GPU (VoxelPostprocessor.post_process_v2xreal through the HIP library) against the
reference's own outputs (tests/golden/postproc_v2xreal.npz) and, end to end from a stage-1 shell with num_class 3, against the
torch-CPU restatement (tests/v2xreal_restatement.py). Kept-box set and order exact, labels exact, scores within 1 ulp of the
sigmoid, corners within fp32 trig / matmul rounding -- the tolerances of tests/test_postprocess.py."""
import copy
import json
import math

import numpy as np
import pytest
import torch

import v2xreal_restatement as R
from helpers import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIDAR_RANGE = [-102.4, -51.2, -15.0, 102.4, 51.2, 15.0]


def _pp(params):
    from gencomm_amd.postprocess import VoxelPostprocessor
    return VoxelPostprocessor(params, train=False, class_names=R.CLASS_NAMES)


def _check(boxes, score_labels, ref_b, ref_sl):
    assert boxes.shape == ref_b.shape and score_labels.shape == ref_sl.shape    # same number of kept boxes ...
    got = score_labels.cpu().numpy()
    np.testing.assert_array_equal(got[:, 1], ref_sl[:, 1])                       # ... in the same order, same classes
    np.testing.assert_allclose(got[:, 0], ref_sl[:, 0], rtol=0, atol=2e-7)
    np.testing.assert_allclose(boxes.cpu().numpy(), ref_b, rtol=0, atol=3e-5)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_hip_post_process_v2xreal_vs_reference_golden(tag):
    g = load_case("postproc_v2xreal")
    params, data, out, projection = R.case_dicts(g, tag, DEV)
    boxes, score_labels = _pp(params).post_process_v2xreal(data, out, projection=projection)
    _check(boxes, score_labels, g[f"boxes_{tag}"], g[f"score_labels_{tag}"])
    ref_sl = g[f"score_labels_{tag}"]
    assert set(np.unique(ref_sl[:, 1]).tolist()) == {1.0, 2.0, 3.0}
    if tag == "c":   # two classes at sigmoid 1.0: the first wins, although the second has the larger logit
        assert ((ref_sl[:, 0] == 1.0) & (ref_sl[:, 1] == 1.0)).sum() == 1
    if tag in ("a", "b"):   # a kept box above z = 15 m: the range mask checks x and y only
        assert (g[f"boxes_{tag}"][:, :, 2] > 15.0).any()


def test_hip_post_process_v2xreal_size_filter_asserts_and_empty_returns_none():
    g = load_case("postproc_v2xreal")
    assert bool(g["raises_e"]) and bool(g["none_f"])
    params, data, out, projection = R.case_dicts(g, "e", DEV)
    pp = _pp(params)
    with pytest.raises(AssertionError):
        pp.post_process_v2xreal(data, out, projection=projection)
    params, data, out, projection = R.case_dicts(g, "f", DEV)
    assert pp.post_process_v2xreal(data, out, projection=projection) == (None, None)
    assert pp.post_process_v2xreal(data, {}, projection=projection) == (None, None)


def test_hip_post_process_v2xreal_capacity_overflow_raises():
    g = load_case("postproc_v2xreal")
    params = json.loads(str(g["params"]))
    params["anchor_args"].update(cav_lidar_range=LIDAR_RANGE, W=512, H=256)
    pp = _pp(params)
    anchors, _ = pp.generate_anchor_box_v2xreal()                     # 64 x 128 x 6 = 49 152 anchors, all above the threshold
    data = {"ego": {"transformation_matrix": torch.eye(4, device=DEV), "anchor_box": anchors}}
    out = {"ego": {"cls_preds": torch.full((1, 18, 64, 128), 5.0, device=DEV), "reg_preds": torch.zeros(1, 42, 64, 128, device=DEV)}}
    with pytest.raises(RuntimeError, match="exceed the capacity"):
        pp.post_process_v2xreal(data, out)


def test_hip_post_process_v2xreal_is_deterministic():
    g = load_case("postproc_v2xreal")
    params, data, out, projection = R.case_dicts(g, "b", DEV)
    pp = _pp(params)
    b1, s1 = pp.post_process_v2xreal(data, out)
    b2, s2 = _pp(params).post_process_v2xreal(data, out)
    assert torch.equal(b1, b2) and torch.equal(s1, s2)


def test_hip_post_process_v2xreal_more_agents_than_one_launch_takes():
    """Ten agents (two chunks of the decode launches) against the restatement; agent order, not id order."""
    from gencomm_amd import synth
    g = load_case("postproc_v2xreal")
    params = json.loads(str(g["params"]))
    anchors = [a for a in g["anchors"]]
    H, W = anchors[0].shape[:2]
    data, out = {}, {}
    for k in range(10):
        th = math.radians(9.0 * k)
        T = torch.tensor([[math.cos(th), -math.sin(th), 0, 1.5 * k - 7], [math.sin(th), math.cos(th), 0, 0.7 * k - 3], [0, 0, 1, 0.0], [0, 0, 0, 1]])
        data[f"a{9 - k}"] = {"transformation_matrix": T.to(DEV), "anchor_box": anchors}
        cls, reg = synth.make_detection_maps_v2xreal(H, W, 6, 3, 700 + k, n_obj=4)
        out[f"a{9 - k}"] = {"cls_preds": torch.from_numpy(cls).to(DEV), "reg_preds": torch.from_numpy(reg).to(DEV)}
    boxes, score_labels = _pp(params).post_process_v2xreal(data, out)
    ref_b, ref_sl = R.post_process_v2xreal(params, data, out)
    assert ref_b.shape[0] > 20
    _check(boxes, score_labels, ref_b.numpy(), ref_sl.numpy())


def test_stage1_shell_with_three_classes_end_to_end():
    """A stage-1 shell with num_class 3 at the V2X-Real lidar range (C = 256, 64 x 128 heads): its output_dict goes straight into
    post_process_v2xreal; the result equals the torch-CPU restatement on the same head tensors."""
    from gencomm_amd import synth
    from gencomm_amd.heter_model_baseline_w_gencomm_stage1 import HeterModelBaselineWGenCommStage1
    args = synth.stage1_model_args(T=3, lidar_range=LIDAR_RANGE, C=256)
    args["m1"]["encoder_args"]["voxel_size"] = [0.4, 0.4, 30]
    args["num_class"] = 3
    model = HeterModelBaselineWGenCommStage1(args).eval()
    synth.fill_params_(model, 21)
    synth.fill_bn_stats_(model, 22)
    model = model.to(DEV)
    rl = [3]
    pil = synth.make_pillars(3000, 3, 512, 256, 23, voxel_size=[0.4, 0.4, 30], pc_range=LIDAR_RANGE)
    data = {"agent_modality_list": ["m1"] * 3, "record_len": torch.tensor(rl),
            "pairwise_t_matrix": torch.from_numpy(synth.make_pairwise_t_matrix(rl, 5, 24, max_shift=6.0)).to(DEV),
            "inputs_m1": {k: torch.from_numpy(pil[k]).to(DEV) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}}
    with torch.no_grad():
        out = model(data)
        assert tuple(out["cls_preds"].shape) == (1, 18, 64, 128) and tuple(out["reg_preds"].shape) == (1, 42, 64, 128)
        # calibrate the synthetic heads like trained ones: ~300 anchors above the 0.2 threshold, box deltas of a few tenths
        best = out["cls_preds"].permute(0, 2, 3, 1).reshape(-1, 3).max(-1)[0]
        model.cls_head.bias.sub_(float(best.topk(300).values[-1]) - math.log(0.2 / 0.8))
        model.reg_head.weight.mul_(0.1 / max(float(out["reg_preds"].std()), 1e-6))
        model.reg_head.bias.zero_()
        out = model(data)
    params = json.loads(str(load_case("postproc_v2xreal")["params"]))
    params["gt_range"] = list(LIDAR_RANGE)
    params["anchor_args"].update(cav_lidar_range=list(LIDAR_RANGE), W=512, H=256)
    pp = _pp(params)
    anchors, _ = pp.generate_anchor_box_v2xreal()
    data_dict = {"ego": {"transformation_matrix": torch.eye(4, device=DEV), "anchor_box": anchors}}
    boxes, score_labels = pp.post_process_v2xreal(data_dict, {"ego": out})
    ref_b, ref_sl = R.post_process_v2xreal(params, data_dict, {"ego": out})
    print(f"stage-1 shell, 3 classes: {ref_b.shape[0]} boxes after NMS, per class {np.bincount(ref_sl[:, 1].numpy().astype(int), minlength=4)[1:].tolist()}")
    assert ref_b.shape[0] >= 20
    _check(boxes, score_labels, ref_b.numpy(), ref_sl.numpy())
