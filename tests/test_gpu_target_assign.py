"""Training-time anchor target assignment on the GPU (gencomm_target_assign_fwd, csrc/target_kernels.h, through
VoxelPostprocessor.generate_label / generate_label_v2xreal / generate_label_batch) against the reference's own outputs
(tests/golden/target_assign.npz), against the numpy restatement on exact ties, for the workspace's self-reset and determinism, and
end to end into the training criteria.

The fixture's inputs keep every IoU 1e-4 away from every decision (tests/test_target_assign.py), so EVERY anchor of EVERY case is
compared: the integer maps exactly, the float64 targets to rtol = atol = 1e-12 (a subtraction and a division, or one log, in
float64; the device's log and sqrt may differ from numpy's in the last bits)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import target_restatement as R
from gencomm_amd import synth
from gencomm_amd.postprocess import VoxelPostprocessor
from test_target_assign import CASES, GOLD, fixture_anchors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("pos_equal_one", "neg_equal_one", "targets")
_state = {}


def ctx():
    """(fixture, single-class post-processor + anchors, V2X-Real post-processor + anchors): one pair of post-processors for the module,
    so that the anchor preparation and the workspaces are shared between the tests as they are between training steps."""
    if not _state:
        g = np.load(GOLD)
        ps, pm = R.fixture_params(g)
        an_s, an_m = fixture_anchors(g)
        _state.update(g=g, s=(VoxelPostprocessor(copy.deepcopy(ps), train=True), an_s),
                      m=(VoxelPostprocessor(copy.deepcopy(pm), train=True, class_names=R.CLASS_NAMES), an_m))
    return _state


def device_inputs(head, tag):
    boxes, mask = R.case_inputs(ctx()["g"], head, tag)
    return torch.from_numpy(boxes).to(DEV), torch.from_numpy(mask).to(DEV)


def run_batch(head, boxes, mask, dtype):
    pp, an = ctx()[head]
    return pp.generate_label_batch(boxes, mask, an, dtype=dtype)


def run_per_sample(head, boxes, mask, dtype):
    pp, an = ctx()[head]
    if head == "s":
        return VoxelPostprocessor.collate_batch([pp.generate_label(gt_box_center=boxes[b], anchors=an, mask=mask[b], dtype=dtype)
                                                 for b in range(boxes.shape[0])])
    return VoxelPostprocessor.collate_batch_v2xreal([pp.generate_label_v2xreal(gt_box_center=boxes[b], anchors=an, num_anchors_per_location=[2, 2, 2],
                                                                               mask=mask[b], dtype=dtype) for b in range(boxes.shape[0])])


def assert_matches(got, want, what):
    """`got`: device dictionary (float64); `want`: numpy dictionary. Integer maps exactly, targets to 1e-12, every anchor."""
    for k in KEYS:
        a = got[k].cpu().numpy()
        assert got[k].dtype == torch.float64 and a.shape == want[k].shape, (what, k, a.shape, want[k].shape)
        if k == "targets":
            err = np.abs(a - want[k])
            print(f"{what}: targets max abs diff {err.max():.3e} over {int((want[k] != 0).sum())} non-zero values, "
                  f"{int((a != want[k]).sum())} values not bit-equal")
            np.testing.assert_allclose(a, want[k], rtol=1e-12, atol=1e-12, err_msg=f"{what} {k}")
        else:
            print(f"{what}: {k} differs at {int((a != want[k]).sum())} of {a.size} anchors")
            np.testing.assert_array_equal(a, want[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("head,tag", CASES)
def test_matches_the_reference(head, tag):
    g = ctx()["g"]
    boxes, mask = device_inputs(head, tag)
    got = run_batch(head, boxes, mask, torch.float64)
    B = boxes.shape[0]
    shapes = {"s": ((B, 64, 128, 2), (B, 64, 128, 2), (B, 64, 128, 14)), "m": ((B, 32, 64, 6), (B, 32, 64, 2), (B, 32, 64, 6, 7))}[head]
    assert tuple(tuple(got[k].shape) for k in KEYS) == shapes
    assert_matches(got, R.case_expected(g, head, tag), f"{head}/{tag}")
    if tag == "h":   # the float64 copy of the float32 boxes gives the same maps
        again = run_batch(head, boxes.double(), mask, torch.float64)
        for k in KEYS:
            assert torch.equal(again[k], got[k]), k


@pytest.mark.parametrize("head,tag", CASES)
def test_float32_is_the_float64_result_rounded_once(head, tag):
    boxes, mask = device_inputs(head, tag)
    f64, f32 = run_batch(head, boxes, mask, torch.float64), run_batch(head, boxes, mask, torch.float32)
    default = ctx()[head][0].generate_label_batch(boxes, mask, ctx()[head][1])
    for k in KEYS:
        assert f32[k].dtype == default[k].dtype == torch.float32
        assert torch.equal(f32[k], f64[k].to(torch.float32)) and torch.equal(default[k], f32[k]), k


@pytest.mark.parametrize("head,tag", CASES)
def test_batch_equals_the_per_sample_calls_stacked(head, tag):
    boxes, mask = device_inputs(head, tag)
    for dtype in (torch.float64, torch.float32):
        a, b = run_batch(head, boxes, mask, dtype), run_per_sample(head, boxes, mask, dtype)
        for k in KEYS:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, dtype)


@pytest.mark.parametrize("head", ["s", "m"])
def test_consecutive_calls_share_one_workspace(head):
    """Different inputs, one after the other, through the same workspace: no per-box key of the first call reaches the second, and
    the workspace is zero again after every call (the kernels clear what they used; nothing is memset per call)."""
    g = ctx()["g"]
    pp, _ = ctx()[head]
    tags = ["a", "e", "c", "b", "a"] if head == "s" else ["a", "e", "g", "b", "a"]
    inputs = {t: tuple(x[:1] for x in device_inputs(head, t)) for t in set(tags)}    # B = 1 everywhere: one workspace
    results = [run_batch(head, *inputs[t], torch.float64) for t in tags]             # enqueued back to back, checked afterwards
    ws = [v for k, v in pp._cache.items() if k[0] == "target_ws" and k[2] == 1]
    assert len(ws) == 1 and not ws[0].any()
    for t, got in zip(tags, results):
        want = {k: v[:1] for k, v in R.case_expected(g, head, t).items()}
        assert_matches(got, want, f"{head}/{t} in a row")


@pytest.mark.parametrize("head", ["s", "m"])
def test_two_runs_are_bit_identical(head):
    boxes, mask = device_inputs(head, "f")
    a, b = run_batch(head, boxes, mask, torch.float64), run_batch(head, boxes, mask, torch.float64)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


def test_mask_dtypes_and_device_anchors():
    boxes, mask = device_inputs("s", "d")
    pp, an = ctx()["s"]
    want = run_batch("s", boxes, mask, torch.float64)
    for m in (mask.float(), mask.long(), mask.int(), mask.bool(), mask.to(torch.uint8), mask.half()):
        got = pp.generate_label_batch(boxes, m, an, dtype=torch.float64)
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (m.dtype, k)
    an_dev = torch.from_numpy(an).to(DEV)
    got = pp.generate_label_batch(boxes, mask, an_dev, dtype=torch.float64)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):     # the caller's stream
        got = pp.generate_label_batch(boxes, mask, an, dtype=torch.float64)
    side.synchronize()
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k


def exact_tie_case():
    """Inputs on which every operation before the thresholds is exact (yaw 0: cos 1, sin 0; coordinates and sizes small multiples of
    2^-3), with ties: the two anchors of a location are the same box (the lower index wins), a box midway between two locations ties
    their anchors, a box midway between four, and two identical boxes (the lower box index wins)."""
    H, W, A = 16, 32, 2
    an = np.zeros((H, W, A, 7))
    an[..., 0] = (np.arange(W) * 1.0 - 16.0)[None, :, None]
    an[..., 1] = (np.arange(H) * 1.0 - 8.0)[:, None, None]
    an[..., 2] = -1.0
    an[..., 3:6] = [1.5, 2.0, 4.0]     # h, w, l
    rows = [[-10.0, -4.0, -1.0, 1.5, 2.0, 4.0, 0.0],      # on an anchor: IoU 1 with both anchors of the location
            [-3.5, 2.0, -1.25, 1.5, 2.0, 4.0, 0.0],       # midway between two locations along x
            [4.5, -2.5, -0.75, 1.75, 2.25, 4.5, 0.0],     # midway between four locations
            [9.0, 4.0, -1.0, 1.5, 2.0, 4.0, 0.0],         # two identical boxes
            [9.0, 4.0, -1.0, 1.5, 2.0, 4.0, 0.0],
            [40.0, 30.0, -1.0, 1.5, 2.0, 4.0, 0.0]]       # far outside: best IoU 0
    boxes, mask = np.zeros((1, 16, 7)), np.zeros((1, 16))
    boxes[0, :len(rows)], mask[0, :len(rows)] = rows, 1
    return an, boxes, mask


def test_exact_ties_equal_the_restatement():
    an, boxes, mask = exact_tie_case()
    params, _ = R.fixture_params(ctx()["g"])
    thr = params["target_args"]["pos_threshold"], params["target_args"]["neg_threshold"]
    iou = R.iou_matrix(an.reshape(-1, 7), boxes[0][mask[0] == 1])
    best = iou.max(axis=0)
    assert [(iou[:, j] == best[j]).sum() for j in range(6)][:5] == [2, 4, 8, 2, 2] and best[5] == 0   # the ties are there
    want = R.collate_batch([R.generate_label(boxes[0], an, mask[0], *thr)])
    pp = VoxelPostprocessor(copy.deepcopy(params), train=True)
    got = pp.generate_label_batch(torch.from_numpy(boxes).to(DEV), torch.from_numpy(mask).to(DEV), an, dtype=torch.float64)
    assert_matches(got, want, "exact ties")
    assert int(want["pos_equal_one"].sum()) >= 5


def _grads(total, leaves):
    total.backward()
    return {k: v.grad.clone() for k, v in leaves.items()}


def _close(a, b, rtol, what):
    """|a - b| <= rtol * max|b|: the figure is printed before it is asserted."""
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print(f"{what}: max abs diff {err:.3e}, scale {scale:.3e}, ratio {err / max(scale, 1e-300):.3e}")
    assert err <= rtol * scale, what


def test_end_to_end_single_class_criterion():
    """PointPillarGencommLoss on synthetic head maps with device-made float32 labels against the same call on the fixture's labels
    converted to float32, case (f): the integer maps are identical and a target may differ by one float32 ulp (6e-8) where the float64
    values differ in their last bits; rtol 1e-6 leaves a factor of ten over that for a sum over a few hundred positives."""
    from gencomm_amd.point_pillar_gencomm_loss import PointPillarGencommLoss
    g = ctx()["g"]
    args = json.loads(str(np.load(os.path.join(os.path.dirname(GOLD), "loss.npz"))["args"]))
    boxes, mask = device_inputs("s", "f")
    B, H, W, A = 3, 64, 128, 2
    maps = [synth.make_detection_maps(H, W, A, 700 + b) for b in range(B)]
    heads = {k: torch.from_numpy(np.concatenate([m[i] for m in maps])).to(DEV) for i, k in enumerate(("cls_preds", "reg_preds", "dir_preds"))}
    r = np.random.RandomState(701)
    gt = torch.from_numpy(np.maximum(r.normal(0, 1, (B, 8, 16, 16)), 0).astype(np.float32)).to(DEV)
    heads["pred_feature"] = gt + 0.3
    made = run_batch("s", boxes, mask, torch.float32)
    want = {k: torch.from_numpy(v).to(DEV).float() for k, v in R.case_expected(g, "s", "f").items()}
    assert torch.equal(made["pos_equal_one"], want["pos_equal_one"]) and torch.equal(made["neg_equal_one"], want["neg_equal_one"])
    res = {}
    for name, labels in (("device", made), ("fixture", want)):
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in heads.items()}
        crit = PointPillarGencommLoss(copy.deepcopy(args))
        total = crit(dict(leaves, gt_feature=gt), labels)
        assert any("HeadLossFn" in type(f).__name__ for f in _graph(total)), "the one-launch head loss takes float32 maps"
        res[name] = (total.detach(), _grads(total, leaves))
    print(f"total: device labels {float(res['device'][0]):.9f}, fixture labels {float(res['fixture'][0]):.9f}")
    assert float(res["device"][0]) == pytest.approx(float(res["fixture"][0]), rel=1e-6)
    for k in ("cls_preds", "reg_preds", "dir_preds"):
        _close(res["device"][1][k], res["fixture"][1][k], 1e-6, f"grad {k}")


def _graph(total):
    todo, seen = [total.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        todo.extend(n for n, _ in f.next_functions)
    return seen


def test_end_to_end_v2xreal_criterion():
    """PointPillarV2XRealLoss with device-made float64 labels against the fixture's, case (f), rtol 1e-10."""
    from gencomm_amd.point_pillar_v2xreal_loss import PointPillarV2XRealLoss
    g = ctx()["g"]
    boxes, mask = device_inputs("m", "f")
    want = R.case_expected(g, "m", "f")
    cls, reg = synth.make_loss_heads_v2xreal(702, want["targets"], 3)
    made = run_batch("m", boxes, mask, torch.float64)
    want = {k: torch.from_numpy(v).to(DEV) for k, v in want.items()}
    assert torch.equal(made["pos_equal_one"], want["pos_equal_one"])
    res = {}
    for name, labels in (("device", made), ("fixture", want)):
        leaves = {"cls_preds": torch.from_numpy(cls).to(DEV).requires_grad_(True), "reg_preds": torch.from_numpy(reg).to(DEV).requires_grad_(True)}
        crit = PointPillarV2XRealLoss({"cls_weight": 1.0, "reg": 2.0, "num_class": 3})
        total = crit(dict(leaves), {"pos_equal_one": labels["pos_equal_one"], "targets": labels["targets"]})
        res[name] = (total.detach(), _grads(total, leaves))
    print(f"total: device labels {float(res['device'][0]):.15f}, fixture labels {float(res['fixture'][0]):.15f}")
    assert float(res["device"][0]) == pytest.approx(float(res["fixture"][0]), rel=1e-10)
    for k in ("cls_preds", "reg_preds"):
        _close(res["device"][1][k], res["fixture"][1][k], 1e-10, f"grad {k}")
