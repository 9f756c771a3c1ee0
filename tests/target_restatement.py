"""numpy restatement of the reference's training-time anchor target assignment (VoxelPostprocessor.generate_label and
generate_label_v2xreal, opencood/data_utils/post_processor/voxel_postprocessor.py:188-310 and :312-463, with collate_batch /
collate_batch_v2xreal :577-655), and the case table of tests/golden/target_assign.npz (tools/make_golden_target_assign.py).
Written from the formulas; never reads the reference. It is the reference's algorithm -- an anchors x boxes IoU matrix per
sample and class, then index logic over it -- but not its Cython: the overlaps are oracle/detect_port.py's numpy port.

Per class, with iou [N anchors, n boxes] (float32, stand-up boxes from float32 corners):
  best[j]  = argmax of column j (first maximum), kept when that maximum is > 0
  pos[a]   = any(iou[a] > pos_threshold) or a in best
  match[a] = the lowest j with iou[a, j] > pos_threshold, else the lowest j with best[j] == a
  neg[a]   = all(iou[a] < neg_threshold) and a not in best
  targets  = the seven float64 deltas of box match[a] against anchor a
generate_label reads the deltas' box from row match[a] of the UNFILTERED box array although the IoUs are those of the rows with
mask == 1 (the reference's :279); generate_label_v2xreal filters by mask and class first.
"""
import json

import numpy as np
import torch

from oracle import detect_port as D

MAX_NUM = 100
CLASS_NAMES = ["vehicle", "pedestrian", "truck"]
# tag -> number of samples; the single-class head has every case but (g), the V2X-Real head every case but (d)
CASES_SINGLE = {"a": 1, "b": 1, "c": 1, "d": 1, "e": 1, "f": 3, "h": 1}
CASES_V2XREAL = {"a": 1, "b": 1, "c": 2, "e": 1, "f": 3, "g": 1, "h": 1}


def standup_boxes(boxes7: np.ndarray) -> np.ndarray:
    """[n, 7] boxes (x, y, z, h, w, l, yaw) -> [n, 4] float32 (x1, y1, x2, y2) of the rotated footprint: float32 corners
    (torch cos / sin, a float32 matrix product, + centre), then min / max."""
    b = torch.from_numpy(np.ascontiguousarray(boxes7, dtype=boxes7.dtype)).float().reshape(-1, 7)
    n = b.shape[0]
    signs = torch.tensor([[1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, -1], [1, -1, 1], [1, 1, 1], [-1, 1, 1], [-1, -1, 1]],
                         dtype=torch.float32) / 2
    local = b[:, [5, 4, 3]][:, None, :].repeat(1, 8, 1) * signs[None]                 # (l, w, h) extents, all eight corners
    c, s = torch.cos(b[:, 6]), torch.sin(b[:, 6])
    zero, one = torch.zeros(n), torch.ones(n)
    rot = torch.stack([c, s, zero, -s, c, zero, zero, zero, one], dim=1).view(-1, 3, 3)
    xy = (torch.matmul(local, rot) + b[:, None, 0:3])[:, :, :2].numpy()
    out = np.zeros((n, 4))
    out[:, 0:2] = xy.min(axis=1)
    out[:, 2:4] = xy.max(axis=1)
    return out.astype(np.float32)


def iou_matrix(anchors7: np.ndarray, boxes7: np.ndarray) -> np.ndarray:
    return D.bbox_overlaps(standup_boxes(anchors7), standup_boxes(boxes7))


def _assign(iou: np.ndarray, pos_thr: float, neg_thr: float):
    """(match [N] int, -1 where not positive; all_below [N] bool; is_best [N] bool) of one class."""
    N, n = iou.shape
    match = np.full(N, -1, dtype=np.int64)
    is_best = np.zeros(N, dtype=bool)
    if n == 0:
        return match, np.ones(N, dtype=bool), is_best
    best = np.argmax(iou, axis=0)
    keep = iou[best, np.arange(n)] > 0
    for j in range(n - 1, -1, -1):    # descending, so that the lowest box index is the one left standing
        if keep[j]:
            match[best[j]] = j
            is_best[best[j]] = True
    above = iou > pos_thr
    has = above.any(axis=1)
    match[has] = above[has].argmax(axis=1)
    return match, (iou < neg_thr).all(axis=1), is_best


def _deltas(gt: np.ndarray, anchors: np.ndarray) -> np.ndarray:
    """[m, 7] float64 regression targets of boxes gt [m, >= 7] against anchors [m, 7]."""
    d = np.sqrt(anchors[:, 4] ** 2 + anchors[:, 5] ** 2)
    out = np.zeros((len(gt), 7))
    out[:, 0] = (gt[:, 0] - anchors[:, 0]) / d
    out[:, 1] = (gt[:, 1] - anchors[:, 1]) / d
    out[:, 2] = (gt[:, 2] - anchors[:, 2]) / anchors[:, 3]
    out[:, 3] = np.log(gt[:, 3] / anchors[:, 3])
    out[:, 4] = np.log(gt[:, 4] / anchors[:, 4])
    out[:, 5] = np.log(gt[:, 5] / anchors[:, 5])
    out[:, 6] = gt[:, 6] - anchors[:, 6]
    return out


def generate_label(gt_box_center, anchors, mask, pos_threshold, neg_threshold):
    """pos_equal_one, neg_equal_one [H, W, A] and targets [H, W, 7A], float64."""
    H, W, A = anchors.shape[:3]
    flat = anchors.reshape(-1, 7)
    valid = gt_box_center[mask == 1]
    match, all_below, is_best = _assign(iou_matrix(flat, valid[:, :7]), pos_threshold, neg_threshold)
    pos = match >= 0
    targets = np.zeros((H * W * A, 7))
    targets[pos] = _deltas(gt_box_center[match[pos]], flat[pos])     # the UNFILTERED array, indexed by the compacted index
    return {"pos_equal_one": pos.astype(np.float64).reshape(H, W, A), "neg_equal_one": (all_below & ~is_best).astype(np.float64).reshape(H, W, A),
            "targets": targets.reshape(H, W, A * 7)}


def generate_label_v2xreal(gt_box_center, anchors, num_anchors_per_location, mask, matched_thresholds, unmatched_thresholds):
    """pos_equal_one (the label map: -1 ignore, 0 background, class id) [H, W, S], targets [H, W, S, 7], neg_equal_one [H, W, R] of the
    last class; float64. `anchors`: per-class [H, W, R, 7]; the thresholds: per class, in the anchors' order."""
    gt_all = gt_box_center[mask == 1]
    labels_l, targets_l, neg = [], [], None
    for k, (an, R) in enumerate(zip(anchors, num_anchors_per_location)):
        H, W = an.shape[:2]
        flat = an.reshape(-1, 7)
        gt = gt_all[gt_all[:, -1] - 1 == k]
        match, all_below, is_best = _assign(iou_matrix(flat, gt[:, :7]), matched_thresholds[k], unmatched_thresholds[k])
        pos = match >= 0
        labels = np.where(all_below, 0.0, -1.0)
        labels[pos] = gt[match[pos], -1]
        targets = np.zeros((H * W * R, 7))
        targets[pos] = _deltas(gt[match[pos]], flat[pos])
        labels_l.append(labels.reshape(H, W, R))
        targets_l.append(targets.reshape(H, W, R, 7))
        neg = (all_below & ~is_best).astype(np.float64).reshape(H, W, R)
    return {"pos_equal_one": np.concatenate(labels_l, axis=-1), "targets": np.concatenate(targets_l, axis=-2), "neg_equal_one": neg}


def collate_batch(label_batch_list):
    return {k: np.array([d[k] for d in label_batch_list]) for k in ("targets", "pos_equal_one", "neg_equal_one")}


# ---------------------------------------------------------------------------------------------------------------------------------
# the fixture's cases
# ---------------------------------------------------------------------------------------------------------------------------------
def fixture_params(g):
    return json.loads(str(g["params_single"])), json.loads(str(g["params_v2xreal"]))


def case_inputs(g, head: str, tag: str):
    """(boxes [B, MAX_NUM, 7 | 8], mask [B, MAX_NUM]) of fixture case `tag` of head 's' (single class) or 'm' (V2X-Real)."""
    return g[f"boxes_{head}_{tag}"], g[f"mask_{head}_{tag}"]


def case_expected(g, head: str, tag: str):
    """The reference's collated outputs of a case, rebuilt from the sparse storage: pos / neg as float64 arrays, targets dense float64."""
    pos = g[f"pos_{head}_{tag}"].astype(np.float64)
    neg = g[f"neg_{head}_{tag}"].astype(np.float64)
    shape = tuple(int(v) for v in g[f"targets_shape_{head}_{tag}"])
    targets = np.zeros((int(np.prod(shape)) // 7, 7))
    targets[g[f"targets_index_{head}_{tag}"]] = g[f"targets_value_{head}_{tag}"]
    return {"pos_equal_one": pos, "neg_equal_one": neg, "targets": targets.reshape(shape)}


def restate_case(g, head: str, tag: str, anchors):
    """The restatement's collated outputs of a case; `anchors`: [H, W, A, 7] for head 's', the per-class list for 'm'."""
    ps, pm = fixture_params(g)
    boxes, mask = case_inputs(g, head, tag)
    out = []
    for b in range(boxes.shape[0]):
        if head == "s":
            out.append(generate_label(boxes[b], anchors, mask[b], ps["target_args"]["pos_threshold"], ps["target_args"]["neg_threshold"]))
        else:
            cfg = pm["anchor_args"]["anchor_generator_config"]
            out.append(generate_label_v2xreal(boxes[b], anchors, [a.shape[2] for a in anchors], mask[b],
                                              [c["matched_threshold"] for c in cfg], [c["unmatched_threshold"] for c in cfg]))
    return collate_batch(out)
