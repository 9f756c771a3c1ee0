#!/usr/bin/env python3
"""Golden fixture of the training-time anchor target assignment, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_target_assign.py      # writes tests/golden/target_assign.npz

The reference's ``VoxelPostprocessor.generate_label`` (opencood/data_utils/post_processor/voxel_postprocessor.py:188-310),
``generate_label_v2xreal`` (:312-463) and ``collate_batch`` / ``collate_batch_v2xreal`` (:577-655) run on synthetic ground-truth
boxes against the reference's own anchors, with the import route of tools/make_golden_postproc_v2xreal.py (``_install_stubs`` and
the compiled ``box_overlaps`` of oracle/_ref).

Grids: single-class 102.4 m x 51.2 m, 0.4 m voxels, stride 2 (64 x 128 x 2 anchors of 3.9 x 1.6 x 1.56 m at 0 / 90 degrees, thresholds
0.6 / 0.45); V2X-Real 32 x 64 with the three-class ANCHOR_CONFIG of tools/make_golden_postproc_v2xreal.py. The anchors themselves are not
stored: the package's generators rebuild them and the file holds their SHA-256, at these grids and at the shipped ones.

Stored per case and head ('s' single class, 'm' V2X-Real): boxes [B, 100, 7 | 8], mask [B, 100], the collated pos_equal_one / neg_equal_one
as int8, and the targets sparsely -- the slots of the positives and their seven float64 values; everything else is asserted zero here.
Cases: (a) about 30 boxes of mixed yaw and size; (b) boxes partly or wholly outside the anchor grid (a best IoU of exactly 0 gives no
positive); (c) mask all zero -- for V2X-Real also a sample whose boxes leave one class empty; (d) a mask that is not a prefix of ones, with
other boxes in the masked rows (single class: the deltas are read from the unfiltered array, :279); (e) pairs of boxes over the same
anchors; (f) three samples through the collate; (g) V2X-Real pedestrians only (thresholds 0.5 / 0.35); (h) float32 boxes (the float64
copy of the same values gives the same outputs, asserted here).

The condition on the inputs, asserted with the reference's own IoU matrix: no IoU within 1e-4 of a threshold it is compared with; for
every box the best and second-best anchor IoUs differ by more than 1e-4 unless the best is exactly 0; every non-zero best IoU exceeds
1e-4. Offending boxes are redrawn; the margins reached and the number of redraws are stored.
"""
from __future__ import annotations

import copy
import json
import math
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np

from make_golden_postproc_v2xreal import CLASS_NAMES, SHIPPED as V2X_SHIPPED, SMALL as V2X_SMALL, anchors_sha256, load_reference
from target_restatement import CASES_SINGLE, CASES_V2XREAL, MAX_NUM

OUT = os.path.join(REPO, "tests", "golden")
SEED = 6300
MARGIN = 1e-4


def single_params(cav_range, W, H):
    r = [float(v) for v in cav_range]
    return {"core_method": "VoxelPostprocessor", "gt_range": r,
            "anchor_args": {"cav_lidar_range": r, "l": 3.9, "w": 1.6, "h": 1.56, "r": [0, 90], "feature_stride": 2, "num": 2,
                            "vw": 0.4, "vh": 0.4, "vd": 4, "W": W, "H": H, "D": 1},
            "target_args": {"pos_threshold": 0.6, "neg_threshold": 0.45, "score_threshold": 0.2},
            "order": "hwl", "max_num": MAX_NUM, "nms_thresh": 0.15,
            "dir_args": {"dir_offset": 0.7853, "num_bins": 2, "anchor_yaw": [0, 90]}}


SINGLE_SHIPPED = single_params([-102.4, -51.2, -3, 102.4, 51.2, 1], 512, 256)   # 128 x 256 x 2 anchors
SINGLE_SMALL = single_params([-51.2, -25.6, -3, 51.2, 25.6, 1], 256, 128)       # 64 x 128 x 2
SIZES = {1: (1.56, 1.6, 3.9), 2: (1.73, 0.6, 0.8), 3: (3.0, 3.0, 8.0)}          # h, w, l of each class's anchor ('hwl' order)
Z = {1: -1.0, 2: -0.6, 3: -1.0}


class Checker:
    """The condition on the inputs, on the reference's own IoU matrix (its boxes_to_corners_3d / corner2d_to_standup_box / bbox_overlaps)."""

    def __init__(self):
        from opencood.utils import box_utils
        from opencood.utils.box_overlaps import bbox_overlaps
        self.bu, self.bo = box_utils, bbox_overlaps
        self.thr_margin, self.gap, self.least_best, self.redraws = math.inf, math.inf, math.inf, 0
        self._anchor_cache = {}

    def standup(self, boxes7):
        return np.ascontiguousarray(self.bu.corner2d_to_standup_box(self.bu.boxes_to_corners_3d(boxes7, "hwl"))).astype(np.float32)

    def iou(self, anchors, boxes7):
        key = id(anchors)
        if key not in self._anchor_cache:
            self._anchor_cache[key] = (anchors, self.standup(anchors.reshape(-1, 7)))
        return self.bo(self._anchor_cache[key][1], self.standup(boxes7))

    def offenders(self, anchors, boxes7, thresholds, record):
        """Indices of the boxes that miss the condition; with `record`, the margins of the others enter the file's statistics."""
        if len(boxes7) == 0:
            return []
        iou = self.iou(anchors, boxes7).astype(np.float64)
        bad = []
        for j in range(iou.shape[1]):
            col = iou[:, j]
            near = min(float(np.abs(col - t).min()) for t in thresholds)
            top = np.sort(col)[-2:]
            best, gap = float(top[1]), float(top[1] - top[0])
            ok = near > MARGIN and (best == 0.0 or (gap > MARGIN and best > MARGIN))
            if not ok:
                bad.append(j)
            elif record:
                self.thr_margin = min(self.thr_margin, near)
                if best > 0:
                    self.gap, self.least_best = min(self.gap, gap), min(self.least_best, best)
        return bad


def draw_box(r, cls, xr, yr, yaw=None):
    h, w, l = SIZES[cls]
    s = r.uniform(0.8, 1.2, 3)
    return [r.uniform(*xr), r.uniform(*yr), Z[cls] + r.uniform(-0.3, 0.3), h * s[0], w * s[1], l * s[2],
            r.uniform(-math.pi, math.pi) if yaw is None else yaw, float(cls)]


def sample_rows(r, tag, head, rng):
    """Box rows (8 wide, class in the last column) of one sample of a case, as (row, group) -- rows of one group are redrawn together."""
    x0, y0, x1, y1 = rng
    inside = ((x0 + 4, x1 - 4), (y0 + 4, y1 - 4))
    classes = [1] if head == "s" else [1, 2, 3]
    rows = []
    if tag in ("a", "d", "f", "h"):
        n = {"a": 30, "d": 14, "f": 18, "h": 20}[tag]
        for i in range(n):
            rows.append(([draw_box(r, classes[i % len(classes)] if r.rand() < 0.8 else classes[r.randint(len(classes))], *inside)], "one"))
    elif tag == "b":
        for i in range(8):   # centre within 3 m of the border: the footprint sticks out of the grid
            cls = classes[i % len(classes)]
            side = r.randint(4)
            xr = (x0 - 1, x0 + 3) if side == 0 else (x1 - 3, x1 + 1) if side == 1 else inside[0]
            yr = (y0 - 1, y0 + 3) if side == 2 else (y1 - 3, y1 + 1) if side == 3 else inside[1]
            rows.append(([draw_box(r, cls, xr, yr)], "one"))
        for i in range(5):   # wholly outside, more than 15 m away: IoU exactly 0 with every anchor
            rows.append(([draw_box(r, classes[i % len(classes)], (x1 + 15, x1 + 40), (y1 + 15, y1 + 30))], "one"))
        for i in range(6):
            rows.append(([draw_box(r, classes[i % len(classes)], *inside)], "one"))
    elif tag == "e":
        for i in range(6):   # two boxes a few centimetres apart, same yaw: the same anchors pass the threshold for both
            cls = classes[i % len(classes)]
            a = draw_box(r, cls, *inside, yaw=r.uniform(-0.2, 0.2) + (math.pi / 2) * r.randint(2))
            b = list(a)
            b[0] += r.uniform(-0.06, 0.06)
            b[1] += r.uniform(-0.06, 0.06)
            b[5] *= r.uniform(0.97, 1.03)
            rows.append(([a, b], "pair"))
        for i in range(6):
            rows.append(([draw_box(r, classes[i % len(classes)], *inside)], "one"))
    elif tag == "g":
        for i in range(25):
            rows.append(([draw_box(r, 2, *inside)], "one"))
    elif tag == "c":
        for i in range(9):
            rows.append(([draw_box(r, classes[i % len(classes)], *inside)], "one"))
    return rows


def build_sample(r, chk, tag, head, b, anchors_of_class, thresholds_of_class, rng):
    """(boxes [MAX_NUM, 8] float64, mask [MAX_NUM]) of sample b of a case, every valid box meeting the condition."""
    groups = sample_rows(r, tag, head, rng)
    if head == "m" and tag == "c" and b == 1:      # a class with no box
        groups = [g for g in groups if g[0][0][7] != 3.0]
    for attempt in range(200):
        rows = [row for g in groups for row in g[0]]
        owner = [gi for gi, g in enumerate(groups) for _ in g[0]]
        arr = np.array(rows).reshape(-1, 8)
        bad_groups = set()
        for cls, an in anchors_of_class.items():
            sel = np.nonzero(arr[:, 7] == cls)[0] if head == "m" else np.arange(len(arr))
            for j in chk.offenders(an, arr[sel, :7], thresholds_of_class[cls], record=False):
                bad_groups.add(owner[sel[j]])
        if not bad_groups:
            break
        chk.redraws += len(bad_groups)
        fresh = sample_rows(r, tag, head, rng)
        for gi in bad_groups:   # a fresh draw of the same kind (and the same class)
            same = [g for g in fresh if g[1] == groups[gi][1] and g[0][0][7] == groups[gi][0][0][7]]
            groups[gi] = same[r.randint(len(same))] if same else groups[gi]
    else:
        raise AssertionError(f"case {tag}/{head}: the condition was not met after 200 redraws")
    for cls, an in anchors_of_class.items():
        sel = np.nonzero(arr[:, 7] == cls)[0] if head == "m" else np.arange(len(arr))
        assert not chk.offenders(an, arr[sel, :7], thresholds_of_class[cls], record=True)
    n = len(arr)
    box, mask = np.zeros((MAX_NUM, 8)), np.zeros(MAX_NUM)
    if tag == "c" and not (head == "m" and b == 1):
        box[:n] = arr                      # boxes present, every one of them masked out
    elif tag == "d":
        # valid rows scattered: a masked row (holding another box) before and between them
        slots = np.sort(r.choice(np.arange(1, 2 * n), n, replace=False))
        fill = np.array([draw_box(r, 1, (rng[0] + 4, rng[2] - 4), (rng[1] + 4, rng[3] - 4)) for _ in range(2 * n)])
        box[:2 * n] = fill
        box[slots] = arr
        mask[slots] = 1
        assert mask[0] == 0 and not np.all(mask[:n] == 1)
    else:
        box[:n] = arr
        mask[:n] = 1
    return box, mask


def store(rec, head, tag, boxes, mask, out):
    pos, neg, tgt = (np.asarray(out[k]) for k in ("pos_equal_one", "neg_equal_one", "targets"))
    assert pos.dtype == neg.dtype == tgt.dtype == np.float64
    assert np.array_equal(pos, pos.astype(np.int8)) and np.array_equal(neg, neg.astype(np.int8))
    rows = tgt.reshape(-1, 7)
    positive = (pos > 0).reshape(-1)
    assert rows.shape[0] == positive.shape[0] and not rows[~positive].any(), "targets are zero off the positives"
    idx = np.nonzero(positive)[0].astype(np.int32)
    assert np.isfinite(rows[idx]).all()
    rec.update({f"boxes_{head}_{tag}": boxes, f"mask_{head}_{tag}": mask, f"pos_{head}_{tag}": pos.astype(np.int8),
                f"neg_{head}_{tag}": neg.astype(np.int8), f"targets_shape_{head}_{tag}": np.array(tgt.shape, dtype=np.int64),
                f"targets_index_{head}_{tag}": idx, f"targets_value_{head}_{tag}": rows[idx]})
    vals, counts = np.unique(pos, return_counts=True)
    print(f"case {tag}/{head}: B {boxes.shape[0]}, valid boxes {mask.sum(axis=1).astype(int).tolist()}, "
          f"pos map values {dict(zip(vals.tolist(), counts.tolist()))}, neg {int(neg.sum())}, shapes {pos.shape} {neg.shape} {tgt.shape}")


def main():
    VP = load_reference()
    chk = Checker()
    rec = dict(params_single=json.dumps(SINGLE_SMALL), params_v2xreal=json.dumps(V2X_SMALL), margin=np.float64(MARGIN))
    # ---- anchors
    ps = VP(copy.deepcopy(SINGLE_SMALL), True)
    an_s = ps.generate_anchor_box()
    assert an_s.shape == (64, 128, 2, 7) and an_s.dtype == np.float64
    shipped_s = VP(copy.deepcopy(SINGLE_SHIPPED), True).generate_anchor_box()
    assert shipped_s.shape == (128, 256, 2, 7)
    pm = VP(copy.deepcopy(V2X_SMALL), True, class_names=CLASS_NAMES)
    an_m, napl = pm.generate_anchor_box_v2xreal()
    assert [a.shape for a in an_m] == [(32, 64, 2, 7)] * 3 and napl == [2, 2, 2]
    shipped_m, _ = VP(copy.deepcopy(V2X_SHIPPED), True, class_names=CLASS_NAMES).generate_anchor_box_v2xreal()
    rec.update(params_single_shipped=json.dumps(SINGLE_SHIPPED), params_v2xreal_shipped=json.dumps(V2X_SHIPPED),
               anchors_sha256_single=anchors_sha256([an_s]), anchors_sha256_single_shipped=anchors_sha256([shipped_s]),
               anchors_sha256_v2xreal=anchors_sha256(an_m), anchors_sha256_v2xreal_shipped=anchors_sha256(shipped_m))
    t = SINGLE_SMALL["target_args"]
    cfg = V2X_SMALL["anchor_args"]["anchor_generator_config"]
    heads = {
        "s": (CASES_SINGLE, {1: an_s}, {1: (t["pos_threshold"], t["neg_threshold"])}, SINGLE_SMALL["anchor_args"]["cav_lidar_range"]),
        "m": (CASES_V2XREAL, {k + 1: a for k, a in enumerate(an_m)},
              {k + 1: (c["matched_threshold"], c["unmatched_threshold"]) for k, c in enumerate(cfg)}, V2X_SMALL["anchor_args"]["cav_lidar_range"]),
    }
    for head, (cases, an_of, thr_of, lr) in heads.items():
        rng = (lr[0], lr[1], lr[3], lr[4])
        for n_tag, (tag, B) in enumerate(cases.items()):
            r = np.random.RandomState(SEED + 100 * (head == "m") + 10 * n_tag)
            boxes, masks = zip(*[build_sample(r, chk, tag, head, b, an_of, thr_of, rng) for b in range(B)])
            boxes, masks = np.stack(boxes), np.stack(masks)
            if head == "s":
                boxes = boxes[:, :, :7]
            if tag == "h":
                boxes = boxes.astype(np.float32)     # the condition is re-asserted on the rounded values below
                for b in range(B):
                    for cls, an in an_of.items():
                        v = boxes[b][masks[b] == 1]
                        v = v[v[:, -1] == cls] if head == "m" else v
                        assert not chk.offenders(an, v[:, :7].astype(np.float64), thr_of[cls], record=True)

            def run(bx):
                if head == "s":
                    return VP.collate_batch([ps.generate_label(gt_box_center=bx[b], anchors=an_s, mask=masks[b]) for b in range(B)])
                return VP.collate_batch_v2xreal([pm.generate_label_v2xreal(gt_box_center=bx[b], anchors=an_m, num_anchors_per_location=napl,
                                                                           mask=masks[b]) for b in range(B)])
            out = {k: v.numpy() for k, v in run(boxes).items()}
            if tag == "h":
                for k, v in run(boxes.astype(np.float64)).items():
                    assert np.array_equal(v.numpy(), out[k]), f"float64 copy of the float32 boxes: {k} differs"
            store(rec, head, tag, boxes, masks, out)
    rec.update(margin_threshold=np.float64(chk.thr_margin), margin_best_gap=np.float64(chk.gap), margin_least_best=np.float64(chk.least_best),
               redraws=np.int64(chk.redraws))
    assert chk.thr_margin > MARGIN and chk.gap > MARGIN and chk.least_best > MARGIN
    print(f"condition: nearest IoU to a threshold {chk.thr_margin:.3e}, least best / second-best gap {chk.gap:.3e}, "
          f"least non-zero best IoU {chk.least_best:.3e}, boxes redrawn {chk.redraws}")
    path = os.path.join(OUT, "target_assign.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
