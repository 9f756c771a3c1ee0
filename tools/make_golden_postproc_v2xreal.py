#!/usr/bin/env python3
"""Golden fixture of the V2X-Real multi-class detection tail, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_postproc_v2xreal.py      # writes tests/golden/postproc_v2xreal.npz

The reference's ``VoxelPostprocessor`` (opencood/data_utils/post_processor/voxel_postprocessor.py) runs with oracle/make_golden.py's
import stubs: ``generate_anchor_box_v2xreal`` (:123-186) and ``post_process_v2xreal`` (:787-943) with the box_utils helpers they
call. shapely is absent: ``common_utils.convert_format`` / ``compute_iou`` (its only users on this path, inside ``nms_rotated``) are
bound to the oracle's float64 convex-clipping quad IoU, as oracle/make_golden.py's ``postproc`` case does, so the polygon IoU
arithmetic stays PARITY UNPINNED here too; the greedy loop, the sort, the filters, the range mask and everything before them are
the reference's. The compiled reference ``bbox_overlaps`` (oracle/_ref) satisfies the module's import.

Stored: the params JSON, the head-map seeds (``gencomm_amd.synth.make_detection_maps_v2xreal``; the case tag names the variant),
the agent-to-ego matrices, the reference's anchors and outputs on a reduced grid (102.4 m x 51.2 m, 32 x 64 head map), and the
SHA-256 of the anchors at the shipped V2X-Real grid (204.8 m x 102.4 m, 0.4 m voxels, stride 4: 64 x 128 head map).
Cases: (a) one agent; (b) three agents, the second absent from output_dict; (c) two classes saturated to a sigmoid of 1.0 at one
anchor; (d) projection=False; (e) a length delta that breaks the 100 m size filter (the reference raises AssertionError);
(f) no candidate above the threshold (the reference returns (None, None)).
"""
from __future__ import annotations

import copy
import hashlib
import json
import math
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import numpy as np
import torch

from gencomm_amd import synth

REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
SEED = 4100

ANCHOR_CONFIG = [   # hypes_yaml/v2xreal/GenComm_yamls/gencomm/stage1/m1_att.yaml:76-100
    {"class_name": "vehicle", "anchor_sizes": [[3.9, 1.6, 1.56]], "anchor_rotations": [0, 1.57], "anchor_bottom_heights": [-1.78],
     "align_center": True, "feature_map_stride": 4, "matched_threshold": 0.6, "unmatched_threshold": 0.45},
    {"class_name": "pedestrian", "anchor_sizes": [[0.8, 0.6, 1.73]], "anchor_rotations": [0, 1.57], "anchor_bottom_heights": [-0.6],
     "align_center": True, "feature_map_stride": 4, "matched_threshold": 0.5, "unmatched_threshold": 0.35},
    {"class_name": "truck", "anchor_sizes": [[8, 3, 3]], "anchor_rotations": [0, 1.57], "anchor_bottom_heights": [-1.78],
     "align_center": True, "feature_map_stride": 4, "matched_threshold": 0.6, "unmatched_threshold": 0.45},
]
CLASS_NAMES = ["vehicle", "pedestrian", "truck"]


def params(cav_range, W, H):
    """The yaml's `postprocess` block, with the voxel grid W x H (x, y) the yaml parser adds to anchor_args."""
    r = [float(v) for v in cav_range]
    return {"core_method": "VoxelPostprocessor", "gt_range": r,
            "anchor_args": {"cav_lidar_range": r, "l": 3.9, "w": 1.6, "h": 1.56, "r": [0, 90], "feature_stride": 4, "num": 2,
                            "vw": 0.4, "vh": 0.4, "vd": 30, "W": W, "H": H, "D": 1, "anchor_generator_config": copy.deepcopy(ANCHOR_CONFIG)},
            "target_args": {"pos_threshold": 0.6, "neg_threshold": 0.45, "score_threshold": 0.2},
            "order": "hwl", "max_num": 150, "nms_thresh": 0.15,
            "dir_args": {"dir_offset": 0.7853, "num_bins": 2, "anchor_yaw": [0, 90]}}


SHIPPED = params([-102.4, -51.2, -15, 102.4, 51.2, 15], 512, 256)
SMALL = params([-51.2, -25.6, -15, 51.2, 25.6, 15], 256, 128)
VARIANT = {"a": "plain", "b": "plain", "c": "saturate", "d": "plain", "e": "oversize", "f": "empty"}


def anchors_sha256(all_anchors) -> str:
    h = hashlib.sha256()
    for a in all_anchors:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def tmat(yaw_deg, tx, ty, tz=0.0):
    c, s = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    return np.array([[c, -s, 0, tx], [s, c, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]], dtype=np.float32)


def load_reference():
    from make_golden import _install_stubs
    import build_ref
    import detect_port as D
    _install_stubs()
    sys.path.insert(0, REF)
    bo = build_ref.load_box_overlaps()
    if bo is None:
        assert build_ref.build(), "oracle/_ref/box_overlaps could not be built"
        bo = build_ref.load_box_overlaps()
    import opencood.utils as ou
    sys.modules["opencood.utils.box_overlaps"] = bo
    ou.box_overlaps = bo
    from opencood.data_utils.post_processor.voxel_postprocessor import VoxelPostprocessor
    from opencood.utils import common_utils
    common_utils.convert_format = lambda boxes: np.asarray(boxes, dtype=np.float64)[:, :4, :2]
    common_utils.compute_iou = lambda box, boxes: D.quad_iou_one_to_many(box, boxes)
    return VoxelPostprocessor


def main():
    VP = load_reference()
    shipped, napl_shipped = VP(copy.deepcopy(SHIPPED), False, class_names=CLASS_NAMES).generate_anchor_box_v2xreal()
    assert [a.shape for a in shipped] == [(64, 128, 2, 7)] * 3 and napl_shipped == [2, 2, 2]
    pp = VP(copy.deepcopy(SMALL), False, class_names=CLASS_NAMES)
    anchors, napl = pp.generate_anchor_box_v2xreal()
    H, W, R = anchors[0].shape[:3]
    A, nc = sum(napl), len(anchors)
    rec = dict(params=json.dumps(SMALL), anchors=np.stack(anchors), anchors_sha256_shipped=anchors_sha256(shipped))
    Ts = [tmat(0, 0, 0), tmat(12.0, 6.5, -3.0, 0.2), tmat(-30.0, -9.0, 4.0, -0.1)]
    rec["T"] = np.stack(Ts)
    cases = {"a": ([0], [0], True), "b": ([0, 1, 2], [2, 0], True), "c": ([1], [1], True), "d": ([1], [1], False),
             "e": ([0], [0], True), "f": ([0], [0], True)}
    for n_tag, tag in enumerate("abcdef"):
        in_data, in_out, projection = cases[tag]
        seed = SEED + 10 * n_tag
        data, out, n_above = {}, {}, 0
        for k in in_data:
            data[f"cav{k}"] = {"transformation_matrix": torch.from_numpy(Ts[k]), "anchor_box": anchors, "num_anchors_per_location": napl}
        for k in in_out:   # output_dict in its own order: the reference visits data_dict's order
            cls, reg = synth.make_detection_maps_v2xreal(H, W, A, nc, seed + k, variant=VARIANT[tag])
            out[f"cav{k}"] = {"cls_preds": torch.from_numpy(cls), "reg_preds": torch.from_numpy(reg)}
            prob = torch.sigmoid(torch.from_numpy(cls).permute(0, 2, 3, 1)).reshape(-1, nc)
            best = prob.max(-1)[0]
            sel = best[best > 0.2]
            n_above += int(sel.numel())
            assert sel.numel() == sel.unique().numel() or tag == "c", f"case {tag}: tied candidate scores (NMS tie order unpinned)"
        rec[f"seed_{tag}"] = np.int64(seed)
        try:
            boxes, score_labels = pp.post_process_v2xreal(data, out, projection=projection)
        except AssertionError:
            assert tag == "e"
            rec["raises_e"] = np.bool_(True)
            print(f"case {tag}: {n_above} candidates -> AssertionError (size filter)")
            continue
        if boxes is None:
            assert tag == "f"
            rec["none_f"] = np.bool_(True)
            print(f"case {tag}: no candidate -> (None, None)")
            continue
        rec[f"boxes_{tag}"] = boxes.numpy().astype(np.float32)
        rec[f"score_labels_{tag}"] = score_labels.numpy().astype(np.float32)
        labels = score_labels[:, 1].numpy()
        print(f"case {tag}: {n_above} candidates -> {len(labels)} boxes, labels {np.bincount(labels.astype(int), minlength=4)[1:].tolist()}, "
              f"max |z| {float(boxes[..., 2].abs().max()):.1f}")
    path = os.path.join(OUT, "postproc_v2xreal.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
