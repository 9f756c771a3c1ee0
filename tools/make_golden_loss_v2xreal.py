#!/usr/bin/env python3
"""Golden fixture of the V2X-Real training criteria, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_loss_v2xreal.py      # writes tests/golden/loss_v2xreal.npz

Labels and targets come from the reference's ``VoxelPostprocessor.generate_label_v2xreal``
(opencood/data_utils/post_processor/voxel_postprocessor.py:312-461) on synthetic ground-truth boxes, against the reference's own
``generate_anchor_box_v2xreal`` anchors, stacked as ``collate_batch_v2xreal`` (:622-656) does (float64). Import stubs are
oracle/make_golden.py's (``swanlab`` among the auto stand-ins); ``bbox_overlaps`` is the reference's Cython module that
oracle/build_ref.py compiles. Both reference criteria (opencood/loss/point_pillar_v2xreal_loss.py and
point_pillar_v2xreal_gencomm_loss.py) then run on the CPU.

The grid is the anchor configuration of tools/make_golden_postproc_v2xreal.py on a quarter of its area (51.2 m x 25.6 m, 16 x 32 head
map, S = 6 slots, K = 3): the classification gradient is dense, and this keeps the file far under the 1 MiB limit.

Stored per case: the labels and targets, the head-map seed (``gencomm_amd.synth.make_loss_heads_v2xreal``), the feature pair, the
totals and parts of both criteria with their dtypes, and the gradients of cls_preds and reg_preds (the same under both) and of
pred_feature.
Cases: (a) B = 2, plain; (b) the second sample without any box (no positives); (c) NaN targets (codes 0..5: a NaN yaw target makes the
reference's loss NaN) at some positive and some ignored slots; (d) labels / targets cast to float32 (the reference's arithmetic is then float32).
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

import numpy as np
import torch

from gencomm_amd import synth
from make_golden_postproc_v2xreal import CLASS_NAMES, load_reference, params

REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
SEED = 5200
ARGS = {"cls_weight": 1.0, "reg": 2.0, "num_class": 3, "generate_weight": 1}   # hypes_yaml/v2xreal/GenComm_yamls/gencomm/stage1/m1_att.yaml:202-208
TINY = params([-25.6, -12.8, -15, 25.6, 12.8, 15], 128, 64)
SIZES = {1: (1.56, 1.6, 3.9), 2: (1.73, 0.6, 0.8), 3: (3.0, 3.0, 8.0)}   # h, w, l of each class's anchor ('hwl' order)
MAX_NUM = 40


def gt_boxes(r, n_per_class):
    """(MAX_NUM, 8) boxes x, y, z, h, w, l, yaw, class and the valid mask; positions inside the range, sizes within 15 % of the
    class's anchor, yaw anywhere on the circle."""
    rows = []
    for cls, n in n_per_class.items():
        h, w, l = SIZES[cls]
        for _ in range(n):
            s = r.uniform(0.85, 1.15, 3)
            rows.append([r.uniform(-23, 23), r.uniform(-11, 11), r.uniform(-1.2, -0.6), h * s[0], w * s[1], l * s[2],
                         r.uniform(-math.pi, math.pi), cls])
    box = np.zeros((MAX_NUM, 8))
    mask = np.zeros(MAX_NUM)
    if rows:
        box[:len(rows)] = rows
        mask[:len(rows)] = 1
    return box, mask


def load_criteria():
    import opencood.loss.point_pillar_v2xreal_gencomm_loss as G
    import opencood.loss.point_pillar_v2xreal_loss as L
    return L.PointPillarV2XRealLoss, G.PointPillarV2XRealGenCommLoss


def main():
    VP = load_reference()
    pp = VP(copy.deepcopy(TINY), True, class_names=CLASS_NAMES)
    anchors, napl = pp.generate_anchor_box_v2xreal()
    H, W = anchors[0].shape[:2]
    K, S = len(anchors), sum(napl)
    Stage2, Stage1 = load_criteria()
    rec = dict(args=json.dumps(ARGS), dims=np.array([H, W, S, K]))
    for n_tag, tag in enumerate("abcd"):
        r = np.random.RandomState(SEED + 10 * n_tag)
        labels, targets = [], []
        for b in range(2):
            n_per_class = {} if (tag == "b" and b == 1) else {1: 6, 2: 8, 3: 3}
            box, mask = gt_boxes(r, n_per_class)
            ld = pp.generate_label_v2xreal(gt_box_center=box, anchors=anchors, num_anchors_per_location=napl, mask=mask)
            labels.append(ld["pos_equal_one"])
            targets.append(ld["targets"])
        lab = torch.from_numpy(np.array(labels))   # collate_batch_v2xreal
        tgt = torch.from_numpy(np.array(targets))
        assert lab.dtype == torch.float64 and tuple(lab.shape) == (2, H, W, S) and tuple(tgt.shape) == (2, H, W, S, 7)
        if tag == "c":
            for sel in (lab > 0, lab < 0):
                idx = torch.nonzero(sel)
                pick = idx[torch.from_numpy(r.rand(len(idx)) < 0.3)]
                tgt[pick[:, 0], pick[:, 1], pick[:, 2], pick[:, 3], torch.from_numpy(r.randint(0, 6, len(pick)))] = float("nan")
        if tag == "d":
            lab, tgt = lab.float(), tgt.float()
        seed = SEED + 10 * n_tag + 1
        cls, reg = synth.make_loss_heads_v2xreal(seed, tgt.double().numpy(), K)
        gt = np.maximum(r.normal(0, 1, (2, 4, 8, 8)), 0).astype(np.float32)
        pred = (gt + r.normal(0, 0.3, gt.shape)).astype(np.float32)
        rec.update({f"labels_{tag}": lab.numpy(), f"targets_{tag}": tgt.numpy(), f"seed_{tag}": np.int64(seed),
                    f"gt_feature_{tag}": gt, f"pred_feature_{tag}": pred})
        for crit_name, crit_cls in (("stage2", Stage2), ("gencomm", Stage1)):
            leaves = {"cls_preds": torch.from_numpy(cls).requires_grad_(True), "reg_preds": torch.from_numpy(reg).requires_grad_(True),
                      "pred_feature": torch.from_numpy(pred).requires_grad_(True)}
            crit = crit_cls(dict(ARGS))
            total = crit(dict(leaves, gt_feature=torch.from_numpy(gt)), {"pos_equal_one": lab, "targets": tgt})
            total.backward()
            p = f"{crit_name}_{tag}"
            rec[f"total_{p}"] = np.float64(total.item())
            rec[f"dtype_{p}"] = str(total.dtype).replace("torch.", "")
            for k in ("conf_loss", "reg_loss") + (("gen_loss",) if crit_name == "gencomm" else ()):
                rec[f"{k}_{p}"] = np.float64(crit.loss_dict[k].item())
            for k in ("cls_preds", "reg_preds"):   # the generate term does not reach the heads: one copy per case
                if crit_name == "stage2":
                    rec[f"grad_{k}_{tag}"] = leaves[k].grad.numpy()
                else:
                    assert np.array_equal(rec[f"grad_{k}_{tag}"], leaves[k].grad.numpy()), k
            if crit_name == "gencomm":
                rec[f"grad_pred_feature_{tag}"] = leaves["pred_feature"].grad.numpy()
            print(f"case {tag} {crit_name}: total {total.item():.6f} ({total.dtype}), conf {crit.loss_dict['conf_loss'].item():.6f}, "
                  f"reg {crit.loss_dict['reg_loss'].item():.6f}, positives per sample {(lab > 0).flatten(1).sum(1).tolist()}, "
                  f"ignored {int((lab < 0).sum())}, NaN targets {int(torch.isnan(tgt).sum())}")
    path = os.path.join(OUT, "loss_v2xreal.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
