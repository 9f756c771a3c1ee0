#!/usr/bin/env python3
"""Anchor target assignment timing at the shipped shapes: OPV2V 128 x 256 x 2 anchors (one class) and V2X-Real 64 x 128 x 6 (three
classes), B = 1 and 4 samples, 20 / 60 / 100 valid boxes per sample of max_num 100. Device time per call of
VoxelPostprocessor.generate_label_batch (two launches of gencomm_target_assign_fwd; boxes, mask and the prepared anchors already on
the device, as they are after train_utils.to_device), float32 outputs: warm-up, then the mean over `--iters` calls enqueued back to
back between two events on the stream, then a synchronisation.

Yardsticks:
  floor      every output map written exactly once, B H W A (1 + 1 + 7) elements (V2X-Real: the label map, the targets and the last
             class's neg_equal_one) at `--hbm-tbps` (default 8.0, the MI355X's HBM3E peak); reported as time / floor.
  cpu        tests/target_restatement.py on this host, per sample summed over the batch: the reference's algorithm (an anchors x boxes
             IoU matrix, then index logic) in numpy, but NOT the reference's Cython -- the reference itself is not on the GPU machine.
  h2d bytes  what no longer crosses per step (the three float64 maps of the collate) against what does (the boxes and the mask): arithmetic.

    python tools/target_assign_bench.py [--iters 200] [--warmup 20] [--no-cpu] [--out profiles/target_assign_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/target_assign_bench.py --no-cpu --iters 10 --warmup 0 --out ''   # launches per call

Prints one JSON line per shape and writes them all to --out.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

from gencomm_amd.postprocess import VoxelPostprocessor

MAX_NUM = 100
V2X_CONFIG = [{"class_name": n, "anchor_sizes": [s], "anchor_rotations": [0, 1.57], "anchor_bottom_heights": [z], "align_center": True,
               "feature_map_stride": 4, "matched_threshold": p, "unmatched_threshold": u}
              for n, s, z, p, u in (("vehicle", [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), ("pedestrian", [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
                                    ("truck", [8, 3, 3], -1.78, 0.6, 0.45))]
V2X_RANGE = [-102.4, -51.2, -15.0, 102.4, 51.2, 15.0]
V2X_PARAMS = {"order": "hwl", "target_args": {"pos_threshold": 0.6, "neg_threshold": 0.45},
              "anchor_args": {"cav_lidar_range": V2X_RANGE, "W": 512, "H": 256, "num": 2, "anchor_generator_config": V2X_CONFIG}}
OPV2V_RANGE = [-102.4, -51.2, -3.0, 102.4, 51.2, 1.0]
OPV2V_PARAMS = {"order": "hwl", "target_args": {"pos_threshold": 0.6, "neg_threshold": 0.45},
                "anchor_args": {"cav_lidar_range": OPV2V_RANGE, "l": 3.9, "w": 1.6, "h": 1.56, "r": [0, 90], "feature_stride": 2, "num": 2,
                                "vw": 0.4, "vh": 0.4, "W": 512, "H": 256}}
SIZES = {1: (1.56, 1.6, 3.9), 2: (1.73, 0.6, 0.8), 3: (3.0, 3.0, 8.0)}   # h, w, l


def make_boxes(seed, B, n, classes):
    r = np.random.RandomState(seed)
    box, mask = np.zeros((B, MAX_NUM, 8)), np.zeros((B, MAX_NUM))
    for b in range(B):
        for j in range(n):
            cls = classes[j % len(classes)]
            h, w, l = SIZES[cls]
            s = r.uniform(0.85, 1.15, 3)
            box[b, j] = [r.uniform(-98, 98), r.uniform(-47, 47), -1.0, h * s[0], w * s[1], l * s[2], r.uniform(-math.pi, math.pi), cls]
        mask[b, :n] = 1
    return box, mask


def device_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hbm-tbps", type=float, default=8.0)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement (for a kernel trace of the device calls alone)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "target_assign_bench.json"))
    a = ap.parse_args()
    import target_restatement as R
    dev = torch.device("cuda:0")
    heads = {}
    pp = VoxelPostprocessor(OPV2V_PARAMS, train=True)
    heads["opv2v"] = (pp, pp.generate_anchor_box(), [1], 7)
    pp = VoxelPostprocessor(V2X_PARAMS, train=True, class_names=[c["class_name"] for c in V2X_CONFIG])
    heads["v2xreal"] = (pp, pp.generate_anchor_box_v2xreal()[0], [1, 2, 3], 8)
    results = []
    for name, (pp, anchors, classes, width) in heads.items():
        parts = anchors if isinstance(anchors, list) else [anchors]
        H, W, R_ = parts[0].shape[:3]
        S = R_ * len(parts)
        for B in (1, 4):
            for n in (20, 60, 100):
                box, mask = make_boxes(1000 + n + B, B, n, classes)
                box = box[:, :, :width]
                db, dm = torch.from_numpy(box).to(dev), torch.from_numpy(mask).to(dev)
                out = pp.generate_label_batch(db, dm, anchors)
                torch.cuda.synchronize()
                us = device_us(lambda: pp.generate_label_batch(db, dm, anchors), a.iters, a.warmup)
                elems = B * H * W * (S * 8 + R_)      # label / pos map + 7 targets per slot, neg_equal_one of one class
                floor_us = elems * 4 / (a.hbm_tbps * 1e12) * 1e6
                res = {"head": name, "shape": f"{H}x{W}x{S}", "B": B, "boxes_per_sample": n, "device_us_per_call": round(us, 2),
                       "launches_per_call": 2, "floor_us": round(floor_us, 3), "times_floor": round(us / floor_us, 1),
                       "positives": int((out["pos_equal_one"] > 0).sum()),
                       "h2d_bytes_before": B * H * W * (S * 8 + R_) * 8, "h2d_bytes_now": B * MAX_NUM * (width + 1) * 8}
                if not a.no_cpu:
                    thr = [(c["matched_threshold"], c["unmatched_threshold"]) for c in V2X_CONFIG]
                    t = OPV2V_PARAMS["target_args"]

                    def cpu():
                        if name == "opv2v":
                            return R.collate_batch([R.generate_label(box[b], anchors, mask[b], t["pos_threshold"], t["neg_threshold"]) for b in range(B)])
                        return R.collate_batch([R.generate_label_v2xreal(box[b], anchors, [R_] * 3, mask[b], [p for p, _ in thr], [u for _, u in thr])
                                                for b in range(B)])
                    want = cpu()
                    reps = 3
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        cpu()
                    res["cpu_restatement_us_per_call"] = round((time.perf_counter() - t0) / reps * 1e6, 1)
                    res["speedup_over_cpu_restatement"] = round(res["cpu_restatement_us_per_call"] / us, 1)
                    # random boxes, not conditioned like the fixture's: an IoU within float rounding of a threshold may fall either way
                    res["integer_map_differences"] = int((out["pos_equal_one"].cpu().numpy() != want["pos_equal_one"]).sum()
                                                         + (out["neg_equal_one"].cpu().numpy() != want["neg_equal_one"]).sum())
                print(json.dumps(res), flush=True)
                results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "hbm_tbps": a.hbm_tbps,
                       "output_dtype": "float32", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
