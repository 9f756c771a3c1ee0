#!/usr/bin/env python3
"""V2X-Real detection tail timing at the shipped shape: `--agents` agents (default 4) with 64 x 128 heads, 6 anchors per location
and 3 classes (18 / 42 channels), about 300 candidates above the 0.2 threshold in all. Median wall time per call of
VoxelPostprocessor.post_process_v2xreal (HIP: decode + NMS + gather, and the one host read of the counts), against the torch-CPU
restatement of the reference's tail (tests/v2xreal_restatement.py: torch ops, numpy NMS loop with the oracle's quad IoU) on the same
head maps, already on the host. The heads are resident on the device before the clock starts, as they are after a model forward.

    python tools/postproc_v2xreal_bench.py [--agents 4] [--iters 50] [--warmup 5] [--no-cpu]

Prints one JSON line.
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

from gencomm_amd import synth
from gencomm_amd.postprocess import VoxelPostprocessor

CONFIG = [{"class_name": n, "anchor_sizes": [s], "anchor_rotations": [0, 1.57], "anchor_bottom_heights": [z], "align_center": True,
           "feature_map_stride": 4, "matched_threshold": 0.6, "unmatched_threshold": 0.45}
          for n, s, z in (("vehicle", [3.9, 1.6, 1.56], -1.78), ("pedestrian", [0.8, 0.6, 1.73], -0.6), ("truck", [8, 3, 3], -1.78))]
RANGE = [-102.4, -51.2, -15.0, 102.4, 51.2, 15.0]
PARAMS = {"gt_range": RANGE, "order": "hwl", "nms_thresh": 0.15, "target_args": {"score_threshold": 0.2},
          "anchor_args": {"cav_lidar_range": RANGE, "W": 512, "H": 256, "num": 2, "anchor_generator_config": CONFIG}}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement (for a kernel trace of the HIP tail alone)")
    a = ap.parse_args()
    import v2xreal_restatement as R
    dev = torch.device("cuda:0")
    pp = VoxelPostprocessor(PARAMS, class_names=[c["class_name"] for c in CONFIG])
    anchors, _ = pp.generate_anchor_box_v2xreal()
    data, out, out_cpu = {}, {}, {}
    for k in range(a.agents):
        th = math.radians(20.0 * k)
        T = torch.tensor([[math.cos(th), -math.sin(th), 0, 8.0 * k], [math.sin(th), math.cos(th), 0, -3.0 * k], [0, 0, 1, 0], [0, 0, 0, 1]])
        cls, reg = synth.make_detection_maps_v2xreal(64, 128, 6, 3, 900 + k, n_obj=48 // a.agents)
        data[f"cav{k}"] = {"transformation_matrix": T.to(dev), "anchor_box": anchors}
        out[f"cav{k}"] = {"cls_preds": torch.from_numpy(cls).to(dev), "reg_preds": torch.from_numpy(reg).to(dev)}
        out_cpu[f"cav{k}"] = {"cls_preds": torch.from_numpy(cls), "reg_preds": torch.from_numpy(reg)}
    data_cpu = {k: {"transformation_matrix": v["transformation_matrix"].cpu(), "anchor_box": anchors} for k, v in data.items()}
    n_cand = sum(int((torch.sigmoid(o["cls_preds"]).permute(0, 2, 3, 1).reshape(-1, 3).max(-1)[0] > 0.2).sum()) for o in out_cpu.values())
    boxes, sl = pp.post_process_v2xreal(data, out)
    torch.cuda.synchronize()
    hip_us = timed(lambda: pp.post_process_v2xreal(data, out), a.iters, a.warmup)
    res = {"shape": f"{a.agents} agents x 64x128, A=6, 3 classes", "candidates": n_cand, "boxes": int(boxes.shape[0]),
           "hip_us_per_call": hip_us}
    if not a.no_cpu:
        ref_b, ref_sl = R.post_process_v2xreal(PARAMS, data_cpu, out_cpu)
        res["cpu_restatement_us_per_call"] = timed(lambda: R.post_process_v2xreal(PARAMS, data_cpu, out_cpu), max(3, a.iters // 10), 1)
        res["speedup"] = res["cpu_restatement_us_per_call"] / hip_us
        res["same_boxes"] = bool(ref_b.shape == boxes.shape and torch.equal(ref_sl[:, 1], sl[:, 1].cpu())
                                 and float((ref_b - boxes.cpu()).abs().max()) <= 3e-5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
