#!/usr/bin/env python3
"""V2X-Real GenComm criterion timing at the stage-1 shape: batch_size 2 scenes of 2 agents, 64 x 128 heads, S = 6 slots, K = 3 classes
(cls [2, 18, 64, 128], reg [2, 42, 64, 128], float64 labels / targets as the reference's collate gives them) and a gt / pred feature pair
[4, 256, 64, 128]. Median wall time per call of forward + backward of PointPillarV2XRealGenCommLoss, with the head terms fused
(gencomm_head_loss_mc) and as the framework-operator composition, alternated in rounds on the same inputs; every call ends in a device
synchronise. Launches per call come from a separate kernel trace of one mode alone:

    python tools/loss_v2xreal_bench.py [--iters 200] [--warmup 20] [--mode both|fused|composed]
    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/loss_v2xreal_bench.py --mode fused --iters 100 --warmup 0

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from gencomm_amd import synth
from gencomm_amd.point_pillar_v2xreal_gencomm_loss import PointPillarV2XRealGenCommLoss

ARGS = {"cls_weight": 1.0, "reg": 2.0, "num_class": 3, "generate_weight": 1}   # v2xreal/GenComm_yamls/gencomm/stage1/m1_att.yaml


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mode", choices=("both", "fused", "composed"), default="both")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    t = synth.make_loss_inputs_v2xreal(31, 2, 64, 128, 2, 3, C=256)
    t = {k: torch.from_numpy(v).to(dev) for k, v in t.items()}
    feat = synth.make_loss_inputs_v2xreal(32, 4, 64, 128, 2, 3, C=256)
    t["gt_feature"], t["pred_feature"] = (torch.from_numpy(feat[k]).to(dev) for k in ("gt_feature", "pred_feature"))
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("cls_preds", "reg_preds", "pred_feature")}
    target = {"pos_equal_one": t["pos_equal_one"], "targets": t["targets"]}
    crits = {}
    for mode in ("fused", "composed"):
        crits[mode] = PointPillarV2XRealGenCommLoss(ARGS)
        crits[mode].fuse_heads = mode == "fused"
    modes = ["fused", "composed"] if a.mode == "both" else [a.mode]

    def call(mode):
        for v in leaves.values():
            v.grad = None
        total = crits[mode](dict(leaves, gt_feature=t["gt_feature"]), target)
        total.backward()
        torch.cuda.synchronize()
        return total

    res = {"shape": "B=2 (2x2 agents), heads 64x128, S=6, K=3, float64 labels/targets, feature [4,256,64,128]", "iters": a.iters}
    grads = {}
    for mode in modes:
        for _ in range(a.warmup):
            call(mode)
        total = call(mode)
        grads[mode] = (float(total.detach()), {k: v.grad.clone() for k, v in leaves.items()})
    times = {m: [] for m in modes}
    for _ in range(a.iters):      # alternate the modes call by call: both see the same host and device load
        for mode in modes:
            t0 = time.perf_counter()
            call(mode)
            times[mode].append(time.perf_counter() - t0)
    for mode in modes:
        res[f"{mode}_us_per_call"] = float(np.median(times[mode])) * 1e6
    if len(modes) == 2:
        res["speedup"] = res["composed_us_per_call"] / res["fused_us_per_call"]
        res["total_rel_diff"] = abs(grads["fused"][0] - grads["composed"][0]) / abs(grads["composed"][0])
        res["grad_max_rel_diff"] = max(float((grads["fused"][1][k] - g).abs().max() / g.abs().max()) for k, g in grads["composed"][1].items())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
