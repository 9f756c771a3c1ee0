#!/usr/bin/env python3
"""Timing of the two terms the HEAL and MPDA criteria add (gencomm_amd/baseline_criteria.py), forward + backward, against the float32
torch restatement (tests/baseline_criteria_restatement.py) on the same GPU in the same process:

  occ      the occupancy term at the shape the pyramid benches use: 5 agents, label maps 128 x 256 x 2 anchors, levels 128 x 256,
           64 x 128, 32 x 64 (relative_downsample [1, 2, 4])
  domain   the domain term on da_feature [5, 1, 64, 128], record_len [2, 3]

Device time between two events on the stream, as tools/bench_pyramid.py measures it (warm-up, then `--reps` rounds of `--iters` calls
of each function in turn; the median window with the fastest and slowest beside it); the copy bandwidth is measured in the same process.
Kernel counts come from torch's profiler (every device kernel of one forward + backward, the framework's conversions included);
`library_launches` is what the library itself enqueues.

    python tools/bench_baseline_criteria.py [--iters 20] [--reps 7] [--warmup 3] [--out profiles/baseline_criteria_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np
import torch

from bench_pyramid import AGENTS, H, W, alternate, count_kernels, stats

LEVELS, WEIGHTS, PCW, GAMMA, ALPHA = [1, 2, 4], [0.4, 0.2, 0.1], 2.0, 2.0, 0.25
DA_SHAPE, RECORD_LEN = (5, 1, 64, 128), [2, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "baseline_criteria_bench.json"))
    a = ap.parse_args()
    import baseline_criteria_restatement as R
    from gencomm_amd import _lib
    from gencomm_amd import baseline_criteria as BC
    if not torch.cuda.is_available():
        raise SystemExit("bench_baseline_criteria needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup}
    src = torch.empty(128 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    w = alternate({"copy": lambda: dst.copy_(src)}, 5, a.reps, a.warmup)["copy"]
    out["copy_gbps"] = round(2 * src.numel() * 4 / statistics.median(w) / 1e3, 1)
    del src, dst
    print(json.dumps({"copy_gbps": out["copy_gbps"]}), flush=True)
    rng = np.random.RandomState(11)

    # ---- the occupancy term
    u = rng.rand(AGENTS, H, W, 2)
    pos, neg = torch.from_numpy((u < 0.02).astype(np.float32)).to(dev), torch.from_numpy((u > 0.05).astype(np.float32)).to(dev)
    occ = [torch.from_numpy(rng.normal(-1.0, 1.5, (AGENTS, 1, H // k, W // k)).astype(np.float32)).to(dev).requires_grad_(True) for k in LEVELS]

    def hip_occ():
        total, _ = BC.pyramid_occ_loss(occ, pos, neg, LEVELS, WEIGHTS, PCW, GAMMA, ALPHA)
        return total, torch.autograd.grad(total, occ)

    def torch_occ():
        total = R.occ_loss(occ, pos, neg, LEVELS, WEIGHTS, PCW, GAMMA, ALPHA)[0]
        return total, torch.autograd.grad(total, occ)

    fns = {"us": hip_occ, "torch_us": torch_occ}
    t = alternate(fns, a.iters, a.reps, a.warmup)
    res = {"labels": [AGENTS, H, W, 2], "levels": [[H // k, W // k] for k in LEVELS], "library_launches": 2}
    for k in fns:
        stats(res, k, t[k])
    res["torch_over_hip"] = round(res["torch_us"] / res["us"], 2)
    res["kernels"], res["torch_kernels"] = count_kernels(hip_occ), count_kernels(torch_occ)
    (lh, gh), (lt, gt) = hip_occ(), torch_occ()
    res["loss_rel_diff_vs_torch"] = abs(float(lh) - float(lt)) / abs(float(lt))
    res["grad_rel_rms_vs_torch"] = [float((x - y).pow(2).mean().sqrt() / y.pow(2).mean().sqrt()) for x, y in zip(gh, gt)]
    res["bytes"] = 4 * (2 * pos.numel() * 2 + 3 * sum(o.numel() for o in occ))   # labels read by both launches, logits read twice, gradient written
    print(json.dumps({"occ": res}), flush=True)
    out["occ"] = res

    # ---- the domain term
    x = torch.from_numpy(rng.normal(0.2, 1.2, DA_SHAPE).astype(np.float32)).to(dev).requires_grad_(True)

    def hip_da():
        v = BC.domain_bce_loss(x, RECORD_LEN)
        return v, torch.autograd.grad(v, x)

    def torch_da():
        v = R.domain_bce(x, RECORD_LEN)
        return v, torch.autograd.grad(v, x)

    fns = {"us": hip_da, "torch_us": torch_da}
    t = alternate(fns, a.iters, a.reps, a.warmup)
    res = {"da_feature": list(DA_SHAPE), "record_len": RECORD_LEN, "library_launches": 2}
    for k in fns:
        stats(res, k, t[k])
    res["torch_over_hip"] = round(res["torch_us"] / res["us"], 2)
    res["kernels"], res["torch_kernels"] = count_kernels(hip_da), count_kernels(torch_da)
    (lh, gh), (lt, gt) = hip_da(), torch_da()
    res["loss_rel_diff_vs_torch"] = abs(float(lh) - float(lt)) / abs(float(lt))
    res["grad_rel_rms_vs_torch"] = float((gh[0] - gt[0]).pow(2).mean().sqrt() / gt[0].pow(2).mean().sqrt())
    print(json.dumps({"domain": res}), flush=True)
    out["domain"] = res

    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
