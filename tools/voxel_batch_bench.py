#!/usr/bin/env python3
"""Batched lidar front end (SpVoxelPreprocessor.preprocess_batch_device) against the per-agent loop it replaces, A = 4 agents x 60 000
points, raw clouds already on the device, ego mask and projection on:

  pillar   the OPV2V PointPillars grid: +-102.4 x +-51.2 m, 0.4 m pillars (512 x 256 x 1), 32 points per voxel, 32 000 voxels per agent
  second   the OPV2V SECOND grid: +-140.8 x +-40 m, 0.1 m voxels (2816 x 800 x 40), 5 points per voxel, 70 000 voxels per agent

  batched  one preprocess_batch_device call. device_us: the mean over `--iters` calls with return_padded=True (no host read) enqueued back
           to back between two stream events; wall_us: the mean wall time of the default call, its one host read included.
  loop     what a caller has to do without it: per agent mask_ego and projection with torch on the device (index + matmul),
           preprocess_device (its host read), the three results copied to the host, the reference's numpy collate, the collated
           arrays copied back. wall_us as above; device_us is the time between two stream events around the loop, so it contains the
           host's gaps. preprocess_device and its kernels are the parent commit's, unchanged, so the loop measured here is the baseline.
  floor    bytes of points read + voxel rows written (features, coordinates, counts) at `--hbm-tbps` (default 6.3, the measured float4
           copy rate of the MI355X; 8.0 is the HBM3E specification).

    python tools/voxel_batch_bench.py [--iters 50] [--warmup 5] [--out profiles/voxel_batch_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/voxel_batch_bench.py --only batched --grid pillar --iters 10 --warmup 0 --out ''

With --only the script runs that side alone (for a kernel trace: dispatches per call = total dispatches / iters).
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

from gencomm_amd.sp_voxel_preprocessor import SpVoxelPreprocessor

GRIDS = {
    "pillar": {"cav_lidar_range": [-102.4, -51.2, -3, 102.4, 51.2, 1],
               "args": {"voxel_size": [0.4, 0.4, 4], "max_points_per_voxel": 32, "max_voxel_train": 32000, "max_voxel_test": 32000}},
    "second": {"cav_lidar_range": [-140.8, -40, -3, 140.8, 40, 1],
               "args": {"voxel_size": [0.1, 0.1, 0.1], "max_points_per_voxel": 5, "max_voxel_train": 70000, "max_voxel_test": 70000}},
}


def make_scene(A, n, seed=0):
    """Clouds that thin out with distance (ground returns within ~60 m), a few points on the ego vehicle, poses a few metres apart."""
    rng = np.random.default_rng(seed)
    clouds, tfms = [], []
    for _ in range(A):
        r, phi = np.abs(rng.normal(0, 35, n)) + 1.0, rng.uniform(-np.pi, np.pi, n)
        p = np.stack([r * np.cos(phi), r * np.sin(phi), rng.normal(-1.6, 0.5, n), rng.uniform(0, 1, n)], axis=1)
        clouds.append(p.astype(np.float32))
        yaw = rng.uniform(-0.3, 0.3)
        t = np.eye(4)
        t[:2, :2], t[:3, 3] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]], (rng.uniform(-20, 20), rng.uniform(-8, 8), 0.05)
        tfms.append(t.astype(np.float32))
    return clouds, np.stack(tfms)


def loop_call(pp, clouds, tfms):
    batch = []
    for a, p in enumerate(clouds):
        keep = ~((p[:, 0] >= -1.95) & (p[:, 0] <= 2.95) & (p[:, 1] >= -1.1) & (p[:, 1] <= 1.1))
        p = p[keep]
        xyz = torch.nn.functional.pad(p[:, :3], (0, 1), value=1.0) @ tfms[a].T
        p = torch.cat([xyz[:, :3], p[:, 3:]], dim=1)
        v, c, k = pp.preprocess_device(p)
        batch.append((v.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy()))
    feats = np.concatenate([b[0] for b in batch])
    coords = np.concatenate([np.pad(b[1], ((0, 0), (1, 0)), mode="constant", constant_values=i) for i, b in enumerate(batch)])
    nums = np.concatenate([b[2] for b in batch])
    dev = clouds[0].device
    return {"voxel_features": torch.from_numpy(feats).to(dev), "voxel_coords": torch.from_numpy(coords).to(dev), "voxel_num_points": torch.from_numpy(nums).to(dev)}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters, (time.perf_counter() - t0) * 1e6 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--points", type=int, default=60000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--grid", choices=list(GRIDS) + ["all"], default="all")
    ap.add_argument("--only", choices=["batched", "loop"], default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel_batch_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    clouds_np, tfms_np = make_scene(a.agents, a.points)
    clouds, tfms = [torch.from_numpy(c).to(dev) for c in clouds_np], torch.from_numpy(tfms_np).to(dev)
    results = []
    for name in (GRIDS if a.grid == "all" else [a.grid]):
        pp = SpVoxelPreprocessor(GRIDS[name], train=False)
        F, mp = 4, int(pp.max_points_per_voxel)
        res = {"grid": name, "agents": a.agents, "points_per_agent": a.points, "max_points": mp, "max_voxels": int(pp.max_voxels)}
        if a.only != "loop":
            out = pp.preprocess_batch_device(clouds, transforms=tfms)
            m = int(out["voxel_coords"].shape[0])
            res["voxels"] = m
            res["batched_device_us"], _ = timed(lambda: pp.preprocess_batch_device(clouds, transforms=tfms, return_padded=True), a.iters, a.warmup)
            _, res["batched_wall_us"] = timed(lambda: pp.preprocess_batch_device(clouds, transforms=tfms), a.iters, a.warmup)
            nbytes = a.agents * a.points * F * 4 + m * (mp * F * 4 + 16 + 4)
            res["floor_bytes"] = nbytes
            res["floor_us"] = nbytes / (a.hbm_tbps * 1e12) * 1e6
            res["batched_device_times_floor"] = res["batched_device_us"] / res["floor_us"]
        if a.only != "batched":
            ref = loop_call(pp, clouds, tfms)
            res["loop_device_us"], res["loop_wall_us"] = timed(lambda: loop_call(pp, clouds, tfms), max(a.iters // 5, 1), min(a.warmup, 2))
            if a.only is None:
                res["loop_voxels"] = int(ref["voxel_coords"].shape[0])
                res["coords_equal"] = bool(torch.equal(ref["voxel_coords"], out["voxel_coords"]))     # the projections differ in rounding only
                res["wall_ratio_loop_over_batched"] = res["loop_wall_us"] / res["batched_wall_us"]
                res["device_ratio_loop_over_batched"] = res["loop_device_us"] / res["batched_device_us"]
        res = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in res.items()}
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "hbm_tbps": a.hbm_tbps, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
