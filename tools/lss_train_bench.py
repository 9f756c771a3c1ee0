#!/usr/bin/env python3
"""Training the Lift-Splat-Shoot camera encoder, timing at the m4 shape (4 agents x 4 cameras, 336 x 448 images, D = 48 LID bins,
C = 128, the shipped 256 x 256 grid):

  * gencomm_lss_splat_bwd alone (its two kernels; per kernel from a `rocprofv3 --kernel-trace --stats` run of this script, --profile),
  * the encoder's forward + backward (LiftSplatShoot(trainable=True).train(), L = <G, bev> + depth loss),
  * the ATen autograd of the dense restatement (softmax, the lifted depth (x) feature rows scattered with index_add, its backward)
    on the same box.

    python tools/lss_train_bench.py [--iters 20] [--warmup 5]            # timings -> profiles/lss_train_bench.json
    python tools/lss_train_bench.py --profile                            # + per-kernel csv beside it (starts rocprofv3 on --kernels-only)

Timing is the mean between two stream events around `iters` back-to-back calls after warm-up. Per agent = per-batch time / 4.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np
import torch

from gencomm_amd import synth
from gencomm_amd.lift_splat_shoot import LiftSplatShoot
from gencomm_amd.point_pillar_gencomm_loss import depth_term
from lss_bench import cameras, m4_args

OUT = os.path.join(REPO, "profiles")
FWD_SPLAT_US_PER_AGENT = 237.0   # the forward splat stage on record


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / iters * 1e3   # us


def aten_dense(logit, feat, flat, pt, pix, ncell):
    prob = logit.softmax(1).reshape(-1)
    rows = feat.permute(0, 2, 3, 1).reshape(-1, feat.shape[1])
    return torch.zeros(ncell, feat.shape[1], device=feat.device).index_add(0, flat, prob[pt][:, None] * rows[pix])


def setup(dev):
    B, N, H, W = 4, 4, 336, 448
    m = LiftSplatShoot(m4_args(), trainable=True).train()
    synth.fill_params_(m, 0)
    synth.fill_running_stats_(m, 0)
    m = m.to(dev)
    rng = np.random.RandomState(0)
    imgs = torch.from_numpy(rng.standard_normal((B, N, 4, H, W)).astype(np.float32)).to(dev)
    imgs[:, :, 3] = imgs[:, :, 3].abs() * 20
    cams = cameras(B, N, dev)
    D, fH, fW, C = 48, 42, 56, 128
    logit = torch.from_numpy((2 * rng.standard_normal((B * N, D, fH, fW))).astype(np.float32)).to(dev)
    feat = torch.from_numpy(rng.standard_normal((B * N, C, fH, fW)).astype(np.float32)).to(dev)
    G = torch.from_numpy(rng.standard_normal((B, C, 256, 256)).astype(np.float32)).to(dev)
    return m, imgs, cams, logit, feat, G, (B, N, D, fH, fW, C)


def splat_backward_only(m, cams, logit, feat, G):
    lg, ft = logit.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    out = m.splat_grad(lg, ft, *cams)
    return lambda: torch.autograd.grad(out, (lg, ft), G, retain_graph=True)


def kernel_stats(a):
    """rocprofv3 --kernel-trace --stats around `--kernels-only` (a fresh child process); the csv goes beside the json."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="lss_train_prof_")
    cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "lss_train", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
           "--kernels-only", "--iters", str(a.iters), "--warmup", str(a.warmup)]
    subprocess.run(cmd, check=True, timeout=600)
    found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {tmp}")
    dst = os.path.join(OUT, "lss_train_kernel_stats.csv")
    rows = [r for r in csv.DictReader(open(found[0])) if "lss_" in r.get("Name", "")]
    with open(dst, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()) if rows else ["Name"])
        w.writeheader()
        w.writerows(rows)
    shutil.rmtree(tmp, ignore_errors=True)
    return {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3} for r in rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="run only the splat backward (the child of --profile)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m, imgs, cams, logit, feat, G, (B, N, D, fH, fW, C) = setup(dev)
    bwd = splat_backward_only(m, cams, logit, feat, G)
    if a.kernels_only:
        timed(bwd, a.iters, a.warmup)
        return
    bwd_us = timed(bwd, a.iters, a.warmup)
    with torch.no_grad():
        fwd_us = timed(lambda: m.splat(logit, feat, *cams), a.iters, a.warmup)
        _, cell = m.splat(logit, feat, *cams, return_cells=True)

    inp = {"inputs_m4": dict(zip(("imgs", "rots", "trans", "intrins", "post_rots", "post_trans"), [imgs] + cams))}
    params = [p for p in m.parameters()]

    def step():
        bev = m(inp, "m4")
        loss = (bev * G).sum() + depth_term({"depth_items": m.depth_items}, "", {"weight": 1.0})
        torch.autograd.grad(loss, params)

    def forward_only():
        with torch.no_grad():
            m(inp, "m4")

    step_us = timed(step, max(3, a.iters // 4), 2)
    enc_fwd_us = timed(forward_only, max(3, a.iters // 4), 2)

    # ATen autograd of the dense restatement on the kernel's own cells
    cell = cell.long()
    pt = torch.nonzero(cell >= 0)[:, 0]
    r = cell[pt]
    flat = ((r % B) * 256 + (r // B) % 256) * 256 + r // (B * 256)     # nz = 1: (b, y, x)
    HW = fH * fW
    pix = (pt // (D * HW)) * HW + pt % HW
    Gr = G.view(B, C, -1).permute(0, 2, 1).reshape(-1, C).contiguous()

    def aten_step():
        lg, ft = logit.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        torch.autograd.grad(aten_dense(lg, ft, flat, pt, pix, B * 256 * 256), (lg, ft), Gr)

    def aten_fwd():
        with torch.no_grad():
            aten_dense(logit, feat, flat, pt, pix, B * 256 * 256)

    aten_us = timed(aten_step, max(3, a.iters // 4), 2) - timed(aten_fwd, max(3, a.iters // 4), 2)
    # agreement
    lg, ft = logit.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    ga = torch.autograd.grad(aten_dense(lg, ft, flat, pt, pix, B * 256 * 256), (lg, ft), Gr)
    gh = bwd()
    diff = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(gh, ga)]

    npts, inside = B * N * D * HW, int(pt.numel())
    # bytes per agent: grad_out read + cell-major copy written; one 4 C-byte row gather per frustum point inside the grid (through L2);
    # prob + cell + feature rows read; the two outputs written
    hbm = (2 * C * 256 * 256 * 4 * B + npts * 8 + B * N * HW * C * 4 * 2 + npts * 4) / B
    gather = inside * C * 4 / B
    floor_hbm_us = hbm / 6.0e12 * 1e6                    # 6 TB/s: the achievable HBM rate DESIGN.md prices the forward with
    res = {"shape": "m4 4 agents x 4 cams 336x448 D48 C128", "splat_bwd_us": bwd_us, "splat_bwd_us_per_agent": bwd_us / B,
           "splat_fwd_us_per_agent": fwd_us / B, "ratio_to_fwd_splat_on_record": bwd_us / B / FWD_SPLAT_US_PER_AGENT,
           "encoder_fwd_bwd_us_per_agent": step_us / B, "encoder_fwd_us_per_agent": enc_fwd_us / B,
           "aten_dense_bwd_us_per_agent": aten_us / B, "speedup_vs_aten": aten_us / bwd_us,
           "points": npts, "points_inside": inside, "hbm_MB_per_agent": hbm / 1e6, "l2_gather_MB_per_agent": gather / 1e6,
           "hbm_floor_us_per_agent": floor_hbm_us, "ratio_to_hbm_floor": bwd_us / B / floor_hbm_us,
           "max_rel_diff_vs_aten": {"d_logit": diff[0], "d_feat": diff[1]}}
    os.makedirs(OUT, exist_ok=True)

    def write():
        with open(os.path.join(OUT, "lss_train_bench.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    write()                      # the timings are kept even if the profiler run below fails
    if a.profile:
        res["kernels"] = kernel_stats(a)
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
