#!/usr/bin/env python3
"""Lift-Splat-Shoot camera encoder timing at the m4 shape (4 agents x 4 cameras, 336 x 448 images, D = 48 LID bins, C = 128, the
shipped 256 x 256 grid): the whole encoder forward, the splat stage alone (gencomm_lss_splat_fwd: softmax + geometry + sort + splat),
and an ATen restatement of the same stage (softmax, get_geometry, the lifted depth (x) feature tensor, voxel_pooling with
QuickCumsum, heter_encoders.py:123-205 / camera_utils.py:218-246, written here from the formulas) on the same box.

    python tools/lss_bench.py [--iters 20] [--warmup 5]

Prints one JSON line. Per agent = per-batch time / 4.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gencomm_amd import synth
from gencomm_amd.lift_splat_shoot import LiftSplatShoot


def m4_args():
    return {"grid_conf": {"xbound": [-51.2, 51.2, 0.4], "ybound": [-51.2, 51.2, 0.4], "zbound": [-10, 10, 20.0], "ddiscr": [2, 50, 48], "mode": "LID"},
            "data_aug_conf": {"final_dim": [336, 448], "H": 600, "W": 800, "Ncams": 4},
            "img_downsample": 8, "img_features": 128, "use_depth_gt": False, "depth_supervision": True, "camera_encoder": "Resnet101"}


def cameras(B, N, dev):
    base = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)
    rots, trans = np.zeros((B, N, 3, 3)), np.zeros((B, N, 3))
    for n in range(N):
        y = math.radians(90.0 * n)
        rots[:, n] = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]]) @ base
        trans[:, n] = [0.5 * math.cos(y), 0.5 * math.sin(y), 1.7]
    intrins = np.tile(np.array([[400.0, 0, 400], [0, 400.0, 300], [0, 0, 1]]), (B, N, 1, 1))
    s = 0.58
    post_rots = np.tile(np.diag([s, s, 1.0]), (B, N, 1, 1))
    post_trans = np.tile(np.array([-(800 * s - 448) / 2, -(600 * s - 336), 0.0]), (B, N, 1))
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    return [t(a) for a in (rots, trans, intrins, post_rots, post_trans)]


def aten_splat(m, depth_logit, feat, rots, trans, intrins, post_rots, post_trans):
    """The reference's splat stage restated in ATen: softmax, get_geometry, lift (the D x C outer product), voxel_pooling + QuickCumsum."""
    B, N = trans.shape[:2]
    fr = m._dev_frustum[feat.device]
    D, fH, fW = fr.shape[:3]
    C = feat.shape[1]
    depth = depth_logit.softmax(1)
    x = (depth.unsqueeze(1) * feat.unsqueeze(2)).view(B, N, C, D, fH, fW).permute(0, 1, 3, 4, 5, 2)
    p = fr - post_trans.view(B, N, 1, 1, 1, 3)
    p = torch.inverse(post_rots).view(B, N, 1, 1, 1, 3, 3).matmul(p.unsqueeze(-1))
    p = torch.cat((p[..., :2, :] * p[..., 2:3, :], p[..., 2:3, :]), 5)
    p = rots.matmul(torch.inverse(intrins)).view(B, N, 1, 1, 1, 3, 3).matmul(p).squeeze(-1) + trans.view(B, N, 1, 1, 1, 3)
    dx, bx, nx = m.dx.to(feat.device), m.bx.to(feat.device), [int(v) for v in m.nx]
    Np = B * N * D * fH * fW
    x = x.reshape(Np, C)
    g = ((p - (bx - dx / 2.)) / dx).long().view(Np, 3)
    b = torch.arange(B, device=feat.device).repeat_interleave(Np // B).view(-1, 1)
    g = torch.cat((g, b), 1)
    kept = (g[:, 0] >= 0) & (g[:, 0] < nx[0]) & (g[:, 1] >= 0) & (g[:, 1] < nx[1]) & (g[:, 2] >= 0) & (g[:, 2] < nx[2])
    x, g = x[kept], g[kept]
    ranks = g[:, 0] * (nx[1] * nx[2] * B) + g[:, 1] * (nx[2] * B) + g[:, 2] * B + g[:, 3]
    s = ranks.argsort()
    x, g, ranks = x[s], g[s], ranks[s]
    x = x.cumsum(0)
    keep = torch.ones(x.shape[0], device=x.device, dtype=torch.bool)
    keep[:-1] = ranks[1:] != ranks[:-1]
    x, g = x[keep], g[keep]
    x = torch.cat((x[:1], x[1:] - x[:-1]))
    final = torch.zeros((B, C, nx[2], nx[1], nx[0]), device=x.device)
    final[g[:, 3], :, g[:, 2], g[:, 1], g[:, 0]] = x
    return torch.cat(final.unbind(dim=2), 1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(iters):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms)) * 1e3   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N, H, W = 4, 4, 336, 448
    m = LiftSplatShoot(m4_args()).eval()
    synth.fill_params_(m, 0)
    synth.fill_running_stats_(m, 0)
    m = m.to(dev)
    rng = np.random.RandomState(0)
    imgs = torch.from_numpy(rng.standard_normal((B, N, 4, H, W)).astype(np.float32)).to(dev)
    imgs[:, :, 3] = imgs[:, :, 3].abs() * 20
    cams = cameras(B, N, dev)
    inp = {"inputs_m4": dict(zip(("imgs", "rots", "trans", "intrins", "post_rots", "post_trans"), [imgs] + cams))}
    with torch.no_grad():
        enc_us = timed(lambda: m(inp, "m4"), a.iters, a.warmup)
        depth_logit, feat = m.camencode(imgs.view(B * N, 4, H, W)[:, :3].contiguous())
        out, cell = m.splat(depth_logit, feat, *cams, return_cells=True)
        splat_us = timed(lambda: m.splat(depth_logit, feat, *cams), a.iters, a.warmup)
        ref = aten_splat(m, depth_logit, feat, *cams)
        aten_us = timed(lambda: aten_splat(m, depth_logit, feat, *cams), max(3, a.iters // 4), 2)
    torch.cuda.synchronize()
    err = float((out - ref).abs().max() / ref.abs().max())
    D, fH, fW, C = 48, 42, 56, 128
    npts = B * N * D * fH * fW
    inside = int((cell >= 0).sum())
    # HBM floor of the splat stage: logits + features read once, featT / prob / keys written and read, the BEV map written
    floor = (B * N * D * fH * fW * 4 + B * N * C * fH * fW * 4 * 3 + npts * 4 * 2 + npts * 16 + out.numel() * 4)
    gather = inside * (C * 4 + 8)   # one C-float row + prob + point index per kept point (L2 / MALL traffic)
    res = {"shape": "m4 4 agents x 4 cams 336x448 D48 C128", "encoder_us": enc_us, "encoder_us_per_agent": enc_us / B,
           "splat_us": splat_us, "splat_us_per_agent": splat_us / B, "aten_splat_us": aten_us, "aten_splat_us_per_agent": aten_us / B,
           "speedup_vs_aten": aten_us / splat_us, "points": npts, "points_inside": inside,
           "hbm_floor_MB_per_agent": floor / B / 1e6, "l2_gather_MB_per_agent": gather / B / 1e6,
           "max_rel_diff_vs_aten": err}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
