#!/usr/bin/env python3
"""PyramidFusion TRAINING timing at the shipped shape: 5 agents in one scene, input 64 x 128 x 256, num_filters [64, 128, 256],
layer_nums [3, 5, 8], resnext true -- against torch autograd in float32 on the same GPU. Device time between two events on the
stream, as tools/bench_pyramid.py measures it (warm-up of every shape, then `--reps` rounds of `--iters` calls of each function in
turn; the median window is reported with the fastest and slowest beside it). One process; the copy bandwidth is measured in it.

Reported:
  copy_gbps     MEASURED HBM copy bandwidth (512 MiB float32 tensor, bytes read + bytes written)
  gconv[...]    per group width and stride: dgrad_us (pack + [spread] + the forward tile kernel on dy) and wgrad_us (partials + ordered
                sum), the floor bytes of each (dgrad: dy read + dx written; wgrad: x + dy read), the bandwidth that gives and its
                fraction of copy_gbps, and torch's F.conv2d(groups=32) backward on the same tensors: torch_us times
                torch.autograd.grad for BOTH gradients, so torch_over_hip = torch_us / (dgrad_us + wgrad_us)
  head_fuse[...]  per level: head_us = gencomm_pyramid_score_bwd (dx, dw, db from d_occ and d_score) against torch autograd of conv1x1 +
                sigmoid (forward included in torch's figure); fuse_us = gencomm_warp_weightfuse_bwd (2 launches) against torch autograd
                of the restatement's weighted_fuse (its forward measured separately and taken out)
  step          forward_collab + backward of every parameter and the input in train() mode, and the frozen dx-only step in eval(),
                each with the peak allocated memory, against torch autograd of the float32 restatement

    python tools/bench_pyramid_train.py [--iters 5] [--reps 5] [--warmup 2] [--out profiles/pyramid_train_bench.json]
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
import torch.nn.functional as F

from bench_pyramid import AGENTS, CIN, H, LAYER_NUMS, W, alternate, stats


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pyramid_train_bench.json"))
    a = ap.parse_args()
    import pyramid_restatement as R
    import pyramid_train_restatement as TR
    from gencomm_amd import PyramidFusion, _lib
    from gencomm_amd import pyramid_bwd as PB
    if not torch.cuda.is_available():
        raise SystemExit("bench_pyramid_train needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup,
           "shape": {"agents": AGENTS, "scenes": 1, "input": [CIN, H, W], "layer_nums": list(LAYER_NUMS)}}
    src = torch.empty(128 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    w = alternate({"copy": lambda: dst.copy_(src)}, a.iters, a.reps, a.warmup)["copy"]
    copy_gbps = 2 * src.numel() * 4 / statistics.median(w) / 1e3
    out["copy_gbps"] = round(copy_gbps, 1)
    del src, dst
    print(json.dumps({"copy_gbps": out["copy_gbps"]}), flush=True)
    rng = np.random.RandomState(7)

    def rand(*shape):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)

    # ---- the grouped layer's two gradients, per width and stride
    out["gconv"] = []
    for level, cpg in enumerate((4, 8, 16)):
        C = 32 * cpg
        h, w_ = H >> level, W >> level
        for stride in ((1,) if level == 0 else (1, 2)):
            hin, win = (h, w_) if stride == 1 else (2 * h, 2 * w_)
            xi, dy = rand(AGENTS, C, hin, win), rand(AGENTS, C, h, w_)
            wt = (rand(C, cpg, 3, 3) / np.sqrt(9 * cpg)).contiguous()
            xg, wg = xi.clone().requires_grad_(True), wt.clone().requires_grad_(True)

            def torch_bwd():
                return torch.autograd.grad(F.conv2d(xg, wg, None, stride, 1, 1, 32), (xg, wg), dy)

            def torch_fwd():
                with torch.no_grad():
                    return F.conv2d(xi, wt, None, stride, 1, 1, 32)

            fns = {"dgrad_us": lambda: PB.gconv3x3_dgrad(dy, wt, cpg, stride, (hin, win)), "wgrad_us": lambda: PB.gconv3x3_wgrad(xi, dy, cpg, stride),
                   "torch_fwd_bwd_us": torch_bwd, "torch_fwd_us": torch_fwd}
            t = alternate(fns, a.iters, a.reps, a.warmup)
            res = {"cpg": cpg, "C": C, "stride": stride, "in": [hin, win], "out": [h, w_]}
            for k in fns:
                stats(res, k, t[k])
            res["torch_us"] = round(res["torch_fwd_bwd_us"] - res["torch_fwd_us"], 1)      # autograd.grad needs its own forward: taken out
            res["dgrad_bytes"], res["wgrad_bytes"] = 4 * AGENTS * C * (hin * win + h * w_), 4 * AGENTS * C * (hin * win + h * w_)
            for k in ("dgrad", "wgrad"):
                res[k + "_gbps"] = round(res[k + "_bytes"] / res[k + "_us"] / 1e3, 1)
                res[k + "_fraction_of_copy"] = round(res[k + "_gbps"] / copy_gbps, 3)
            res["torch_over_hip"] = round(res["torch_us"] / (res["dgrad_us"] + res["wgrad_us"]), 2)
            gx, gw = torch_bwd()
            res["dgrad_max_abs_diff"] = float((PB.gconv3x3_dgrad(dy, wt, cpg, stride, (hin, win)) - gx).abs().max())
            res["wgrad_max_rel_diff"] = float((PB.gconv3x3_wgrad(xi, dy, cpg, stride) - gw).abs().max() / gw.abs().max())
            print(json.dumps(res), flush=True)
            out["gconv"].append(res)
            del xi, dy, xg

    cfg = R.cfg(layer_nums=LAYER_NUMS)
    torch.manual_seed(0)
    model = R.fill_params_(PyramidFusion(cfg, trainable=True)).to(dev)
    ref = R.fill_params_(TR.PyramidTrainRestatement(cfg)).to(dev)
    x = rand(AGENTS, CIN, H, W)
    scene = [R.theta(H, W)] + [R.rot(H, W, rng.uniform(-0.6, 0.6), rng.uniform(-40, 40) + 0.37, rng.uniform(-20, 20) + 0.41) for _ in range(AGENTS - 1)]
    aff = torch.from_numpy(R.affine_of([scene], L=5)).to(dev)
    rl = [AGENTS]

    # ---- head and fuse backward per level
    from gencomm_amd.fusion import gather_ego_thetas
    from gencomm_amd.runtime import dev_ints
    with torch.no_grad():
        feats = [f.clone() for f in model.eval().get_multiscale_feature(x)]
    theta, off = gather_ego_thetas(aff, rl).to(dev), dev_ints([0, AGENTS], dev)
    out["head_fuse"] = []
    for i, f in enumerate(feats):
        head = getattr(model, f"single_head_{i}")
        n, C, h, w_ = f.shape
        wv, bv = head.weight.detach().clone(), head.bias.detach().clone()
        with torch.no_grad():
            occ = F.conv2d(f, wv, bv)
            score = torch.sigmoid(occ) + 1e-4
        d_occ, d_sc, dout = rand(n, 1, h, w_), rand(n, 1, h, w_), rand(1, C, h, w_)
        fg, wg, bg, sg = f.clone().requires_grad_(True), wv.clone().requires_grad_(True), bv.clone().requires_grad_(True), score.clone().requires_grad_(True)

        def torch_head():
            o = F.conv2d(fg, wg, bg)
            return torch.autograd.grad([o, torch.sigmoid(o) + 1e-4], (fg, wg, bg), [d_occ, d_sc])

        def torch_fuse():
            return torch.autograd.grad(R.weighted_fuse(fg, sg, rl, aff), (fg, sg), dout)

        def torch_fuse_fwd():
            with torch.no_grad():
                return R.weighted_fuse(f, score, rl, aff)

        fns = {"head_us": lambda: PB.score_head_bwd(f, wv, occ, None, d_occ, d_sc, True, True), "head_torch_us": torch_head,
               "fuse_us": lambda: PB.weighted_fuse_bwd(f, score, theta, off, dout, 1), "fuse_torch_fwd_bwd_us": torch_fuse, "fuse_torch_fwd_us": torch_fuse_fwd}
        t = alternate(fns, a.iters, a.reps, a.warmup)
        res = {"level": i, "map": [C, h, w_]}
        for k in fns:
            stats(res, k, t[k])
        res["fuse_torch_us"] = round(res["fuse_torch_fwd_bwd_us"] - res["fuse_torch_fwd_us"], 1)
        res["head_torch_over_hip"] = round(res["head_torch_us"] / res["head_us"], 2)       # torch's figure includes the head's forward
        res["fuse_torch_over_hip"] = round(res["fuse_torch_us"] / res["fuse_us"], 2)
        res["fuse_bytes"] = 4 * (2 * AGENTS + 1) * C * h * w_                              # x read, dx written, dout read
        res["fuse_gbps"] = round(res["fuse_bytes"] / res["fuse_us"] / 1e3, 1)
        gx, gs = torch_fuse()
        dx, ds = PB.weighted_fuse_bwd(f, score, theta, off, dout, 1)
        res["fuse_dx_max_abs_diff"], res["fuse_dscore_max_abs_diff"] = float((dx - gx).abs().max()), float((ds - gs).abs().max())
        print(json.dumps(res), flush=True)
        out["head_fuse"].append(res)
    del feats

    # ---- whole steps
    g = rand(1, 384, H, W)

    def step(m, frozen):
        m.train(not frozen)
        for p in m.parameters():
            p.requires_grad_(not frozen)
            p.grad = None
        xg = x.clone().requires_grad_(True)
        fused, occs = m.forward_collab(xg, rl, aff)
        ((fused * g).sum() + sum(o.sum() for o in occs)).backward()
        return xg.grad

    out["step"] = {}
    for name, frozen in (("train", False), ("frozen", True)):
        fns = {"us": lambda: step(model, frozen), "torch_us": lambda: step(ref, frozen)}
        t = alternate(fns, max(a.iters // 2, 1), a.reps, a.warmup)
        res = {}
        for k in fns:
            stats(res, k, t[k])
        res["torch_over_hip"] = round(res["torch_us"] / res["us"], 2)
        res["peak_mib"], res["torch_peak_mib"] = peak_mib(fns["us"]), peak_mib(fns["torch_us"])
        d, r = step(model, frozen), step(ref, frozen)
        res["dx_rel_rms_vs_torch"] = float((d - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt())
        print(json.dumps({name: res}), flush=True)
        out["step"][name] = res

    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
