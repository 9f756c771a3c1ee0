#!/usr/bin/env python3
"""Device time of the max fusion's backward (gencomm_warp_maxfuse_bwd) beside the attention fusion's backward
(gencomm_warp_attfuse_bwd) at the same shape on the same GPU, and beside the ATen autograd of the max restatement
(tests/fusion_train_restatement.py, float32, backward only). Per call: warm-up, then the mean over `--iters` calls enqueued back to
back between two events on the stream.

Shapes: one scene of 5 agents x 128 x 64 x 128 (the shipped map) and one of 4 x 64 x 200 x 704 (the metric shape); post-ReLU maps, the
rigid transforms of `synth.make_pairwise_t_matrix` (identity ego: every agent takes the deterministic paths in both kernels).
No absolute time is a target: the yardstick is the attention backward, which moves the same bytes and does more arithmetic, so the
ratio max / att is expected to be at most 1.

    python tools/fusion_train_bench.py [--iters 20] [--warmup 3] [--out profiles/fusion_train_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch

SHAPES = [(5, 128, 64, 128), (4, 64, 200, 704)]   # (agents, C, H, W), one scene each


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fusion_train_bench.json"))
    a = ap.parse_args()
    import fusion_train_restatement as R
    from gencomm_amd import _lib, normalize_pairwise_tfm, synth
    from gencomm_amd.fusion import gather_ego_thetas
    from gencomm_amd.runtime import dev_ints, ptr, stream_ptr
    dev = torch.device("cuda:0")
    l, st = _lib.lib(), stream_ptr(dev)
    results = []
    for n, C, H, W in SHAPES:
        inp = synth.make_inputs([n], C, H, W, 21, max_cav=5, max_shift=0.15 * W)
        affine = normalize_pairwise_tfm(torch.from_numpy(inp["pairwise_t_matrix"]), H * 0.8, W * 0.8, 1)
        x = torch.from_numpy(inp["feat"]).to(dev)
        g = torch.randn(1, C, H, W, device=dev)
        theta = gather_ego_thetas(affine, [n]).to(dev)
        off = dev_ints([0, n], dev)
        gx = torch.empty_like(x)
        s_att = torch.empty(_lib.check_size(l.gencomm_warp_attfuse_bwd_scratch_floats(n, H, W), "scratch"), device=dev)
        s_max = torch.empty(_lib.check_size(l.gencomm_warp_maxfuse_bwd_scratch_floats(1, n, C, H, W), "scratch"), device=dev)
        att = lambda: _lib.check(l.gencomm_warp_attfuse_bwd(ptr(x), ptr(theta), ptr(off), ptr(g), ptr(gx), ptr(s_att), 1, n, C, H, W, st), "att")
        mx = lambda: _lib.check(l.gencomm_warp_maxfuse_bwd(ptr(x), ptr(theta), ptr(off), ptr(g), ptr(gx), ptr(s_max), 1, n, C, H, W, st), "max")
        mx_scatter = lambda: _lib.check(l.gencomm_warp_maxfuse_bwd(ptr(x), ptr(theta), ptr(off), ptr(g), ptr(gx), None, 1, n, C, H, W, st), "max")
        t_att, t_max = device_us(att, a.iters, a.warmup), device_us(mx, a.iters, a.warmup)
        t_att2, t_max2 = device_us(att, a.iters, 1), device_us(mx, a.iters, 1)          # alternated once more: the spread of the pair
        t_scatter = device_us(mx_scatter, a.iters, a.warmup)
        xg = x.clone().requires_grad_(True)
        out = R.max_fusion_forward(xg, [n], affine.to(dev))
        t_aten = device_us(lambda: torch.autograd.grad(out, xg, g, retain_graph=True), a.iters, a.warmup)
        res = {"agents": n, "C": C, "map": f"{H}x{W}", "algorithmic_bytes": (2 * n * C * H * W + C * H * W) * 4,
               "attfuse_bwd_us": [round(t_att, 1), round(t_att2, 1)], "maxfuse_bwd_us": [round(t_max, 1), round(t_max2, 1)],
               "ratio_max_over_att": round(min(t_max, t_max2) / min(t_att, t_att2), 3),
               "maxfuse_bwd_scatter_only_us": round(t_scatter, 1), "aten_autograd_restatement_bwd_us": round(t_aten, 1)}
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "src": _lib.library_src_hash(), "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
