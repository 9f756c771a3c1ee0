#!/usr/bin/env python3
"""PyramidFusion timing at the shipped shape: 5 agents in one scene, input 64 x 128 x 256, num_filters [64, 128, 256],
layer_nums [3, 5, 8], resnext true -- against torch in float32 on the same GPU. Device time between two events on the stream: warm-up
of every shape, then `--reps` rounds; a round times a window of `--iters` calls of each function in turn, so that all see the same
clocks and neighbours. The median window is reported with the fastest and slowest beside it. One process.

Reported:
  copy_gbps           MEASURED HBM copy bandwidth: a 512 MiB float32 tensor copied with Tensor.copy_ (bytes read + bytes written) / time
  gconv[...]          per group width (4 / 8 / 16 channels per group = level 0 / 1 / 2) and stride: one launch of gencomm_gconv3x3_fwd
                      on the layer's map (us), the bytes it must move (input + output, 4 B each; the weights are noise), the bandwidth that
                      gives and its fraction of copy_gbps, and torch's F.conv2d(groups=32) + folded-BatchNorm-free bare convolution on
                      the same tensors (torch_us; torch_over_hip = torch_us / us). The HIP figure includes scale, shift and ReLU, torch's does
                      not.
  fuse[...]           per level: gencomm_pyramid_score_fwd + gencomm_warp_weightfuse_fwd (us, 2 launches) against the restatement's chain
                      (1x1 head, sigmoid, two affine_grid + grid_sample, masked_fill, softmax, where, multiply, sum) in torch float32
  collab              the whole PyramidFusion.forward_collab against the restatement in torch float32, with the launch counts of both
                      (torch.profiler)

    python tools/bench_pyramid.py [--iters 10] [--reps 7] [--warmup 3] [--out profiles/pyramid_bench.json]
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

import numpy as np
import torch
import torch.nn.functional as F

AGENTS, CIN, H, W = 5, 64, 128, 256
LAYER_NUMS = (3, 5, 8)


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, iters, reps, warmup):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(window_us(fn, iters))
    return out


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as exc:   # noqa: BLE001 -- a diagnostic figure: report why it is missing instead of failing the timing run
        print(f"kernel count not available: {exc}", file=sys.stderr)
        return None


def stats(res, key, w):
    res[key], res[key + "_min"], res[key + "_max"] = round(statistics.median(w), 1), round(min(w), 1), round(max(w), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pyramid_bench.json"))
    a = ap.parse_args()
    import pyramid_restatement as R
    from gencomm_amd import PyramidFusion, _lib, weighted_fuse
    from gencomm_amd.bev_backbone import gconv3x3_hip
    from gencomm_amd.pyramid_fuse import score_head
    if not torch.cuda.is_available():
        raise SystemExit("bench_pyramid needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True      # let torch's grouped convolution pick its best algorithm
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup,
           "shape": {"agents": AGENTS, "scenes": 1, "input": [CIN, H, W], "layer_nums": list(LAYER_NUMS)}}

    # ---- measured copy bandwidth
    src = torch.empty(128 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    w = alternate({"copy": lambda: dst.copy_(src)}, a.iters, a.reps, a.warmup)["copy"]
    copy_gbps = 2 * src.numel() * 4 / statistics.median(w) / 1e3
    out["copy_gbps"] = round(copy_gbps, 1)
    del src, dst
    print(json.dumps({"copy_gbps": out["copy_gbps"]}), flush=True)

    cfg = R.cfg(layer_nums=LAYER_NUMS)
    model = R.fill_params_(PyramidFusion(cfg).eval()).to(dev)
    ref = R.fill_params_(R.PyramidRestatement(cfg).eval()).to(dev)
    for p in list(model.parameters()) + list(ref.parameters()):
        p.requires_grad_(False)
    rng = np.random.RandomState(7)
    x = torch.from_numpy(rng.standard_normal((AGENTS, CIN, H, W)).astype(np.float32)).to(dev)
    scene = [R.theta(H, W)] + [R.rot(H, W, rng.uniform(-0.6, 0.6), rng.uniform(-40, 40) + 0.37, rng.uniform(-20, 20) + 0.41) for _ in range(AGENTS - 1)]
    aff = torch.from_numpy(R.affine_of([scene], L=5)).to(dev)
    rl = [AGENTS]

    with torch.no_grad():
        # ---- the grouped layer, per width and stride
        out["gconv"] = []
        for level, cpg in enumerate((4, 8, 16)):
            C = 32 * cpg
            h, w_ = H >> level, W >> level
            for stride in ((1,) if level == 0 else (1, 2)):
                hin, win = (h, w_) if stride == 1 else (2 * h, 2 * w_)
                blk = getattr(model.resnet, f"layer{level}")[1 if stride == 1 else 0]
                conv, bn = blk.conv2, blk.bn2
                assert conv.stride == (stride, stride) and conv.in_channels == C
                xi = torch.from_numpy(rng.standard_normal((AGENTS, C, hin, win)).astype(np.float32)).to(dev)
                wt = conv.weight.detach()
                fns = {"us": lambda: gconv3x3_hip(xi, conv, bn, relu=True), "torch_us": lambda: F.conv2d(xi, wt, None, stride, 1, 1, 32)}
                t = alternate(fns, a.iters, a.reps, a.warmup)
                res = {"cpg": cpg, "C": C, "stride": stride, "in": [hin, win], "out": [h, w_]}
                for k in fns:
                    stats(res, k, t[k])
                res["bytes"] = 4 * AGENTS * C * (hin * win + h * w_)
                res["gbps"] = round(res["bytes"] / res["us"] / 1e3, 1)
                res["fraction_of_copy"] = round(res["gbps"] / copy_gbps, 3)
                res["gflop"] = round(2 * 9 * cpg * AGENTS * C * h * w_ / 1e9, 3)
                res["tflops"] = round(res["gflop"] / res["us"] * 1e3, 2)
                res["torch_over_hip"] = round(res["torch_us"] / res["us"], 2)
                bnf = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).view(1, -1, 1, 1)
                want = torch.relu((F.conv2d(xi, wt, None, stride, 1, 1, 32) - bn.running_mean.view(1, -1, 1, 1)) * bnf + bn.bias.view(1, -1, 1, 1))
                res["max_abs_diff"] = float((gconv3x3_hip(xi, conv, bn, relu=True) - want).abs().max())
                print(json.dumps(res), flush=True)
                out["gconv"].append(res)
                del xi

        # ---- score head + weighted fuse per level
        feats = model.get_multiscale_feature(x)
        out["fuse"] = []
        for i, f in enumerate(feats):
            head, rhead = getattr(model, f"single_head_{i}"), getattr(ref, f"single_head_{i}")

            def hip(f=f, head=head):
                _, s = score_head(f, head)
                return weighted_fuse(f, s, rl, aff, False)

            def chain(f=f, rhead=rhead):
                return R.weighted_fuse(f, torch.sigmoid(rhead(f)) + 1e-4, rl, aff)

            fns = {"us": hip, "torch_us": chain}
            t = alternate(fns, a.iters, a.reps, a.warmup)
            res = {"level": i, "map": list(f.shape[1:])}
            for k in fns:
                stats(res, k, t[k])
            res["launches"], res["torch_launches"] = count_kernels(hip), count_kernels(chain)
            res["bytes"] = 4 * (AGENTS + 1) * f.shape[1] * f.shape[2] * f.shape[3]      # every agent map read once, the fused map written once
            res["gbps"] = round(res["bytes"] / res["us"] / 1e3, 1)
            res["torch_over_hip"] = round(res["torch_us"] / res["us"], 2)
            res["max_abs_diff"] = float((hip() - chain()).abs().max())
            print(json.dumps(res), flush=True)
            out["fuse"].append(res)
        del feats

        # ---- the whole forward_collab
        fns = {"us": lambda: model.forward_collab(x, rl, aff), "torch_us": lambda: ref.forward_collab(x, rl, aff)}
        t = alternate(fns, max(a.iters // 2, 1), a.reps, a.warmup)
        res = {}
        for k in fns:
            stats(res, k, t[k])
        res["launches"], res["torch_launches"] = count_kernels(fns["us"]), count_kernels(fns["torch_us"])
        got, _ = model.forward_collab(x, rl, aff)
        res["torch_over_hip"] = round(res["torch_us"] / res["us"], 2)
        want, _ = ref.forward_collab(x, rl, aff)
        res["max_abs_diff"], res["max_abs_ref"] = float((got - want).abs().max()), float(want.abs().max())
        print(json.dumps(res), flush=True)
        out["collab"] = res

    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
