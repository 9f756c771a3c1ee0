#!/usr/bin/env python3
"""STAMP adapter timing: the fused ConvNeXt block and the whole ``Adapter`` (adapterconvnext, 3 blocks) at the two shipped
configurations -- in 128 / dim 64 and in 256 / dim 128 -- on 5 agents x 128 x 256, against the torch restatement
(tests/stamp_adapter_restatement.py) in float32 on the same GPU. Device time between two events on the stream: warm-up of every shape,
then `--reps` rounds; a round times a window of `--iters` calls of the fused adapter, then one of the torch restatement, alternating, so
that both see the same clocks and neighbours. The median window is reported with the fastest and slowest beside it. One process.

Reported per configuration:
  block_us            one launch of gencomm_convnext_block_fwd on the [5, dim, 128, 256] map
  block_floor_us      DERIVED, not measured: the FLOP of the block's two Linears (pixels x 2 x 2 x dim x 4 dim) at `--fp32-matrix-tflops`
                      (default 155, the exact-fp32 MFMA rate of the MI355X); block_times_floor = block_us / block_floor_us
  adapter_us          Adapter.forward: 1x1 convolution, 3 block launches, 1x1 convolution; adapter_launches from torch.profiler
  torch_us            the restatement of the same adapter with torch in float32 (its [pixels, 4 dim] hidden tensor goes to memory twice per
                      block); torch_launches; torch_over_fused = torch_us / adapter_us
  torch_block_us      the restatement of one block alone, and torch_block_over_fused
  max_abs_diff        fused against torch float32 on the timed input (a sanity figure; the tests hold the tolerance against float64)

    python tools/stamp_adapter_bench.py [--iters 20] [--reps 7] [--warmup 5] [--out profiles/stamp_adapter_bench.json]

Prints one JSON line per configuration and writes them all to --out.
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

import torch

CONFIGS = [("in128_dim64", 128, 64), ("in256_dim128", 256, 128)]
AGENTS, H, W = 5, 128, 256


def window_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, iters, reps, warmup):
    """{name: [window us per round]}: every round times each function once, in the given order."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fp32-matrix-tflops", type=float, default=155.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stamp_adapter_bench.json"))
    a = ap.parse_args()
    import stamp_adapter_restatement as R
    from gencomm_amd import Adapter, _lib
    from gencomm_amd.stamp_adapter import convnext_block
    if not torch.cuda.is_available():
        raise SystemExit("stamp_adapter_bench needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    order = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias", "gamma")
    results = []
    for key, cin, dim in CONFIGS:
        cfg = R.SHIPPED[key]
        sd = R.make_params(cfg, "adapter", 51, R.STD if dim == 64 else R.STD_WIDE)
        mod = Adapter(cfg)
        mod.load_state_dict(sd, strict=True)
        mod = mod.to(dev).eval()
        x = R.make_x((AGENTS, cin, H, W), 52).to(dev)
        xb = 2.0 * R.make_x((AGENTS, dim, H, W), 53).to(dev)
        sdd = {k: v.to(dev) for k, v in sd.items()}
        bp = R.block_params(sdd, "adapter", 0)
        bargs = [bp[k] for k in order]
        yb = torch.empty_like(xb)
        pixels = AGENTS * H * W
        res = {"config": key, "in_channels": cin, "dim": dim, "agents": AGENTS, "map": f"{H}x{W}", "pixels": pixels, "blocks": 3}
        with torch.no_grad():
            fns = {"block_us": lambda: convnext_block(xb, *bargs, out=yb),
                   "torch_block_us": lambda: R.convnext_block(bp, xb),
                   "adapter_us": lambda: mod(x),
                   "torch_us": lambda: R.adapter_forward(cfg, sdd, "adapter", x)}
            w = alternate(fns, a.iters, a.reps, a.warmup)
            for k in fns:
                stats(res, k, w[k])
            res["adapter_launches"], res["torch_launches"] = count_kernels(fns["adapter_us"]), count_kernels(fns["torch_us"])
            res["block_launches"], res["torch_block_launches"] = count_kernels(fns["block_us"]), count_kernels(fns["torch_block_us"])
            with _lib.kernel_log() as kl:
                mod(x)
            res["kernels"] = kl.counts
            flop = pixels * 2 * 2 * dim * 4 * dim
            res["block_linear_flop"], res["block_floor_us"] = flop, round(flop / (a.fp32_matrix_tflops * 1e12) * 1e6, 1)
            res["block_times_floor"] = round(res["block_us"] / res["block_floor_us"], 2)
            res["block_achieved_tflops"] = round(flop / res["block_us"] / 1e6, 1)
            res["hidden_bytes_not_written"] = pixels * 4 * dim * 4
            res["torch_over_fused"] = round(res["torch_us"] / res["adapter_us"], 2)
            res["torch_block_over_fused"] = round(res["torch_block_us"] / res["block_us"], 2)
            res["max_abs_diff"] = float((mod(x) - R.adapter_forward(cfg, sdd, "adapter", x)).abs().max())
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup,
                       "fp32_matrix_tflops": a.fp32_matrix_tflops, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
