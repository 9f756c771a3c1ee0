#!/usr/bin/env python3
"""CodeFilling codebook codec timing: UMGMQuantizer.forward_map on the shipped shape (C = 128, m = 2, k = [16, 16, 16], a 64 x 128 map,
5 agents: n = 40 960 rows) and on C = 256, Philox noise drawn in the kernel. Device time per forward between two events on the stream:
warm-up, then `--reps` windows of `--iters` forwards enqueued back to back; the median window is reported with the fastest and slowest
beside it. One process.

Reported per shape:
  forward_us        the fused codec (one launch of the codec kernel plus the one-workgroup loss sum) and its launch count (torch.profiler)
  flop, floor_us    the matrix arithmetic of the algorithm from the shapes -- per row 2 C^2 per Linear, 6 per level and 4 on the last (21.5
                    GFLOP at the shipped shape) -- at `--fp32-matrix-tflops` (default 157.3, the fp32 matrix rate of the MI355X): time /
                    floor; distance_flop (2 k C per row and level, on the VALU) is listed beside it
  bytes, hbm_floor_us  x read once, restored and the codes written once, the parameters read once, at `--hbm-tbps` (default 6.3)
  l2_weight_bytes   what the kernel re-reads from L2: the parameters once per 64-row tile
  bound             which pipe bounds the kernel, from the kernel's own arithmetic (csrc/codebook_kernels.h): the matrix pipe issues one
                    16x16x4 fp32 MFMA per 2 048 FLOP; everything else (LDS reads, L2 weight reads, the VALU distances) fits under it
  torch_us          tests/codebook_restatement.py's forward run with torch on the same GPU in float32, same uniforms supplied (the draws
                    themselves are not timed), and the number of kernels it launches

    python tools/codebook_bench.py [--iters 50] [--reps 7] [--warmup 10] [--out profiles/codebook_bench.json]

Prints one JSON line per shape and writes them all to --out.
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

SHAPES = [(128, 2, [16, 16, 16], 5, 64, 128), (256, 2, [16, 16, 16], 5, 64, 128)]   # (C, m, k, agents, H, W)
TILE_ROWS = 64


def windows_us(fn, iters, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
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


def algorithm_flop(n, C, ks):
    """(the Linear layers, the distances)"""
    return n * (6 * len(ks) - 2) * 2 * C * C, n * sum(2 * k * C for k in ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fp32-matrix-tflops", type=float, default=157.3)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "codebook_bench.json"))
    a = ap.parse_args()
    import codebook_restatement as R
    from gencomm_amd import UMGMQuantizer, _lib
    if not torch.cuda.is_available():
        raise SystemExit("codebook_bench needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    results = []
    for C, m, ks, A, H, W in SHAPES:
        n = A * H * W
        sd = R.make_params(C, m, ks, 41, 4.0, 2.0)
        mod = UMGMQuantizer(C, m, list(ks), 0.0, R.components(C))
        mod.load_state_dict(sd, strict=True)
        mod = mod.to(dev).eval()
        x = R.make_x(n, C, 42).view(A, H * W, C).permute(0, 2, 1).reshape(A, C, H, W).contiguous().to(dev)
        param_floats = sum(v.numel() for k, v in sd.items() if "_dequantizer" not in k)
        res = {"channel": C, "m": m, "k": ks, "agents": A, "map": f"{H}x{W}", "rows": n, "noise": "in-kernel Philox",
               "payload_bits_per_row": mod.payload_bits_per_row}
        with torch.no_grad():
            fn = lambda: mod.forward_map(x, seed=7)
            w = windows_us(fn, a.iters, a.reps, a.warmup)
            res["forward_us"], res["forward_us_min"], res["forward_us_max"] = round(statistics.median(w), 1), round(min(w), 1), round(max(w), 1)
            res["launches_per_forward"] = count_kernels(fn)
            with _lib.kernel_log() as kl:
                fn()
            res["kernels"] = kl.counts
            flop, dist_flop = algorithm_flop(n, C, ks)
            res["distance_flop"] = dist_flop
            nbytes = 2 * n * C * 4 + len(ks) * n * m * 8 + param_floats * 4
            res["flop"], res["floor_us"] = flop, round(flop / (a.fp32_matrix_tflops * 1e12) * 1e6, 1)
            res["times_floor"] = round(res["forward_us"] / res["floor_us"], 2)
            res["achieved_tflops"] = round(flop / res["forward_us"] / 1e6, 1)
            res["bytes"], res["hbm_floor_us"] = nbytes, round(nbytes / (a.hbm_tbps * 1e12) * 1e6, 1)
            tiles = (n + TILE_ROWS - 1) // TILE_ROWS
            res["l2_weight_bytes"] = tiles * param_floats * 4
            res["l2_weight_tbps_at_measured_time"] = round(res["l2_weight_bytes"] / res["forward_us"] / 1e6, 2)
            res["bound"] = "fp32 matrix pipe (compute-bound: the arithmetic floor is %.0f x the HBM floor)" % (res["floor_us"] / res["hbm_floor_us"])
            # ---- the torch restatement, float32, same GPU, uniforms supplied
            sdd = {k: v.to(dev) for k, v in sd.items()}
            xr = x.view(A, C, H * W).permute(0, 2, 1).reshape(n, C).contiguous()
            u = mod.philox_uniforms(7, n)
            tfn = lambda: R.umgm_forward(sdd, xr, m, ks, u, torch.float32)
            tw = windows_us(tfn, max(a.iters // 5, 3), max(a.reps // 2, 3), 3)
            res["torch_us"], res["torch_launches"] = round(statistics.median(tw), 1), count_kernels(tfn)
            res["torch_over_fused"] = round(res["torch_us"] / res["forward_us"], 2)
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup,
                       "fp32_matrix_tflops": a.fp32_matrix_tflops, "hbm_tbps": a.hbm_tbps, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
