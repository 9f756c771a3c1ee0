#!/usr/bin/env python3
"""Training-step timing of the CodeFilling codec: UMGMQuantizer(trainable=True).forward_map plus the straight-through backward
(gencomm_umgm_bwd) on the shipped shape (C = 128, m = 2, k = [16, 16, 16], a 64 x 128 map, 5 agents: n = 40 960 rows) and on C = 256,
Philox noise drawn in the kernel, NCHW entry. Same method as tools/codebook_bench.py: device time between two events on the stream,
warm-up, then `--reps` windows of `--iters` steps enqueued back to back; the median window is reported with the fastest and slowest
beside it. One process.

Reported per shape:
  step_us           forward + backward of sum(restored * G) + code_loss through autograd, every parameter and x wanting a gradient
  backward_us       gencomm_umgm_bwd alone (the ABI entry on the saved tensors), and backward_dx_only_us with its dx-only flag
  launches          kernels per step (torch.profiler) and the library's own kernel log of one backward
  kernel_us         device time per kernel name of one step (torch.profiler), where the time goes
  peak_bytes        torch's peak allocation over one step above the resident parameters and inputs, and the backward's workspace
  floor_us          the fp32-matrix floor of the backward from the shapes: the recomputed forward's Linears, as many input-gradient
                    products and as many weight-gradient products, 2 rows C^2 each, at `--fp32-matrix-tflops` (default 157.3)
  torch_step_us     the same step by torch autograd of tests/codebook_train_restatement.py in float32 on the same GPU, same uniforms
                    supplied (the draws themselves are not timed), its launch count and peak allocation

    python tools/codebook_train_bench.py [--iters 20] [--reps 7] [--warmup 5] [--out profiles/codebook_train_bench.json]

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
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch

from codebook_bench import SHAPES, count_kernels, windows_us


def kernel_times(fn):
    """{kernel name: device microseconds} of one call"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                t = getattr(e, "device_time", None)
                t = getattr(e, "cuda_time", 0.0) if t is None else t
                name = e.name.split("(")[0][:60]
                out[name] = round(out.get(name, 0.0) + float(t), 1)
        return dict(sorted(out.items(), key=lambda kv: -kv[1])[:12])
    except Exception as exc:   # noqa: BLE001 -- a diagnostic figure: report why it is missing instead of failing the timing run
        print(f"kernel times not available: {exc}", file=sys.stderr)
        return None


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fp32-matrix-tflops", type=float, default=157.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "codebook_train_bench.json"))
    a = ap.parse_args()
    import codebook_restatement as R
    import codebook_train_restatement as T
    from gencomm_amd import UMGMQuantizer, _lib
    from gencomm_amd.runtime import ptr, stream_ptr
    if not torch.cuda.is_available():
        raise SystemExit("codebook_train_bench needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    results = []
    for C, m, ks, A, H, W in SHAPES:
        n, L = A * H * W, len(ks)
        sd = R.make_params(C, m, ks, 41, 4.0, 2.0)
        mod = UMGMQuantizer(C, m, list(ks), 0.0, R.components(C), trainable=True)
        mod.load_state_dict(sd, strict=True)
        mod = mod.to(dev).eval()
        x = R.make_x(n, C, 42).view(A, H * W, C).permute(0, 2, 1).reshape(A, C, H, W).contiguous().to(dev).requires_grad_(True)
        G = R.make_x(n, C, 43).view(A, H * W, C).permute(0, 2, 1).reshape(A, C, H, W).contiguous().to(dev)
        res = {"channel": C, "m": m, "k": ks, "agents": A, "map": f"{H}x{W}", "rows": n, "noise": "in-kernel Philox"}

        def step():
            x.grad = None
            for p in mod.parameters():
                p.grad = None
            restored, _, _, loss = mod.forward_map(x, seed=7)
            ((restored * G).sum() + loss).backward()

        w = windows_us(step, a.iters, a.reps, a.warmup)
        res["step_us"], res["step_us_min"], res["step_us_max"] = round(statistics.median(w), 1), round(min(w), 1), round(max(w), 1)
        res["launches_per_step"] = count_kernels(step)
        res["kernel_us"] = kernel_times(step)
        res["peak_bytes_step"] = peak_bytes(step)
        with torch.no_grad():
            fwd = lambda: mod.forward_map(x, seed=7)
            fw = windows_us(fwd, a.iters, a.reps, a.warmup)
            res["forward_us"] = round(statistics.median(fw), 1)
            # ---- the backward alone, on the saved tensors
            l = _lib.lib()
            xr = x.detach().view(A, C, H * W).permute(0, 2, 1).reshape(n, C).contiguous()
            sampled = torch.stack(mod(xr, seed=7, return_sampled=True)[4]).contiguous()
            blob, dx, dblob = mod._params(dev), torch.empty_like(x), torch.empty_like(mod._params(dev))
            need = l.gencomm_umgm_bwd_workspace_bytes(n, C, m, mod._k_arr, L)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            gl = torch.ones((), dtype=torch.float32, device=dev)
            res["backward_workspace_bytes"] = int(need)

            def bwd(dx_only=0):
                _lib.check(l.gencomm_umgm_bwd(ptr(blob), ptr(x), None, None, 7, 2, ptr(sampled), ptr(G), ptr(gl), ptr(dx), ptr(dblob), dx_only, A, H * W,
                                              C, m, mod._k_arr, L, ptr(ws), need, stream_ptr(dev)), "gencomm_umgm_bwd")

            bw = windows_us(bwd, a.iters, a.reps, a.warmup)
            res["backward_us"], res["backward_us_min"], res["backward_us_max"] = round(statistics.median(bw), 1), round(min(bw), 1), round(max(bw), 1)
            res["backward_dx_only_us"] = round(statistics.median(windows_us(lambda: bwd(1), a.iters, a.reps, a.warmup)), 1)
            with _lib.kernel_log() as kl:
                bwd()
            res["backward_kernels"] = kl.counts
            lin = (6 * L - 2) * 2 * n * C * C
            res["backward_flop"] = 3 * lin
            res["backward_floor_us"] = round(3 * lin / (a.fp32_matrix_tflops * 1e12) * 1e6, 1)
            res["backward_times_floor"] = round(res["backward_us"] / res["backward_floor_us"], 2)
            del ws, dblob, dx
        # ---- torch autograd of the float32 restatement, same GPU, uniforms supplied
        u = mod.philox_uniforms(7, n)
        P = {k: v.to(dev) for k, v in sd.items()}
        keys = T.param_keys(sd)
        for k in keys:
            P[k].requires_grad_(True)
        for i in range(L):
            P[f"_encoders.{i}._dequantizer._codebook"] = P[f"_decoders.{i}._dequantizer._codebook"] = P[f"_encoders.{i}._quantizer._codebook"]
        xt, Gr = xr.clone().requires_grad_(True), G.view(A, C, H * W).permute(0, 2, 1).reshape(n, C).contiguous()

        def torch_step():
            out = T.train_forward(P, xt, m, ks, u)
            torch.autograd.grad((out["restored"] * Gr).sum() + out["loss"], [xt] + [P[k] for k in keys])

        tw = windows_us(torch_step, max(a.iters // 4, 3), max(a.reps // 2, 3), 3)
        res["torch_step_us"], res["torch_launches"] = round(statistics.median(tw), 1), count_kernels(torch_step)
        res["peak_bytes_torch_step"] = peak_bytes(torch_step)
        res["torch_over_fused"] = round(res["torch_step_us"] / res["step_us"], 2)
        print(json.dumps(res), flush=True)
        results.append(res)
        del P, u, xt, Gr
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup,
                       "fp32_matrix_tflops": a.fp32_matrix_tflops, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
