#!/usr/bin/env python3
"""STAMP adapter TRAINING timing: the fused ConvNeXt-block backward and one whole adapter-training step (adapter + reverter under
adapter_loss, the reverter called twice) at the two shipped configurations -- in 128 / dim 64 and in 256 / dim 128 -- on
5 agents x 128 x 256, against torch autograd of the float32 restatement (tests/stamp_adapter_train_restatement.py) on the same GPU in
the same call. The protocol of tools/stamp_adapter_bench.py: device time between two stream events, warm-up of every shape, then
`--reps` rounds of alternating windows of `--iters` calls; the median window with the fastest and slowest beside it. One process.

Reported per configuration:
  block_fwd_bwd_us / torch_block_fwd_bwd_us   one block forward + backward (all ten gradients), fused and torch autograd
  block_bwd_us                                gencomm_convnext_block_bwd alone (6 launches); block_dx_only_us with dx_only (3 launches)
  step_us / torch_step_us                     forward + backward of 9 mse(FM, R(FP)) + 1 mse(FM, R(A(FM))) + 10 mse(FP, A(FM)), no optimizer
  *_launches                                  device kernels of one call (torch.profiler)
  *_peak_bytes                                torch.cuda.max_memory_allocated over one call, above what was allocated before it
  workspace_bytes                             gencomm_convnext_block_bwd_workspace_bytes (inside the fused peak)
  block_bwd_floor_us                          DERIVED, not measured: the FLOP of the SEVEN pixels x dim x 4 dim products the chosen
                                              decomposition executes in a backward (pixel pass: u, dh, dln; weight pass: u, dh, S, dW1) at
                                              `--fp32-matrix-tflops` (default 155, the exact-fp32 MFMA rate); recompute_share = 3 / 7 of it
                                              is recomputation (u twice, dh once) that a tape of the hidden tensor would not need

    python tools/stamp_adapter_train_bench.py [--iters 5] [--reps 5] [--warmup 2] [--out profiles/stamp_adapter_train_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch

from stamp_adapter_bench import AGENTS, CONFIGS, H, W, alternate, count_kernels, stats


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fp32-matrix-tflops", type=float, default=155.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stamp_adapter_train_bench.json"))
    a = ap.parse_args()
    import stamp_adapter_restatement as R
    import stamp_adapter_train_restatement as T
    from gencomm_amd import Adapter, Reverter, _lib
    from gencomm_amd import convnext_bwd as B
    from gencomm_amd.stamp_adapter import convnext_block
    if not torch.cuda.is_available():
        raise SystemExit("stamp_adapter_train_bench needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    mse = torch.nn.functional.mse_loss
    results = []
    for key, cin, dim in CONFIGS:
        cfg = R.SHIPPED[key]
        std = R.STD if dim == 64 else R.STD_WIDE
        sd_a, sd_r = R.make_params(cfg, "adapter", 51, std), R.make_params(cfg, "reverter", 58, R.STD_CHAIN)
        adapter, reverter = Adapter(cfg, trainable=True), Reverter(cfg, trainable=True)
        adapter.load_state_dict(sd_a, strict=True)
        reverter.load_state_dict(sd_r, strict=True)
        adapter, reverter = adapter.to(dev), reverter.to(dev)
        FM, FP = R.make_x((AGENTS, cin, H, W), 52).to(dev), R.make_x((AGENTS, cin, H, W), 54).to(dev)
        xb, dyb = 2.0 * R.make_x((AGENTS, dim, H, W), 53).to(dev), R.make_x((AGENTS, dim, H, W), 55).to(dev)
        bp = {k: v.to(dev) for k, v in R.block_params(sd_a, "adapter", 0).items()}
        bargs = [bp[k] for k in T.ORDER]
        yb, dxb = torch.empty_like(xb), torch.empty_like(xb)
        # torch side: leaves that require a gradient
        tq = {k: v.clone().requires_grad_(True) for k, v in bp.items()}
        txb = xb.clone().requires_grad_(True)
        ta = {k: v.to(dev).requires_grad_(".smoothing." not in k) for k, v in sd_a.items()}
        tr = {k: v.to(dev).requires_grad_(".smoothing." not in k) for k, v in sd_r.items()}
        params = [p for m in (adapter, reverter) for p in m.parameters()]

        def fused_block():
            with torch.no_grad():
                convnext_block(xb, *bargs, out=yb)
                B.convnext_block_bwd(xb, dyb, bargs, out=dxb)

        def fused_bwd():
            B.convnext_block_bwd(xb, dyb, bargs, out=dxb)

        def fused_dx_only():
            B.convnext_block_bwd(xb, dyb, bargs, dx_only=True, out=dxb)

        def torch_block():
            for t in list(tq.values()) + [txb]:
                t.grad = None
            R.convnext_block(tq, txb).backward(dyb)

        def fused_step():
            for p in params:
                p.grad = None
            FM2P = adapter(FM)
            loss = T.ALPHA["alpha_P2M"] * mse(reverter(FP), FM) + T.ALPHA["alpha_M2P2M"] * mse(reverter(FM2P), FM) + T.ALPHA["alpha_M2P"] * mse(FM2P, FP)
            loss.backward()
            return loss

        def torch_step():
            for t in list(ta.values()) + list(tr.values()):
                t.grad = None
            loss = T.step_loss(cfg, ta, cfg, tr, FM, FP, torch.float32)
            loss.backward()
            return loss

        pixels = AGENTS * H * W
        res = {"config": key, "in_channels": cin, "dim": dim, "agents": AGENTS, "map": f"{H}x{W}", "pixels": pixels, "blocks": 3}
        fns = {"block_fwd_bwd_us": fused_block, "torch_block_fwd_bwd_us": torch_block, "block_bwd_us": fused_bwd, "block_dx_only_us": fused_dx_only,
               "step_us": fused_step, "torch_step_us": torch_step}
        w = alternate(fns, a.iters, a.reps, a.warmup)
        for k in fns:
            stats(res, k, w[k])
        for k, fn in (("block_bwd", fused_bwd), ("block_fwd_bwd", fused_block), ("torch_block_fwd_bwd", torch_block), ("step", fused_step),
                      ("torch_step", torch_step)):
            res[k + "_launches"] = count_kernels(fn)
            res[k + "_peak_bytes"] = peak_bytes(fn)
        with _lib.kernel_log() as kl:
            fused_bwd()
        res["block_bwd_kernels"] = kl.counts
        res["workspace_bytes"] = B.workspace_bytes(AGENTS, dim, H, W)
        product = pixels * 2 * dim * 4 * dim
        res["block_bwd_product_flop"], res["recompute_share"] = 7 * product, round(3 / 7, 3)
        res["block_bwd_floor_us"] = round(7 * product / (a.fp32_matrix_tflops * 1e12) * 1e6, 1)
        res["block_bwd_times_floor"] = round(res["block_bwd_us"] / res["block_bwd_floor_us"], 2)
        res["hidden_bytes_not_kept_per_block"] = 2 * pixels * 4 * dim * 4
        res["torch_block_over_fused"] = round(res["torch_block_fwd_bwd_us"] / res["block_fwd_bwd_us"], 2)
        res["torch_step_over_fused"] = round(res["torch_step_us"] / res["step_us"], 2)
        res["step_loss"], res["torch_step_loss"] = float(fused_step().detach()), float(torch_step().detach())
        print(json.dumps(res), flush=True)
        results.append(res)
        del tq, ta, tr, txb
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "library": _lib.library_src_hash(), "iters": a.iters, "reps": a.reps, "warmup": a.warmup,
                       "fp32_matrix_tflops": a.fp32_matrix_tflops, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
