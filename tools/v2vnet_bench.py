#!/usr/bin/env python3
"""V2VNet fusion timing, one scene with 2 and with 5 agents: the shipped-map shape (C = 128, 64 x 128) and the yaml block's own shape
(C = 256, 128 x 128), 2 rounds, `avg`, one [3, 3] GRU layer. Device time per call: warm-up, then the mean over `--iters` calls enqueued
back to back between two events on the stream, then a synchronisation. One process.

Reported per shape:
  forward          the whole V2VNetFusion.forward, and the number of kernels it launches (counted with torch.profiler in this process)
  warp_pairs, aggregate, gru_gate
                   each of the three message-passing kernels alone at the shapes of a full round (n^2 pairs, n nodes) against its
                   algorithmic bytes -- every distinct input read once, the output written once -- at `--hbm-tbps` (default 6.3, the
                   achievable HBM rate of the MI355X, not the 8 TB/s of the specification): time / floor
  conv share       the convolutions of one forward (source half and node half of msg_cnn, the GRU cell, mlp; timed alone at their shapes,
                   summed over the rounds) as a share of the forward
  torch loop       for orientation: tests/v2vnet_restatement.py's restatement of the reference's loop (undecomposed, every node in the
                   last round) run with torch on the same GPU in float32

    python tools/v2vnet_bench.py [--iters 20] [--warmup 3] [--out profiles/v2vnet_bench.json]

Prints one JSON line per shape and writes them all to --out.
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

L = 5
SHAPES = [(128, 64, 128, 2), (128, 64, 128, 5), (256, 128, 128, 2), (256, 128, 128, 5)]   # (C, H, W, agents)


def block_args(C, H, W):
    return {"in_channels": C, "num_iteration": 2, "gru_flag": True, "agg_operator": "avg",
            "conv_gru": {"H": H, "W": W, "num_layers": 1, "kernel_size": [[3, 3]]}}


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


def count_kernels(fn):
    """Device kernels of one call, from torch.profiler (None where the profiler is not available)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "v2vnet_bench.json"))
    a = ap.parse_args()
    import v2vnet_restatement as R
    from gencomm_amd import V2VNetFusion, _lib, synth
    from gencomm_amd.runtime import ptr, stream_ptr
    dev = torch.device("cuda:0")
    l, st = _lib.lib(), stream_ptr(dev)
    results = []
    for C, H, W, n in SHAPES:
        args = block_args(C, H, W)
        m = V2VNetFusion(args).eval()
        synth.fill_params_(m, 9)
        m = m.to(dev)
        x = torch.from_numpy(R.make_x(n, C, H, W, 10 + n)).to(dev)
        aff = torch.from_numpy(R.make_affine([n], L, H, W, 11)).to(dev)
        P, HW = n * n, H * W
        plane = C * HW * 4
        floor = lambda nbytes: nbytes / (a.hbm_tbps * 1e12) * 1e6
        res = {"in_channels": C, "map": f"{H}x{W}", "agents": n, "num_iteration": 2, "agg_operator": "avg", "pairs_full_round": P}
        with torch.no_grad():
            res["forward_us"] = round(device_us(lambda: m(x, [n], aff), a.iters, a.warmup), 1)
            res["launches_per_forward"] = count_kernels(lambda: m(x, [n], aff))
            # ---- the three kernels at the shapes of a full round
            theta = aff[0, :n, :n].reshape(P, 2, 3).contiguous()
            src = torch.tensor([j for _ in range(n) for j in range(n)], dtype=torch.int32, device=dev)
            rows = torch.arange(n, dtype=torch.int32, device=dev)
            poff = torch.arange(0, P + 1, n, dtype=torch.int32, device=dev)
            warped, y = torch.empty(P, C, H, W, device=dev), torch.randn(P, C, H, W, device=dev)
            e, cat, g, hn = torch.randn(n, C, H, W, device=dev), torch.empty(n, 2 * C, H, W, device=dev), torch.randn(n, 2 * C, H, W, device=dev), torch.empty(n, C, H, W, device=dev)
            kernels = {
                "warp_pairs": (lambda: _lib.check(l.gencomm_v2v_warp_pairs_fwd(ptr(x), ptr(theta), ptr(src), ptr(warped), P, C, H, W, st), "warp_pairs"),
                               (n + P) * plane),
                "aggregate": (lambda: _lib.check(l.gencomm_v2v_aggregate_fwd(ptr(y), ptr(e), ptr(x), ptr(theta), ptr(rows), ptr(poff), ptr(cat), n, C, H, W,
                                                                           0, 0, st), "aggregate"), (P + 2 * n + 2 * n) * plane),
                "gru_gate": (lambda: _lib.check(l.gencomm_gru_gate_fwd(ptr(g), ptr(hn), n, C, HW, st), "gru_gate"), 3 * n * plane),
            }
            for name, (fn, nbytes) in kernels.items():
                us = device_us(fn, a.iters, a.warmup)
                res[f"{name}_us"], res[f"{name}_bytes"], res[f"{name}_floor_us"] = round(us, 2), nbytes, round(floor(nbytes), 2)
                res[f"{name}_times_floor"] = round(us / floor(nbytes), 2)
            # ---- the convolutions of one forward: a full round (P pairs, n nodes) and the last round (n pairs, 1 node), then mlp
            src_w = m._weights("msg_src", [m.msg_cnn.weight], lambda: (m.msg_cnn.weight[:, :C], None), 3, dev)
            node_w = m._weights("msg_node", [m.msg_cnn.weight, m.msg_cnn.bias], lambda: (m.msg_cnn.weight[:, C:], m.msg_cnn.bias), 3, dev)
            cell_w = m._cell_weights(0, dev)
            conv = {}
            conv["msg_src_full"] = device_us(lambda: m._conv(warped, src_w), a.iters, a.warmup)
            conv["msg_node_full"] = device_us(lambda: m._conv(x, node_w), a.iters, a.warmup)
            conv["cell_full"] = device_us(lambda: m._conv(cat, cell_w), a.iters, a.warmup)
            conv["msg_src_last"] = device_us(lambda: m._conv(warped[:n], src_w), a.iters, a.warmup)
            conv["msg_node_last"] = device_us(lambda: m._conv(x[:1], node_w), a.iters, a.warmup)
            conv["cell_last"] = device_us(lambda: m._conv(cat[:1], cell_w), a.iters, a.warmup)
            from gencomm_amd.v2xvit import _linear
            mlp_w = m._weights("mlp", [m.mlp.weight, m.mlp.bias], lambda: (m.mlp.weight[:, :, None, None], m.mlp.bias), 1, dev)
            conv["mlp"] = device_us(lambda: _linear(hn[:1], mlp_w[:4]), a.iters, a.warmup)
            res["conv_us"] = {k: round(v, 1) for k, v in conv.items()}
            res["conv_share_of_forward"] = round(sum(conv.values()) / res["forward_us"], 3)
            # ---- orientation: the reference's loop restated in torch, float32, same GPU
            sd = {k: v.detach() for k, v in m.state_dict().items()}
            res["torch_loop_us"] = round(device_us(lambda: R.v2vnet_loop_forward(sd, args, x, [n], aff), max(a.iters // 5, 2), 1), 1)
        print(json.dumps(res), flush=True)
        results.append(res)
        del warped, y, e, cat, g, hn
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "hbm_tbps": a.hbm_tbps, "results": results},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
