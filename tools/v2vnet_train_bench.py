#!/usr/bin/env python3
"""V2VNet fusion TRAINING timing at the four shapes of tools/v2vnet_bench.py (one scene with 2 and with 5 agents; C = 128 at 64 x 128 and
the yaml block's C = 256 at 128 x 128; 2 rounds, `avg`, one [3, 3] GRU layer). Device time, mean over `--iters` calls after warm-up.

Reported per shape:
  step / forward / backward   `V2VNetFusion(args, trainable=True)`: the training forward and the backward, timed with one event pair each
                   inside every step; beside them the inference forward (no_grad) and, for orientation only, torch autograd of the
                   restated reference loop (tests/v2vnet_restatement.py, float32) on the same GPU
  gru_gate_bwd, aggregate_train_fwd (max: the instantiation that writes the winner map), aggregate_bwd, warp_pairs_bwd
                   each new kernel alone at the shapes of a full round (n^2 pairs, n nodes) against its algorithmic bytes -- every
                   distinct input read once, every output written once -- at `--hbm-tbps` (default 6.3): time / floor
  conv share       the convolutions' input- and weight-gradient kernels of one backward, timed alone at their shapes, as a share of it
  warp_pairs_bwd against the old route
                   what the library offered before for the same result: gencomm_warp_affine_bwd over the P maps (zero fill + float
                   atomics) followed by index_add_ over src_row. The two alternate `--repeats` times in this one call; mean and spread
                   (max - min over the repeats) of each
  peak memory      torch.cuda.max_memory_allocated over one training step, and the same step if the P warped maps of every round were
                   kept for the backward (computed: the measured peak plus their bytes, not run)

    python tools/v2vnet_train_bench.py [--iters 20] [--warmup 3] [--out profiles/v2vnet_train_bench.json]
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

from v2vnet_bench import L, SHAPES, block_args, device_us


def step_us(m, x, n, aff, go, iters, warmup):
    """(forward, backward) device microseconds of a training step, each between its own pair of events."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters)]
    for i in range(warmup + iters):
        m.zero_grad(set_to_none=True)
        x.grad = None
        e = ev[i - warmup] if i >= warmup else None
        if e:
            e[0].record()
        out = m(x, [n], aff)
        if e:
            e[1].record()
        out.backward(go)
        if e:
            e[2].record()
    torch.cuda.synchronize()
    return (sum(e[0].elapsed_time(e[1]) for e in ev) * 1e3 / iters, sum(e[1].elapsed_time(e[2]) for e in ev) * 1e3 / iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "v2vnet_train_bench.json"))
    a = ap.parse_args()
    import v2vnet_restatement as R
    import v2vnet_train_restatement as TR
    from gencomm_amd import V2VNetFusion, _lib, synth, train_ops as T
    from gencomm_amd.runtime import ptr, stream_ptr
    from gencomm_amd.v2vnet import pairs_by_source_row
    dev = torch.device("cuda:0")
    l, st = _lib.lib(), stream_ptr(dev)
    results = []
    for C, H, W, n in SHAPES:
        args = block_args(C, H, W)
        m = V2VNetFusion(args, trainable=True).eval()
        synth.fill_params_(m, 9)
        m = m.to(dev)
        x = torch.from_numpy(R.make_x(n, C, H, W, 10 + n)).to(dev).requires_grad_()
        aff = torch.from_numpy(R.make_affine([n], L, H, W, 11)).to(dev)
        go = torch.randn(1, C, H, W, device=dev)
        P, HW = n * n, H * W
        plane = C * HW * 4
        floor = lambda nbytes: nbytes / (a.hbm_tbps * 1e12) * 1e6
        res = {"in_channels": C, "map": f"{H}x{W}", "agents": n, "num_iteration": 2, "agg_operator": "avg", "pairs_full_round": P}
        fwd, bwd = step_us(m, x, n, aff, go, a.iters, a.warmup)
        res.update(train_forward_us=round(fwd, 1), backward_us=round(bwd, 1), step_us=round(fwd + bwd, 1))
        with torch.no_grad():
            res["inference_forward_us"] = round(device_us(lambda: m(x, [n], aff), a.iters, a.warmup), 1)
        # ---- peak memory of one step
        m.zero_grad(set_to_none=True)
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m(x, [n], aff).backward(go)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        kept = (P + n) * plane                                    # the warped maps of the full round and of the ego-only round
        res.update(resident_before_step_mib=round(base / 2 ** 20, 1), peak_step_mib=round(peak / 2 ** 20, 1),
                   peak_step_if_warped_maps_were_kept_mib=round((peak + kept) / 2 ** 20, 1), warped_maps_mib=round(kept / 2 ** 20, 1))
        m.zero_grad(set_to_none=True)
        x.grad = None
        with torch.no_grad():
            # ---- the four kernels at the shapes of a full round
            xd = x.detach()
            theta = aff[0, :n, :n].reshape(P, 2, 3).contiguous()
            srcl = [j for _ in range(n) for j in range(n)]
            src = torch.tensor(srcl, dtype=torch.int32, device=dev)
            rpo, rp = (torch.tensor(v, dtype=torch.int32, device=dev) for v in pairs_by_source_row(srcl, n))
            rows = torch.arange(n, dtype=torch.int32, device=dev)
            poff = torch.arange(0, P + 1, n, dtype=torch.int32, device=dev)
            y, dy, warped = torch.randn(P, C, H, W, device=dev), torch.empty(P, C, H, W, device=dev), torch.randn(P, C, H, W, device=dev)
            e, de, dh = torch.randn(n, C, H, W, device=dev), torch.empty(n, C, H, W, device=dev), torch.randn(n, C, H, W, device=dev)
            cat, g, dg = torch.randn(n, 2 * C, H, W, device=dev), torch.randn(n, 2 * C, H, W, device=dev), torch.empty(n, 2 * C, H, W, device=dev)
            winner = torch.zeros(n, C, H, W, dtype=torch.uint8, device=dev)
            scratch = torch.empty(_lib.check_size(l.gencomm_v2v_warp_pairs_bwd_scratch_floats(P), "scratch"), device=dev)
            gather = lambda: _lib.check(l.gencomm_v2v_warp_pairs_bwd(ptr(warped), ptr(theta), ptr(src), ptr(rpo), ptr(rp), ptr(dh), ptr(scratch), P, n, C, H, W,
                                                                     1, st), "warp_pairs_bwd")
            kernels = {
                "gru_gate_bwd": (lambda: _lib.check(l.gencomm_gru_gate_bwd(ptr(g), ptr(e), ptr(dg), n, C, HW, st), "gru_gate_bwd"), 5 * n * plane),
                "aggregate_train_fwd_max": (lambda: _lib.check(l.gencomm_v2v_aggregate_train_fwd(
                    ptr(y), ptr(e), ptr(xd), ptr(theta), ptr(rows), ptr(poff), ptr(cat), ptr(winner), n, C, H, W, 1, 0, st), "aggregate_train_fwd"),
                    (P + 2 * n + 2 * n) * plane + n * C * HW),
                "aggregate_bwd": (lambda: _lib.check(l.gencomm_v2v_aggregate_bwd(ptr(cat), ptr(theta), ptr(rows), ptr(poff), None, ptr(dy), ptr(de), n, C, H, W,
                                                                               0, 0, st), "aggregate_bwd"), (P + 2 * n) * plane),
                "warp_pairs_bwd": (gather, (P + 2 * n) * plane),
            }
            for name, (fn, nbytes) in kernels.items():
                us = device_us(fn, a.iters, a.warmup)
                res[f"{name}_us"], res[f"{name}_bytes"], res[f"{name}_floor_us"] = round(us, 2), nbytes, round(floor(nbytes), 2)
                res[f"{name}_times_floor"] = round(us / floor(nbytes), 2)
            # ---- warp_pairs_bwd against the old route, alternating
            tmp = torch.empty(P, C, H, W, device=dev)
            src64 = src.long()

            def old_route():
                _lib.check(l.gencomm_warp_affine_bwd(ptr(theta), ptr(warped), ptr(tmp), P, C, H, W, st), "warp_affine_bwd")
                dh.index_add_(0, src64, tmp)

            new_us, old_us = [], []
            for _ in range(a.repeats):
                new_us.append(device_us(gather, a.iters, a.warmup))
                old_us.append(device_us(old_route, a.iters, a.warmup))
            res["warp_bwd_gather_us"] = {"mean": round(sum(new_us) / len(new_us), 2), "spread": round(max(new_us) - min(new_us), 2)}
            res["warp_bwd_atomics_index_add_us"] = {"mean": round(sum(old_us) / len(old_us), 2), "spread": round(max(old_us) - min(old_us), 2)}
            del tmp
            # ---- the convolutions of one backward: a full round (P pairs, n nodes), the ego-only round (n pairs, 1 node), mlp
            wm, wc = m.msg_cnn.weight.detach(), torch.randn(2 * C, 2 * C, 3, 3, device=dev)
            conv = {}
            for tag, pp, nn_ in (("full", P, n), ("last", n, 1)):
                conv[f"msg_src_wgrad_{tag}"] = device_us(lambda: T.conv2d_wgrad_fixed(y[:pp], warped[:pp], 3, False), a.iters, a.warmup)
                conv[f"msg_src_dgrad_{tag}"] = device_us(lambda: T.conv2d_dgrad(y[:pp], wm[:, :C], 1), a.iters, a.warmup)
                conv[f"msg_node_wgrad_{tag}"] = device_us(lambda: T.conv2d_wgrad_fixed(e[:nn_], dh[:nn_], 3, True), a.iters, a.warmup)
                conv[f"msg_node_dgrad_{tag}"] = device_us(lambda: T.conv2d_dgrad(e[:nn_], wm[:, C:], 1), a.iters, a.warmup)
                conv[f"cell_wgrad_{tag}"] = device_us(lambda: T.conv2d_wgrad_fixed(g[:nn_], cat[:nn_], 3, True), a.iters, a.warmup)
                conv[f"cell_dgrad_{tag}"] = device_us(lambda: T.conv2d_dgrad(g[:nn_], wc, 1), a.iters, a.warmup)
            conv["mlp_wgrad"] = device_us(lambda: T.conv2d_wgrad_fixed(go, e[:1], 1, True), a.iters, a.warmup)
            conv["mlp_dgrad"] = device_us(lambda: T.conv2d_dgrad(go, m.mlp.weight.detach()[:, :, None, None], 0), a.iters, a.warmup)
            res["conv_bwd_us"] = {k: round(v, 1) for k, v in conv.items()}
            res["conv_share_of_backward"] = round(sum(conv.values()) / res["backward_us"], 3)
            del y, dy, warped, e, de, dh, cat, g, dg, winner
        # ---- orientation: torch autograd of the reference's loop restated in torch, float32, same GPU
        p = {k: v.detach().clone().requires_grad_() for k, v in m.state_dict().items()}
        live = {k: TR.KeepGraph(v) for k, v in p.items()}

        def torch_step():
            for v in p.values():
                v.grad = None
            x.grad = None
            R.v2vnet_loop_forward(live, args, x, [n], aff).backward(go)

        res["torch_autograd_step_us"] = round(device_us(torch_step, max(a.iters // 5, 2), 1), 1)
        x.grad = None
        print(json.dumps(res), flush=True)
        results.append(res)
        del p, live
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "repeats": a.repeats, "hbm_tbps": a.hbm_tbps,
                       "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
