#!/usr/bin/env python3
"""MPDA aligner TRAINING step timing at the shipped shape (128 channels, a 64 x 128 map, one scene of 1 ego + 1..4 collaborators,
``resizer`` and ``cdt`` as in GenComm_yamls/baselines/stage2/MPDA/m1m3_att.yaml), with the method of tools/mpda_bench.py: device time
between two events on the stream, warm-up of every function, then ``--reps`` rounds; a round times a window of ``--iters`` calls of
each function in turn, so that all see the same clocks and neighbours; the median window is reported with the fastest and slowest.

Reported per collaborator count:
  step       forward + backward of MPDAAlign(trainable=True) in eval() (dropout off, BatchNorm folded: what the float32 restatement
             computes without being handed masks) against torch autograd of tests/mpda_train_restatement.py's mpda_align in float32,
             on the same card in the same process; loss = the linear functional + BCE-with-logits of the golden cases. Beside it the HIP
             step in train() (dropout 0.1 drawn on the device, BatchNorm batch statistics) -- HIP only, no torch counterpart is timed.
  peak       peak allocated device memory of one step of each, above what is allocated before the step.
  quad_bwd   one call of gencomm_quad_attn_bwd in the cdt's cross form (16 heads x 32, ONE ego map: the per-map dk / dv slabs and their
             fixed-order sum are part of the call) and in the resizer's self form (4 heads x 32, with the bias table: the dbias
             partials and their sum are part of the call), window and grid. Bytes: the floor (q, k, v, dout read once; dq, dk, dv
             written once) and what the call really requests (q, k and dout are read TWICE -- pass 1 and pass 2 --; the cross form
             also writes and re-reads 2 n slabs). The bandwidth is the FLOOR's bytes over the time, as a fraction of the copy
             bandwidth measured in this process (a float32 tensor copy over the same rotation of buffers).
  resize_bwd one call of gencomm_resize_bilinear_bwd: the shipped same-size case (64 x 128 -> 64 x 128: dy is copied) and a real resize
             (the adjoint of 96 x 192 -> 64 x 128). Bytes: dy read once, dx written once.
The launches rotate over ``--rotate`` buffer sets so the bytes come from HBM, not the Infinity Cache.

    python tools/mpda_train_bench.py [--iters 10] [--reps 5] [--warmup 2] [--out profiles/mpda_train_bench.txt]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch

from mpda_bench import C, DH, H, HEADS, SELF_HEADS, W, alternate, med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rotate", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mpda_train_bench.txt"))
    a = ap.parse_args()
    import mpda_restatement as R
    import mpda_train_restatement as TR
    from gencomm_amd import MPDAAlign, _lib, synth
    from gencomm_amd.mpda import quad_attention_bwd, resize_bilinear_bwd
    if not torch.cuda.is_available():
        raise SystemExit("mpda_train_bench needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; library {_lib.library_src_hash()}; iters {a.iters} reps {a.reps} warmup {a.warmup} rotate {a.rotate}")
    say(f"shape: {C} channels, {H} x {W} map, 1 ego + n collaborators in one scene; cross form {HEADS} heads, self form {SELF_HEADS} heads, dim_head {DH}")
    args = R.shipped_args()
    model = MPDAAlign(args, trainable=True).eval()
    synth.fill_params_(model, 11)
    synth.fill_bn_stats_(model, 12)
    model = model.to(dev)
    train_model = copy.deepcopy(model).train()   # its BatchNorm running statistics move with every step: a copy, so `model` keeps the restatement's
    sd = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and k in dict(model.named_parameters()) else v.detach().clone())
          for k, v in model.state_dict().items()}
    leaves = [v for v in sd.values() if v.requires_grad]
    gen = torch.Generator(device="cpu").manual_seed(13)
    torch.manual_seed(14)
    inner, sinner = HEADS * DH, SELF_HEADS * DH

    def peak_mb(fn):
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e6

    # the copy bandwidth of this process: 64 MB float32 tensors, rotated
    src = [torch.randn(16 << 20, device=dev) for _ in range(a.rotate)]
    dst = [torch.empty(16 << 20, device=dev) for _ in range(a.rotate)]
    turn = {"i": 0}

    def copy_once():
        turn["i"] = (turn["i"] + 1) % a.rotate
        dst[turn["i"]].copy_(src[turn["i"]])

    w = alternate({"copy": copy_once}, a.iters, a.reps, a.warmup)
    copy_tbps = 2 * (16 << 20) * 4 / statistics.median(w["copy"]) / 1e6
    say(f"copy bandwidth in this process (64 MB float32 tensor copy, read + write): {med(w['copy'])} -> {copy_tbps:.2f} TB/s")
    del src, dst
    torch.cuda.empty_cache()

    for n in (1, 2, 3, 4):
        x = torch.randn(1 + n, C, H, W, generator=gen).to(dev)
        g = torch.randn(1 + n, C, H, W, generator=gen).to(dev)
        rl = [1 + n]

        def hip_step(m=model):
            xd = x.detach().requires_grad_(True)
            aligned, logits = m(xd, rl)
            TR.align_loss(aligned, logits, g, rl).backward()
            return xd.grad

        def hip_train_step():
            return hip_step(train_model)

        def torch_step():
            xd = x.detach().requires_grad_(True)
            aligned, logits = TR.mpda_align(sd, args, xd, rl)
            return torch.autograd.grad(TR.align_loss(aligned, logits, g, rl), [xd] + leaves, allow_unused=True)[0]

        err = float((hip_step() - torch_step()).abs().max() / torch_step().abs().max())
        w = alternate({"hip": hip_step, "torch": torch_step}, a.iters, a.reps, a.warmup)
        ratio = statistics.median(w["torch"]) / statistics.median(w["hip"])
        say(f"n {n} step eval()  HIP {med(w['hip'])}   torch {med(w['torch'])}   torch / HIP {ratio:.2f}   max |d x HIP - torch| / max {err:.2e}")
        say(f"n {n} peak eval()  HIP {peak_mb(hip_step):8.1f} MB   torch {peak_mb(torch_step):8.1f} MB")
        w = alternate({"hip": hip_train_step}, a.iters, a.reps, a.warmup)
        say(f"n {n} step train() HIP {med(w['hip'])}   (dropout 0.1, BatchNorm batch statistics; HIP only)   peak {peak_mb(hip_train_step):8.1f} MB")
        for p in [*model.parameters(), *train_model.parameters()]:
            p.grad = None

        # the kernels alone, over rotating buffer sets
        sets = [dict(q=torch.randn(n, inner, H, W, device=dev), k=torch.randn(1, inner, H, W, device=dev), v=torch.randn(1, inner, H, W, device=dev),
                     do=torch.randn(n, inner, H, W, device=dev), qkv=torch.randn(n, 3 * sinner, H, W, device=dev),
                     sdo=torch.randn(n, sinner, H, W, device=dev)) for _ in range(a.rotate)]
        table = torch.randn(9, SELF_HEADS, device=dev)
        unit = H * W * 4
        cross_floor, cross_real = (3 * n + 4) * inner * unit, (3 * n + 4 + 2 * n + 1 + (4 * n if n > 1 else 0)) * inner * unit   # + second reads + slabs
        self_floor, self_real = 7 * n * sinner * unit, 10 * n * sinner * unit
        for grid in (0, 1):
            t = {"c": 0, "s": 0}

            def nxt(key):
                t[key] = (t[key] + 1) % a.rotate
                return sets[t[key]]

            def hip_cross():
                s = nxt("c")
                return quad_attention_bwd(s["q"], s["k"], s["v"], None, s["do"], HEADS, DH, grid)

            def hip_self():
                s = nxt("s")
                return quad_attention_bwd(s["qkv"], s["qkv"], s["qkv"], table, s["sdo"], SELF_HEADS, DH, grid, 0, sinner, 2 * sinner, self_form=True)

            with torch.no_grad():
                w = alternate({"cross": hip_cross, "self": hip_self}, a.iters, a.reps, a.warmup)
            for form, floor, real in (("cross", cross_floor, cross_real), ("self", self_floor, self_real)):
                us = statistics.median(w[form])
                tbps = floor / us / 1e6
                say(f"n {n} quad_bwd[{form:5s} {'grid  ' if grid else 'window'}] {med(w[form])}   floor {floor / 1e6:6.1f} MB (requested {real / 1e6:6.1f} MB) -> "
                    f"{tbps:.2f} TB/s of the floor = {100 * tbps / copy_tbps:.0f} % of the copy bandwidth")
        del sets
        torch.cuda.empty_cache()
        for (hi, wi), label in (((H, W), "same size"), ((96, 192), "96 x 192 source")):
            dys = [torch.randn(n, C, H, W, device=dev) for _ in range(a.rotate)]
            t = {"i": 0}

            def rz():
                t["i"] = (t["i"] + 1) % a.rotate
                return resize_bilinear_bwd(dys[t["i"]], (hi, wi))

            w = alternate({"rz": rz}, a.iters, a.reps, a.warmup)
            nbytes = n * C * (H * W + hi * wi) * 4
            tbps = nbytes / statistics.median(w["rz"]) / 1e6
            say(f"n {n} resize_bwd[{label:15s}] {med(w['rz'])}   {nbytes / 1e6:6.1f} MB -> {tbps:.2f} TB/s = {100 * tbps / copy_tbps:.0f} % of the copy bandwidth")
            del dys
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
