#!/usr/bin/env python3
"""MPDA aligner timing at the shipped shape: 128 channels, a 64 x 128 map, one scene of 1 ego + 1..4 collaborators, ``resizer`` and
``cdt`` as in GenComm_yamls/baselines/stage2/MPDA/m1m3_att.yaml -- against the plain-torch restatement (tests/mpda_restatement.py) in
float32 on the same GPU, in the same process. Device time between two events on the stream: warm-up of every shape, then ``--reps``
rounds; a round times a window of ``--iters`` calls of each function in turn, so that both see the same clocks and neighbours. The
median window is reported with the fastest and slowest beside it.

Reported per collaborator count:
  align      MPDAAlign.forward (HIP) and the restatement's mpda_align (torch float32), us per call, and torch / HIP
  quad[...]  one launch of gencomm_quad_attn_fwd in the cdt's cross form (16 heads x dim_head 32; queries of the n collaborators, ONE
             ego map of keys / values) and in the resizer's self form (4 heads x dim_head 32; q | k | v blocks of one tensor, with
             the bias table), window and grid mode:
             us, the bytes the launch must move (q, k, v read once, out written once, 4 B each), the bandwidth that gives, and its
             share of the HBM figures of MI355X_MICROARCH.md (6.29 TB/s measured float4 copy; 8.0 TB/s spec). The launches rotate
             over ``--rotate`` buffer sets (each form's tensors together exceed the 256 MB Infinity Cache), so the bytes come from HBM. Beside it the
             restatement's quad_attention on the same tensors in torch float32 (the ego expanded, as the reference repeats it).

    python tools/mpda_bench.py [--iters 20] [--reps 7] [--warmup 3] [--out profiles/mpda_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch

C, H, W, HEADS, DH = 128, 64, 128, 16, 32
SELF_HEADS = C // DH          # the resizer's Attention: dim 128 / dim_head 32
HBM_MEASURED_TBPS, HBM_SPEC_TBPS = 6.29, 8.0


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


def med(w):
    return f"{statistics.median(w):9.1f} us (min {min(w):.1f}, max {max(w):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rotate", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mpda_bench.txt"))
    a = ap.parse_args()
    import mpda_restatement as R
    from gencomm_amd import MPDAAlign, _lib, synth
    from gencomm_amd.mpda import quad_attention
    if not torch.cuda.is_available():
        raise SystemExit("mpda_bench needs a ROCm GPU: a time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; library {_lib.library_src_hash()}; iters {a.iters} reps {a.reps} warmup {a.warmup} rotate {a.rotate}")
    say(f"shape: {C} channels, {H} x {W} map, 1 ego + n collaborators in one scene; cross form {HEADS} heads, self form {SELF_HEADS} heads, dim_head {DH}")
    model = MPDAAlign(R.shipped_args()).eval()
    synth.fill_params_(model, 11)
    synth.fill_bn_stats_(model, 12)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(dev)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    args = R.shipped_args()
    gen = torch.Generator(device="cpu").manual_seed(13)
    torch.manual_seed(14)
    index = R.rel_pos_indices(2).to(dev)
    inner, sinner = HEADS * DH, SELF_HEADS * DH

    for n in (1, 2, 3, 4):
        x = torch.randn(1 + n, C, H, W, generator=gen).to(dev)
        with torch.no_grad():
            got = model(x, [1 + n])[0]
            ref = R.mpda_align(sd, args, x, [1 + n])[0]
            err = float((got - ref).abs().max())
            w = alternate({"hip": lambda: model(x, [1 + n]), "torch": lambda: R.mpda_align(sd, args, x, [1 + n])}, a.iters, a.reps, a.warmup)
        ratio = statistics.median(w["torch"]) / statistics.median(w["hip"])
        say(f"n {n} align       HIP {med(w['hip'])}   torch {med(w['torch'])}   torch / HIP {ratio:.2f}   max |HIP - torch| {err:.2e}")

        # the kernel alone, over rotating buffer sets
        sets = [dict(q=torch.randn(n, inner, H, W, device=dev), k=torch.randn(1, inner, H, W, device=dev),
                     v=torch.randn(1, inner, H, W, device=dev), qkv=torch.randn(n, 3 * sinner, H, W, device=dev))
                for _ in range(a.rotate)]
        table = torch.randn(9, SELF_HEADS, device=dev)
        cross_bytes = (2 * n + 2) * inner * H * W * 4
        self_bytes = 4 * n * sinner * H * W * 4
        for grid in (0, 1):
            turn = {"c": 0, "s": 0, "tc": 0, "ts": 0}

            def nxt(key):
                turn[key] = (turn[key] + 1) % a.rotate
                return sets[turn[key]]

            def hip_cross():
                s = nxt("c")
                return quad_attention(s["q"], s["k"], s["v"], None, HEADS, DH, grid)

            def hip_self():
                s = nxt("s")["qkv"]
                return quad_attention(s, s, s, table, SELF_HEADS, DH, grid, 0, sinner, 2 * sinner)

            def torch_cross():
                s = nxt("tc")
                return R.quad_attention(s["q"], s["k"], s["v"], None, None, HEADS, DH, bool(grid))

            def torch_self():
                q, k, v = nxt("ts")["qkv"].chunk(3, dim=1)
                return R.quad_attention(q, k, v, table, index, SELF_HEADS, DH, bool(grid))

            with torch.no_grad():
                w = alternate({"hip_cross": hip_cross, "torch_cross": torch_cross, "hip_self": hip_self, "torch_self": torch_self},
                              a.iters, a.reps, a.warmup)
            for form, nbytes in (("cross", cross_bytes), ("self", self_bytes)):
                us = statistics.median(w["hip_" + form])
                tbps = nbytes / us / 1e6
                say(f"n {n} quad[{form:5s} {'grid  ' if grid else 'window'}] HIP {med(w['hip_' + form])}   {nbytes / 1e6:6.1f} MB -> {tbps:.2f} TB/s = "
                    f"{100 * tbps / HBM_MEASURED_TBPS:.0f} % of {HBM_MEASURED_TBPS} TB/s (measured copy), {100 * tbps / HBM_SPEC_TBPS:.0f} % of {HBM_SPEC_TBPS} TB/s (spec)"
                    f"   torch {med(w['torch_' + form])}   torch / HIP {statistics.median(w['torch_' + form]) / us:.2f}")
        del sets
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
