#!/usr/bin/env python3
"""CoBEVT training step timing: the shipped `cobevt:` block (input_dim 256, mlp_dim 256, window_size 4, dim_head 32, depth 3) on a
64 x 128 map, one scene of agent_size 5 with 5 and with 2 agents present, ``CoBEVT(args, trainable=True)`` with every parameter and the
input requiring grad, loss ``(y * g).sum()``. Device time per call: warm-up, then the mean over `--iters` calls enqueued back to back
between two events on the stream, then a synchronisation.

Reported per shape:
  forward_us / train_forward_us   the no_grad forward and the grad-enabled forward (the train entry of the attention + the tape)
  step_us / step_dropout_us       forward + backward in eval() and in train() mode (drop_out 0.1: masks drawn, residuals unfused)
  attn_bwd_{window,grid}_us       gencomm_swap_attn_bwd alone (both launches)
  half_block_wgrad_us / half_block_wgrad_fixed_order_us   the four Linear weight gradients of one half block on gencomm_conv2d_wgrad (what
                                  the backward calls) and on gencomm_conv2d_wgrad_fixed (what bit-identical weight gradients would cost)
  peak_step_bytes / tape_bytes    torch's peak allocation during one step, and that peak minus what is allocated before the step
                                  (parameters, prepared weights, input): the tape and the backward's temporaries
  backward_by_family_us           with --profile: device time per kernel family of the backward, from the kernel traces of two
                                  `rocprofv3 --kernel-trace --stats` runs of this script's `--child` mode (fresh child processes): a full
                                  step minus a grad-enabled forward, per family, per iteration
  torch_step_us / torch_peak_step_bytes   the same step under torch autograd of tests/cobevt_train_restatement.py (float32) on the device

    python tools/cobevt_train_bench.py [--iters 20] [--warmup 3] [--profile] [--out profiles/cobevt_train_bench.json]

Prints one JSON line per shape and writes them all to --out.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np
import torch

from cobevt_bench import H, L, W, block_args, device_us

C = 256
PRESENT = (5, 2)
# kernel name fragment -> family, first match wins
FAMILIES = (("swap_attn_bwd_q", "swap attention backward: query pass (dq, dtable)"), ("swap_attn_bwd_k", "swap attention backward: key pass (dk, dv)"),
            ("swap_attn_kernel", "swap attention forward"), ("wgrad", "weight gradients"),
            ("conv_prep_w", "weight layout for the transposed 1x1 convolutions"), ("conv_fold", "weight layout for the transposed 1x1 convolutions"),
            ("conv", "1x1 convolutions (input gradients, recomputed pre-activation)"), ("ln_nchw_fwd", "LayerNorm forward (recomputed)"),
            ("ln_nchw", "LayerNorm backward"), ("gelu_bwd", "GELU backward"), ("warp_affine_bwd", "warp backward"), ("warp_affine", "warp forward"),
            ("agent_mean", "agent mean"))
OTHER = "torch elementwise (residual sums, mean adjoint, fills)"


def setup(n, dev, train=False):
    import cobevt_restatement as R
    from gencomm_amd import CoBEVT, synth
    m = CoBEVT(block_args(C), trainable=True)
    synth.fill_params_(m, 9)
    m = m.to(dev).train(train)
    rng = np.random.RandomState(10 + n)
    x = torch.from_numpy(np.maximum(rng.standard_normal((n, C, H, W)), 0.0).astype(np.float32)).to(dev).requires_grad_(True)
    aff = torch.from_numpy(R.make_affine([n], L, H, W, 11)).to(dev)
    g = torch.from_numpy(rng.standard_normal((1, C, H, W)).astype(np.float32)).to(dev)
    return m, x, aff, g


def make_step(m, x, aff, g, n):
    params = list(m.parameters())

    def step():
        for p in params:
            p.grad = None
        x.grad = None
        (m(x, [n], aff) * g).sum().backward()
    return step


def family_us(mode, n, iters):
    """Device microseconds per iteration and family of a traced `--child mode,n` run."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="cobevt_train_prof_")
    cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "cobevt_train", "--output-format", "csv", "--", sys.executable,
           os.path.abspath(__file__), "--child", f"{mode},{n}", "--iters", str(iters), "--warmup", "0"]
    subprocess.run(cmd, check=True, timeout=600)
    found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if not found:
        raise RuntimeError(f"rocprofv3 wrote no kernel_trace.csv under {tmp}")
    out = {}
    for r in csv.DictReader(open(found[0])):
        fam = next((f for frag, f in FAMILIES if frag in r["Kernel_Name"]), OTHER)
        out[fam] = out.get(fam, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 / iters
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="split the backward by kernel family from rocprofv3 kernel traces (fresh child processes)")
    ap.add_argument("--child", default="", metavar="MODE,N", help="run only `fwd` (grad-enabled forward) or `step` of one shape (the child of --profile)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cobevt_train_bench.json"))
    a = ap.parse_args()
    split = {}
    if a.profile:   # before this process opens the GPU
        for n in PRESENT[:1]:
            fwd, step = family_us("fwd", n, 4), family_us("step", n, 4)
            split[n] = {k: round(step[k] - fwd.get(k, 0.0), 1) for k in sorted(step, key=lambda k: fwd.get(k, 0.0) - step[k])}
    dev = torch.device("cuda:0")
    if a.child:
        mode, n = a.child.split(",")
        m, x, aff, g = setup(int(n), dev)
        device_us(make_step(m, x, aff, g, int(n)) if mode == "step" else (lambda: m(x, [int(n)], aff)), a.iters, a.warmup)
        return
    import cobevt_train_restatement as TR
    from gencomm_amd import _lib
    from gencomm_amd.runtime import ptr, stream_ptr
    l = _lib.lib()
    results = []
    for n in PRESENT:
        m, x, aff, g = setup(n, dev)
        step = make_step(m, x, aff, g, n)
        res = {"input_dim": C, "map": f"{H}x{W}", "agent_size": L, "agents_present": n, "window_size": 4, "dim_head": 32, "depth": 3}
        with torch.no_grad():
            res["forward_us"] = round(device_us(lambda: m(x, [n], aff), a.iters, a.warmup), 1)
        res["train_forward_us"] = round(device_us(lambda: m(x, [n], aff), a.iters, a.warmup), 1)
        res["step_us"] = round(device_us(step, a.iters, a.warmup), 1)
        x.grad = None
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        res["peak_step_bytes"] = int(torch.cuda.max_memory_allocated())
        res["tape_bytes"] = int(torch.cuda.max_memory_allocated() - before)
        m.train()
        res["step_dropout_us"] = round(device_us(step, a.iters, a.warmup), 1)
        m.eval()
        heads, dh, ws = C // 32, 32, 4
        qkv = torch.randn(L, 3 * C, H, W, device=dev)
        table = torch.rand((2 * L - 1) * (2 * ws - 1) ** 2, heads, device=dev)
        nv = torch.tensor([n], dtype=torch.int32, device=dev)
        out, lse, dout = torch.empty(L, C, H, W, device=dev), torch.empty(L, heads, H, W, device=dev), torch.randn(L, C, H, W, device=dev)
        dqkv, dtable = torch.empty_like(qkv), torch.zeros_like(table)
        st = stream_ptr(dev)
        for name, grid in (("window", 0), ("grid", 1)):
            dims = (1, L, heads, dh, ws, H, W, grid, st)
            _lib.check(l.gencomm_swap_attn_train_fwd(ptr(qkv), ptr(table), ptr(nv), ptr(out), ptr(lse), *dims), "gencomm_swap_attn_train_fwd")
            res[f"attn_bwd_{name}_us"] = round(device_us(lambda: _lib.check(l.gencomm_swap_attn_bwd(
                ptr(qkv), ptr(table), ptr(nv), ptr(out), ptr(lse), ptr(dout), ptr(dqkv), ptr(dtable), *dims), "gencomm_swap_attn_bwd"), a.iters, a.warmup), 2)
        # the weight gradients of one half block's four Linears (to_qkv, to_out, and the FeedForward's two), on the kernel the backward
        # uses (gencomm_conv2d_wgrad: split-K on the matrix cores, meeting in float atomics) and on the fixed-order one
        from gencomm_amd import train_ops as T
        lin = [(qkv, out, False), (out, dout, False), (out, dout, True), (dout, out, True)]       # (dy, x, bias): the shapes are what counts
        res["half_block_wgrad_us"] = round(device_us(lambda: [T.conv2d_wgrad(dy, xx, 1, 0, b) for dy, xx, b in lin], a.iters, a.warmup), 1)
        res["half_block_wgrad_fixed_order_us"] = round(device_us(lambda: [T.conv2d_wgrad_fixed(dy, xx, 1, b) for dy, xx, b in lin], a.iters, a.warmup), 1)
        del qkv, out, dout, dqkv, lin
        if n in split:
            res["backward_by_family_us"] = split[n]
        sd = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in m.state_dict().items()}
        leaves = [x] + [sd[k] for k in TR.param_names(sd)]

        def torch_step():
            torch.autograd.grad((TR.cobevt_train_forward(sd, block_args(C), x, [n], aff) * g).sum(), leaves)
        res["torch_step_us"] = round(device_us(torch_step, max(a.iters // 4, 2), 2), 1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        torch_step()
        torch.cuda.synchronize()
        res["torch_peak_step_bytes"] = int(torch.cuda.max_memory_allocated())
        print(json.dumps(res), flush=True)
        results.append(res)
        del m, x, sd, leaves
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
