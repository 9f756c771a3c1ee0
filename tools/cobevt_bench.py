#!/usr/bin/env python3
"""CoBEVT fusion timing on a 64 x 128 map, one scene of agent_size 5 with 2 and with 5 agents present: the shipped `cobevt:` block
(input_dim 256, mlp_dim 256, window_size 4, dim_head 32, depth 3) and the same block at input_dim 128. Device time per call: warm-up,
then the mean over `--iters` calls enqueued back to back between two events on the stream, then a synchronisation.

Reported per shape:
  swap attention   gencomm_swap_attn_fwd alone (window and grid partition) against its algorithmic bytes -- the qkv maps read once,
                   the output written once -- at `--hbm-tbps` (default 8.0, the MI355X's HBM3E peak): time / floor. The 2-agent scene
                   still has 5 rows of queries (padded agents are queries); only its keys are fewer.
  forward          the whole CoBEVT.forward (warp, `depth` x {LN, qkv, attention, out, LN, FFN} x 2, mean, LN, Linear)
  launches         kernel launches of one steady-state forward, counted in the kernel trace of a `rocprofv3 --kernel-trace --stats`
                   run of this script's `--forward-only` mode (a fresh child process, --profile)
  torch            for orientation only: tests/cobevt_restatement.py run with torch on the same GPU (float32)

    python tools/cobevt_bench.py [--iters 50] [--warmup 5] [--profile] [--out profiles/cobevt_bench.json]

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

import numpy as np
import torch

H, W, L = 64, 128, 5
SHAPES = [(256, 2), (256, 5), (128, 2), (128, 5)]   # (input_dim, agents present)


def block_args(C):
    return {"input_dim": C, "mlp_dim": C, "agent_size": L, "window_size": 4, "dim_head": 32, "drop_out": 0.1, "depth": 3}


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


def setup(C, n, dev):
    import cobevt_restatement as R
    from gencomm_amd import CoBEVT, synth
    m = CoBEVT(block_args(C)).eval()
    synth.fill_params_(m, 9)
    rng = np.random.RandomState(10 + n)
    x = torch.from_numpy(np.maximum(rng.standard_normal((n, C, H, W)), 0.0).astype(np.float32)).to(dev)
    aff = torch.from_numpy(R.make_affine([n], L, H, W, 11)).to(dev)
    return m.to(dev), x, aff


def launches_per_forward(C, n, iters):
    """Launches between the last two agent_mean_kernel dispatches of a traced `--forward-only` child (one forward = one mean)."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="cobevt_prof_")
    cmd = [rocprof, "--kernel-trace", "--stats", "-d", tmp, "-o", "cobevt", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
           "--forward-only", f"{C},{n}", "--iters", str(iters), "--warmup", "1"]
    subprocess.run(cmd, check=True, timeout=600)
    found = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if not found:
        raise RuntimeError(f"rocprofv3 wrote no kernel_trace.csv under {tmp}")
    rows = sorted(csv.DictReader(open(found[0])), key=lambda r: int(r["Start_Timestamp"]))
    shutil.rmtree(tmp, ignore_errors=True)
    ends = [i for i, r in enumerate(rows) if "agent_mean_kernel" in r["Kernel_Name"]]
    gaps = {b - a for a, b in zip(ends[1:], ends[2:])}          # the first forward also prepares the weights
    assert len(ends) == iters + 1 and len(gaps) == 1, (len(ends), gaps)
    return gaps.pop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-tbps", type=float, default=8.0)
    ap.add_argument("--profile", action="store_true", help="count the launches of a forward in a rocprofv3 kernel trace (fresh child processes)")
    ap.add_argument("--forward-only", default="", metavar="C,N", help="run only the forward of one shape (the child of --profile)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cobevt_bench.json"))
    a = ap.parse_args()
    launches = {}
    if a.profile:   # before this process opens the GPU
        for C, n in SHAPES[:2]:   # the shipped block; the launch sequence does not depend on input_dim
            launches[(C, n)] = launches_per_forward(C, n, 4)
    dev = torch.device("cuda:0")
    if a.forward_only:
        C, n = (int(v) for v in a.forward_only.split(","))
        m, x, aff = setup(C, n, dev)
        with torch.no_grad():
            device_us(lambda: m(x, [n], aff), a.iters, a.warmup)
        return
    import cobevt_restatement as R
    from gencomm_amd import _lib
    from gencomm_amd.runtime import ptr, stream_ptr
    l = _lib.lib()
    results = []
    for C, n in SHAPES:
        m, x, aff = setup(C, n, dev)
        heads, dh, ws = C // 32, 32, 4
        qkv = torch.randn(L, 3 * C, H, W, device=dev)
        table = torch.rand((2 * L - 1) * (2 * ws - 1) ** 2, heads, device=dev)
        nv = torch.tensor([n], dtype=torch.int32, device=dev)
        out = torch.empty(L, C, H, W, device=dev)
        st = stream_ptr(dev)
        floor_us = (qkv.numel() + out.numel()) * 4 / (a.hbm_tbps * 1e12) * 1e6
        res = {"input_dim": C, "map": f"{H}x{W}", "agent_size": L, "agents_present": n, "window_size": ws, "dim_head": dh, "depth": 3,
               "attn_algorithmic_bytes": (qkv.numel() + out.numel()) * 4, "attn_floor_us": round(floor_us, 2)}
        for name, grid in (("window", 0), ("grid", 1)):
            us = device_us(lambda: _lib.check(l.gencomm_swap_attn_fwd(ptr(qkv), ptr(table), ptr(nv), ptr(out), 1, L, heads, dh, ws, H, W, grid, st),
                                              "gencomm_swap_attn_fwd"), a.iters, a.warmup)
            res[f"attn_{name}_us"] = round(us, 2)
            res[f"attn_{name}_times_floor"] = round(us / floor_us, 1)
        with torch.no_grad():
            res["forward_us"] = round(device_us(lambda: m(x, [n], aff), a.iters, a.warmup), 1)
            sd = {k: v.detach() for k, v in m.state_dict().items()}
            args = block_args(C)
            res["torch_restatement_us"] = round(device_us(lambda: R.cobevt_forward(sd, args, x, [n], aff), max(a.iters // 5, 2), 2), 1)
        if (C, n) in launches:
            res["launches_per_forward"] = launches[(C, n)]
        print(json.dumps(res), flush=True)
        results.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "hbm_tbps": a.hbm_tbps, "results": results},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
