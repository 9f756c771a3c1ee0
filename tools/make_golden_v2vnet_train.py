#!/usr/bin/env python3
"""Golden fixtures for TRAINING the V2VNet fusion, from the reference's own module under torch autograd (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_v2vnet_train.py   # writes tests/golden/v2vnet_train.npz and tests/golden/v2vnet_train_d.npz

``V2VNetFusion`` (opencood/models/fuse_modules/fusion_in_one.py:238-353) is run in float32 and in float64 on the same values and
``out.backward(grad_out)`` with a seeded upstream gradient, for the cases a, c, d of tests/golden/v2vnet.npz (weights, inputs and poses
are loaded from it, not stored again) and for the max case ``bt`` of tests/v2vnet_train_restatement.py, which replaces the forward
fixture's b: b's smallest float64 margin between the winner and the runner-up of a max is the size of float32 rounding. The tool takes
the first seed in 0..31 whose ``margin_report`` meets: smallest float64 margin over the live positions >= 16 x the largest
|message32 - message64|, and identical float32 / float64 winner maps; seed, margin and ratio are stored.

Stored per case: ``grad_out``; the reference's float64 gradients of x (``gx64_<case>``) and of every parameter (``g64_<case>/<name>``;
a parameter the reference leaves without gradient is absent); per tensor the relative rms error of the reference's own float32
gradients against them (``ref_rel_rms_<case>/<name>``, ``.../x``): the GPU tests' yardsticks. Case d (C = 32) goes to a file of its own;
each file stays under 1 MiB.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import v2vnet_restatement as R
import v2vnet_train_restatement as TR
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")
SEED = 6200


def load_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    from opencood.models.fuse_modules.fusion_in_one import V2VNetFusion
    return V2VNetFusion


def reference_grads(V2VNetFusion, args, sd, x, rl, aff, grad_out, dtype):
    torch.manual_seed(0)
    m = V2VNetFusion(args).eval()
    m.load_state_dict(sd, strict=True)
    m = m.to(dtype)
    xx = torch.from_numpy(x).to(dtype).requires_grad_()
    out = m(xx, torch.tensor(rl), torch.from_numpy(aff))
    out.backward(torch.from_numpy(grad_out).to(dtype))
    return out.detach().numpy(), xx.grad.numpy(), {k: (None if p.grad is None else p.grad.numpy()) for k, p in m.named_parameters()}


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixtures can only be regenerated in the build container")
    V2VNetFusion = load_reference()
    from test_v2vnet import load_v2vnet_case
    stores = {"v2vnet_train": {"seed": np.int64(SEED)}, "v2vnet_train_d": {"seed": np.int64(SEED)}}
    for i, tag in enumerate(TR.TRAIN_CASES):
        store = stores["v2vnet_train_d" if tag == "d" else "v2vnet_train"]
        args = TR.case_args(tag)
        if tag == "bt":
            for s in range(32):
                sd, x, aff = TR.bt_inputs(s)
                rep = TR.margin_report(sd, args, x, TR.BT["record_len"], aff)
                ok = rep["ratio"] >= TR.MARGIN_FACTOR and rep["same_winners"]
                print(f"  bt seed {s}: live positions {rep['live']}, margin {rep['margin']:.3e}, float32 message error {rep['err']:.3e}, ratio "
                      f"{rep['ratio']:.1f}, same winners {rep['same_winners']}{'  <- taken' if ok else ''}")
                if ok:
                    break
            else:
                raise AssertionError("no seed in 0..31 meets the margin condition")
            rl = list(TR.BT["record_len"])
            store.update({"x_bt": x, "affine_bt": aff, "bt_seed": np.int64(s), "bt_margin": np.float64(rep["margin"]),
                          "bt_ratio": np.float64(rep["ratio"]), "bt_live": np.int64(rep["live"])})
            for k, v in sd.items():
                store[f"w_bt/{k}"] = v.numpy()
        else:
            _, sd, x, rl, aff, *_ = load_v2vnet_case(tag)
        C, H, W = x.shape[1:]
        grad_out = np.random.RandomState(SEED + i).standard_normal((len(rl), C, H, W)).astype(np.float32)
        o32, gx32, g32 = reference_grads(V2VNetFusion, args, sd, x, rl, aff, grad_out, torch.float32)
        o64, gx64, g64 = reference_grads(V2VNetFusion, args, sd, x, rl, aff, grad_out, torch.float64)
        assert gx64.dtype == np.float64 and gx32.dtype == np.float32
        _, rx, rg = TR.restatement_grads(sd, args, x, rl, aff, grad_out, torch.float64)
        store.update({f"grad_out_{tag}": grad_out, f"gx64_{tag}": gx64, f"ref_rel_rms_{tag}/x": np.float64(R.rel_rms(gx32, gx64))})
        print(f"case {tag}: {args}\n  d x: reference float32 vs float64 rel rms {R.rel_rms(gx32, gx64):.3e}; restatement autograd vs reference in "
              f"float64 {R.rel_rms(rx, gx64):.2e}")
        for k, v in g64.items():
            if v is None:
                assert g32[k] is None and rg[k] is None, k
                print(f"  {k}: no gradient")
                continue
            e = R.rel_rms(g32[k], v)
            print(f"  {k} {tuple(v.shape)}: reference float32 vs float64 rel rms {e:.3e}; restatement {R.rel_rms(rg[k], v) if rg[k] is not None else float('nan'):.2e}")
            store[f"g64_{tag}/{k}"] = v
            store[f"ref_rel_rms_{tag}/{k}"] = np.float64(e)
    for name, store in stores.items():
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **store)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
