#!/usr/bin/env python3
"""Golden fixtures for TRAINING STAMP's adapter / reverter: gradients from the reference's own modules and ``AdapterLoss`` (CPU autograd).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_stamp_adapter_train.py   # writes tests/golden/stamp_adapter_train_<case>_<i>.npz

Cases (tests/stamp_adapter_train_restatement.py): ``cnx64``, ``cnx128``, ``rev64``, ``conv`` -- the module of tests/stamp_adapter_restatement.py's
case of that name, input requiring a gradient, objective ``sum(y * G)`` with a seeded ``G``; and ``step`` -- one adapter-training step,
``9 mse(FM, R(FP)) + 1 mse(FM, R(A(FM))) + 10 mse(FP, A(FM))`` through the reference's ``AdapterLoss`` (opencood/loss/adapter_loss.py) with
the alphas of the shipped yamls, ``FM`` and ``FP`` without gradient, the reverter called twice.

* Parameters, inputs and ``G`` are regenerated from seeds by the restatement (every parameter random, ``gamma`` included); a fixture holds
  the seed, float64 checksums, the reference's float64 gradient of every trained parameter (and of the input), and per tensor the relative
  rms error of the reference's own float32 gradient (the yardstick). It holds no parameters. ``smoothing`` gets no gradient in the
  reference (its forward never uses it): the tool asserts that.
* A tensor of more than DIGEST_ABOVE elements (the 1x1 convolutions and pwconv matrices of the dim-128 case) is stored as a digest:
  sum, sum of squares and the dot products with two seeded normal vectors (``digest_vectors``), all float64.
* A case is split into files below MAX_BYTES so that no file outgrows the largest committed fixture.
* The tool refuses to write unless, for every tensor, the restatement's float64 gradient equals the reference's (<= 1e-10 relative rms) and
  the reference's own float32 gradient meets the test criterion against its float64 gradient with the float32 RESTATEMENT as yardstick.
"""
from __future__ import annotations

import glob
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np
import torch

import stamp_adapter_restatement as R
import stamp_adapter_train_restatement as T
from make_golden import REF
from make_golden_stamp_adapter import build, load_reference

OUT = os.path.join(REPO, "tests", "golden")
SEED = 8300
MAX_BYTES = 950000


def reference_module_grads(ad, cls, cfg, sd, x, G, dtype):
    model = build(ad, cls, cfg, sd, dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    (model(xx) * G.to(dtype)).sum().backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(v is None for k, v in grads.items() if ".smoothing." in k), "the reference gave smoothing a gradient"
    out = {k: v for k, v in grads.items() if ".smoothing." not in k}
    assert all(v is not None for v in out.values())
    out["x"] = xx.grad
    return out


def reference_step_grads(ad, loss_cls, data, dtype):
    cfg_a, sd_a, cfg_r, sd_r, FM, FP = data
    a, r = build(ad, "Adapter", cfg_a, sd_a, dtype), build(ad, "Reverter", cfg_r, sd_r, dtype)
    crit = loss_cls(dict(T.ALPHA))
    FM, FP = FM.to(dtype), FP.to(dtype)
    FM2P = a(FM)
    loss = crit(FM, r(FP), r(FM2P), FP, FM2P)
    loss.backward()
    grads = {k: p.grad for m in (a, r) for k, p in m.named_parameters()}
    assert all(v is None for k, v in grads.items() if ".smoothing." in k)
    return float(loss.detach()), {k: v for k, v in grads.items() if ".smoothing." not in k}


def pack(name, seed, extra, g64, g32, r64, r32):
    """Check every tensor, then write the case's files."""
    store = {"seed": np.int64(seed), "keys": np.array(sorted(g64))}
    store.update(extra)
    worst = 0.0
    for i, k in enumerate(sorted(g64)):
        same = T.rel_rms(r64[k], g64[k])
        assert same <= 1e-10, f"{name} {k}: the restatement's float64 gradient is not the reference's ({same:.2e})"
        yard_r = T.rel_rms(r32[k], g64[k])
        yard = T.check(f"{name} {k} (reference float32)", g32[k], g64[k], yard_r)    # raises: nothing is written
        worst = max(worst, yard)
        store[f"yard/{k}"] = np.float64(yard)
        if g64[k].numel() > T.DIGEST_ABOVE and k != "x":
            store[f"digest64/{k}"] = T.digest(g64[k], seed, i)
        else:
            store[f"grad64/{k}"] = g64[k].numpy()
    for f in glob.glob(os.path.join(OUT, f"stamp_adapter_train_{name}_*.npz")):
        os.remove(f)
    parts, size = [{}], 0
    for k, v in store.items():
        nbytes = np.asarray(v).nbytes + 256
        if size + nbytes > MAX_BYTES and parts[-1]:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += nbytes
    for i, part in enumerate(parts):
        path = os.path.join(OUT, f"stamp_adapter_train_{name}_{i + 1}.npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 1000000, (path, os.path.getsize(path))
        print(f"  wrote {os.path.relpath(path, REPO)} ({os.path.getsize(path) / 1024:.0f} KiB)")
    print(f"case {name}: {len(g64)} tensors, seed {seed}; the reference's float32 gradients: worst relative rms error {worst:.2e}")


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    ad = load_reference()
    from opencood.loss.adapter_loss import AdapterLoss
    for ci, name in enumerate(T.TRAIN_CASES):
        seed = SEED + 10 * ci
        cls, cfg, sd, x = R.case_data(name, seed)
        prefix = R.prefix_of(cls)
        with torch.no_grad():
            shape = tuple(R.adapter_forward(cfg, sd, prefix, x).shape)
        G = T.make_G(shape, seed + 2)
        g64 = reference_module_grads(ad, cls, cfg, sd, x, G, torch.float64)
        g32 = reference_module_grads(ad, cls, cfg, sd, x, G, torch.float32)
        r64 = T.module_grads(cfg, sd, prefix, x, G, torch.float64)
        r32 = T.module_grads(cfg, sd, prefix, x, G, torch.float32)
        assert sorted(g64) == sorted(r64)
        extra = {"checksum_params": np.float64(R.checksum(sd.values())), "checksum_x": np.float64(R.checksum([x])),
                 "checksum_G": np.float64(R.checksum([G]))}
        pack(name, seed, extra, g64, g32, r64, r32)
    seed = SEED + 100
    data = T.step_data(seed)
    l64, g64 = reference_step_grads(ad, AdapterLoss, data, torch.float64)
    l32, g32 = reference_step_grads(ad, AdapterLoss, data, torch.float32)
    rl64, r64 = T.step_grads(data, torch.float64)
    _, r32 = T.step_grads(data, torch.float32)
    assert abs(rl64 - l64) <= 1e-12 * abs(l64), (rl64, l64)
    assert abs(l32 - l64) <= 1e-5 + 1e-4 * abs(l64), (l32, l64)
    extra = {"loss64": np.float64(l64), "checksum_params": np.float64(R.checksum(list(data[1].values()) + list(data[3].values()))),
             "checksum_x": np.float64(R.checksum([data[4], data[5]]))}
    pack("step", seed, extra, g64, g32, r64, r32)


if __name__ == "__main__":
    main()
