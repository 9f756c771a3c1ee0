#!/usr/bin/env python3
"""Golden fixture of one TRAINING step of the Lift-Splat-Shoot camera encoder, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_lss_train.py      # writes tests/golden/lss_train.npz

The reference's ``LiftSplatShoot`` (import stubs and ``torch.device`` mapping of tools/make_golden_lss.py) runs in ``.train()`` mode
(batch-statistics BatchNorm, running statistics updated) on the inputs of tests/golden/lss.npz -- B = 2, N = 2, 64 x 128 images, C = 8,
weights ``synth.fill_params_(module, SEED)`` / ``synth.fill_running_stats_(module, SEED)`` -- followed by its ``FocalLoss``
(opencood/loss/point_pillar_depth_loss.py:105-185, alpha 0.25, gamma 2, ``.mean() * 1.0`` as the m4 yamls weigh it). The loss is

    L = <G, bev> + depth_loss,      G = cotangent(SEED, bev.shape): seeded, on a 1/16 grid (the tests rebuild it from the seed)

and one ``L.backward()`` gives what is stored: the two loss values, d L / d depth_logit and d L / d (image features), the gradients of
a handful of parameters along the trunk (stem, first and last block, both heads) and the running statistics of the first and last
BatchNorm after the step; besides, ``focal_eval_loss`` / ``focal_eval_grad``: the reference's FocalLoss alone on the depth logits of
lss.npz, value and gradient (the training step's d depth_logit holds the splat's part too). For each stored array ``e_ref__<name>`` is the relative rms error of that fp32 result against a float64 run
of the same modules on the same cells (the fp32 geometry is kept, so that no frustum point changes its cell between the two runs):
the reference's own rounding error, which is what the tests scale their criterion by.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

from gencomm_amd import synth
from make_golden_lss import OUT, SEED, cells_of, load_reference, small_args

PARAMS = ("conv1.weight", "bn1.weight", "layer1.0.conv2.weight", "layer2.0.downsample.0.weight", "layer2.3.bn3.bias", "depth_head.weight",
          "depth_head.bias", "image_head.weight")
STATS = ("bn1.running_mean", "bn1.running_var", "layer2.3.bn3.running_mean", "layer2.3.bn3.running_var")
CAMS = ("rots", "trans", "intrins", "post_rots", "post_trans")


def cotangent(seed, shape):
    """The seeded cotangent of the BEV map: values on a 1/16 grid in [-2, 2] (tests/test_gpu_lss_train.py rebuilds it)."""
    rng = np.random.RandomState(seed + 1000)
    return (np.clip(np.round(16 * rng.standard_normal(shape)), -32, 32) / 16).astype(np.float32)


def run(he, focal, inp, dtype, geom32=None):
    """One training step of the reference's modules in `dtype`; returns (dict of results, the fp32 geometry)."""
    torch.set_default_dtype(dtype)   # voxel_pooling allocates its output with torch.zeros(...) of the default dtype
    try:
        model = he.LiftSplatShoot(small_args()).train()
        synth.fill_params_(model, SEED)
        synth.fill_running_stats_(model, SEED)
        model = model.to(dtype)
        if geom32 is not None:       # the float64 run keeps the fp32 run's geometry: identical cells
            model.get_geometry = lambda *a: geom32
        t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
        t["imgs"] = t["imgs"].to(dtype)
        kept = {}

        def keep(_module, _inputs, output):   # the image features: an intermediate whose gradient is stored
            output.retain_grad()
            kept["feat"] = output

        hook = model.camencode.image_head.register_forward_hook(keep)
        bev = model({"inputs_m4": dict(t)}, "m4")
        hook.remove()
        depth_logit, depth_gt = model.depth_items
        depth_logit.retain_grad()
        G = torch.from_numpy(cotangent(SEED, tuple(bev.shape))).to(dtype)
        bev_term = (G * bev).sum()
        depth_loss = focal(depth_logit, depth_gt).mean() * 1.0
        (bev_term + depth_loss).backward()
        enc = model.camencode
        named = dict(enc.named_parameters())
        bufs = dict(enc.named_buffers())
        res = {"loss_bev": bev_term.detach(), "loss_depth": depth_loss.detach(), "d_depth_logit": depth_logit.grad, "d_feat": kept["feat"].grad}
        res.update({"grad__" + k: named[k].grad for k in PARAMS})
        res.update({"stat__" + k: bufs[k] for k in STATS})
        with torch.no_grad():
            geom = model.get_geometry(*[t[k] for k in CAMS]) if geom32 is None else geom32
            cell = cells_of(model, geom)
        return {k: v.detach().numpy().copy() for k, v in res.items()}, geom, cell.numpy(), depth_gt.numpy()
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    he = load_reference()
    import build_ref
    assert build_ref.build(), "oracle/_ref/box_overlaps could not be built"   # the loss module imports the post-processor (unused by it)
    import opencood.utils as ou
    sys.modules["opencood.utils.box_overlaps"] = ou.box_overlaps = build_ref.load_box_overlaps()
    from opencood.loss.point_pillar_depth_loss import FocalLoss
    focal = FocalLoss(alpha=0.25, gamma=2.0, reduction="none")
    g = np.load(os.path.join(OUT, "lss.npz"))
    inp = {k: g[k].astype(np.float32) for k in ("imgs",) + CAMS}
    torch.manual_seed(0)
    r32, geom32, cell, depth_gt = run(he, focal, inp, torch.float32)
    r64, _, cell64run, _ = run(he, focal, inp, torch.float64, geom32)
    assert np.array_equal(cell, g["cell"]) and np.array_equal(cell, cell64run) and np.array_equal(depth_gt, g["depth_gt_indices"])

    # the condition of the end-to-end test: pixels with any of their D points in a different cell under exact geometry stay below 1 %
    from lss_restatement import cells64, geometry64
    c64, _ = cells64(geometry64(g["frustum"], *[g[k] for k in CAMS]), small_args()["grid_conf"])
    BN, D, fH, fW = r32["d_depth_logit"].shape
    flipped = (c64.reshape(BN, D, fH * fW) != cell.reshape(BN, D, fH * fW)).any(1)
    print(f"pixels with a frustum point in another cell under float64 geometry: {int(flipped.sum())} of {flipped.size}")
    assert flipped.mean() <= 0.01

    # the reference's FocalLoss alone, value and gradient, on the (eval-mode) depth logits that lss.npz already stores: what the CPU test
    # of the criteria's composed depth term compares with
    lg = torch.from_numpy(g["depth_logit"]).requires_grad_(True)
    fl = focal(lg, torch.from_numpy(g["depth_gt_indices"])).mean() * 1.0
    fl.backward()
    out = {"seed": np.int64(SEED), "focal_eval_loss": np.float32(fl.item()), "focal_eval_grad": lg.grad.numpy()}
    for k, v in r32.items():
        ref = r64[k]
        e = float(np.sqrt(((v.astype(np.float64) - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))
        out[k] = v.astype(np.float32)
        out["e_ref__" + k] = np.float64(e)
        print(f"{k:45s} shape {str(v.shape):20s} rms {np.sqrt((ref ** 2).mean()):.3e}  e_ref {e:.2e}")
    path = os.path.join(OUT, "lss_train.npz")
    np.savez_compressed(path, **out)
    print("lss_train.npz:", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
