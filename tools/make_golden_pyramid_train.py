#!/usr/bin/env python3
"""Golden fixtures for TRAINING HEAL's PyramidFusion, from the reference's own module (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_pyramid_train.py   # writes tests/golden/pyramid_train_<case>_<k>.npz

``PyramidFusion`` is imported as tools/make_golden_pyramid.py imports it and takes ONE step per case (tests/pyramid_train_restatement.py:
``CASES``, ``run_case``) in float64 (the truth) and in float32 (the yardstick), at the shipped filters with ``resnext: true`` and
layer_nums [1, 2, 1] on 24 x 40 maps; the parameters come from the seed (``pyramid_restatement.fill_params_``) and are not stored.

  train    train() mode, forward_collab on the forward fixture's two scenes, cam_crop_info passed (and ignored, as the reference does when
           self.training); loss = fixed cotangents on the fused feature and on every occ_map
  frozen   eval(), every parameter frozen, the input trainable, crop mask on: the input gradient only
  single   train(), forward_single

Stored per case: the float64 loss, the whole float64 input gradient, every parameter gradient (whole up to 4096 elements, else a
fixed-stride sample + sum + L2 norm), every BatchNorm's running statistics after the step, and per tensor ``e32/<key>``: the relative
rms error of the reference's float32 step against its float64 step -- the tests' error bar is twice that. Arrays that do not fit one
file of 880 KiB are split over several (``save_sharded``).

The 0 -> -inf step of the fuse is a kink: the tool REFUSES a case in which the margin rule (``pyramid_restatement.margin_mask``) marks
any output pixel at any level -- the gather mixes output pixels, so a marked pixel cannot be masked out of a gradient afterwards."""
from __future__ import annotations

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

import pyramid_restatement as R
import pyramid_train_restatement as TR
from make_golden import REF
from make_golden_pyramid import load_reference


def spy_scores(P, model, name):
    """The float64 scores the reference hands to weighted_fuse in case `name` (no gradients)."""
    scores, orig = [], P.weighted_fuse

    def spy(xx, score, *a):
        scores.append(score.detach().clone())
        return orig(xx, score, *a)

    x, rl, aff, _, _ = TR.case_inputs(name)
    P.weighted_fuse = spy
    try:
        model.train(TR.CASES[name][0] == "train")
        with torch.no_grad():
            model.forward_collab(torch.from_numpy(x).double(), torch.tensor(rl), torch.from_numpy(aff), TR.MODALITIES, TR.CROP_INFO)
    finally:
        P.weighted_fuse = orig
    return scores, rl, aff


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    P = load_reference()
    cfg = R.cfg()
    for name, (mode, frozen, fwd) in TR.CASES.items():
        torch.manual_seed(0)
        store = {}
        if fwd == "collab":
            probe = R.fill_params_(P.PyramidFusion(cfg).double())
            if mode == "train":
                # the margin rule is about the forward the step takes: batch statistics, without moving the running ones
                for m in probe.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.momentum = 0.0
            scores, rl, aff = spy_scores(P, probe, name)
            for i, s in enumerate(scores):
                mask = R.margin_mask(s, rl, aff).numpy()
                print(f"{name}: level {i}: {int(mask.sum())} marked pixels of {mask.size}; zero scores {int((s == 0).sum())}")
                if mask.any():
                    raise SystemExit(f"{name}: choose other poses: an empty margin mask is a condition of the gradient fixtures")
                store[f"margin_{i}"] = mask
        m64 = R.fill_params_(P.PyramidFusion(cfg).double())
        m32 = R.fill_params_(P.PyramidFusion(cfg))
        r64, r32 = TR.run_case(m64, name, torch.float64), TR.run_case(m32, name, torch.float32)
        store["loss"] = TR.np64(r64["loss"])
        store["e32/loss"] = np.float64(abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"])))
        store["dx"] = TR.np64(r64["dx"])
        store["e32/dx"] = np.float64(TR.rel_rms(TR.np64(r32["dx"]), store["dx"]))
        for i, o in enumerate(r64["occs"]):
            store[f"occ_{i}"] = TR.np64(o)
        for k, g in r64["grads"].items():
            TR.summarise(store, "grad/" + k, g)
            store["e32/grad/" + k] = np.float64(TR.rel_rms(TR.np64(r32["grads"][k]), TR.np64(g)))
        if mode == "train":
            for k, v in r64["stats"].items():
                store["stat/" + k] = TR.np64(v)
                if not k.endswith("num_batches_tracked"):
                    store["e32/stat/" + k] = np.float64(TR.rel_rms(TR.np64(r32["stats"][k]), TR.np64(v)))
        assert frozen == (len(r64["grads"]) == 0)
        e = {k: float(v) for k, v in store.items() if k.startswith("e32/")}
        worst = max(e, key=e.get)
        print(f"{name}: loss {float(store['loss']):.6e}; float32 vs float64: dx {e['e32/dx']:.2e}, worst tensor {worst} {e[worst]:.2e}; "
              f"{len(r64['grads'])} parameter gradients")
        paths = TR.save_sharded(os.path.join(TR.GOLDEN, f"pyramid_train_{name}"), store)
        print(f"{name}: wrote {[(os.path.basename(p), os.path.getsize(p) // 1024) for p in paths]} (KiB)")


if __name__ == "__main__":
    main()
