#!/usr/bin/env python3
"""Golden fixtures of the TRAINABLE MPDA feature aligner: outputs and gradients of the reference's own modules (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_mpda_train.py      # writes tests/golden/mpda_train_<case>.npz (+ _f64.npz where one file would be too large)

The modules are imported from ``opencood.models.mpda_modules`` as tools/make_golden_mpda.py imports them (they need ``einops``); the
aligner's loop is that file's ``Aligner``. float64 autograd is the truth, the same step in float32 the yardstick. Parameters come from
``synth.fill_params_`` / ``fill_bn_stats_`` seeds and inputs from seeds (``mpda_train_restatement.case_seed`` / ``case_inputs``): neither
is stored. Stored per case of ``mpda_train_restatement.TRAIN_CASES``, in the ``y32`` / ``d64`` form of ``mpda.npz`` (``d64 = float32(y32 -
y64)``; the tests rebuild y64 = y32 - d64 in float64 and compute the yardstick's own error from the pair): the output(s), the input
gradients ``d_<input>``, every parameter gradient ``g:<name>`` and, for the ``train()`` case, the BatchNorm running statistics after the
step ``rs:<name>``. Loss: ``sum(out * functional)`` with a seeded functional; the aligner cases add BCE-with-logits on ``class_logits``
against the shell's labels (0 ego, 1 collaborator), so the gradient-reversal layer is exercised.

Kink condition: LeakyReLU (the resizer's residual blocks) and ReLU (the classifier) are not differentiable at 0. The generator records
every such pre-activation in both runs, ASSERTS that none changes sign between float32 and float64, and prints the smallest
|pre-activation| / rms per case. If a seed fails, change the seed; no element is ever masked out.
"""
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
import torch.nn as nn

import mpda_restatement as R
import mpda_train_restatement as TR
from gencomm_amd import synth
from make_golden import REF
from make_golden_mpda import Aligner, load_reference

OUT = os.path.join(REPO, "tests", "golden")
LIMIT = 900 << 10   # one committed file stays well under 1 MiB


def build(refs, tag, dtype):
    LearnableResizer, CrossDomainFusionEncoder, DAImgHead = refs
    c, args = TR.TRAIN_CASES[tag], TR.case_args(tag)
    torch.manual_seed(0)
    m = {"resizer": lambda: LearnableResizer(args["resizer"]), "cdt": lambda: CrossDomainFusionEncoder(args["cdt"]),
         "da": lambda: DAImgHead(TR.C), "align": lambda: Aligner(refs, args)}[c["kind"]]()
    synth.fill_params_(m, TR.case_seed(tag))
    synth.fill_bn_stats_(m, TR.case_seed(tag) + 50)
    m = m.train() if c["mode"] == "train" else m.eval()
    return m.to(dtype)


def run(refs, tag, dtype):
    """One step of the reference's module -> (dict of numpy arrays under the fixture's names, list of kink pre-activations)."""
    c = TR.TRAIN_CASES[tag]
    m = build(refs, tag, dtype)
    pre, hooks = [], []
    for mod in m.modules():
        if isinstance(mod, nn.LeakyReLU):
            hooks.append(mod.register_forward_hook(lambda _m, inp, _out: pre.append(inp[0].detach().numpy().copy())))
        if type(mod).__name__ == "DAImgHead":
            hooks.append(mod.conv1_da.register_forward_hook(lambda _m, _inp, out: pre.append(out.detach().numpy().copy())))
    t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in TR.case_inputs(tag)]
    fn = lambda shape: torch.from_numpy(TR.functional(tag, shape)).to(dtype)
    rec = {}
    if c["kind"] == "resizer":
        out = m(t[0], t[1])
        loss, ins = (out * fn(out.shape)).sum(), {"cav": t[1]}
        rec["out"] = out
    elif c["kind"] == "cdt":
        out = m(t[0].repeat(t[1].shape[0], 1, 1, 1), t[1])
        loss, ins = (out * fn(out.shape)).sum(), {"ego": t[0], "cav": t[1]}
        rec["out"] = out
    elif c["kind"] == "da":
        out = m(t[0])
        loss, ins = (out * fn(out.shape)).sum(), {"x": t[0]}
        rec["out"] = out
    else:
        aligned, logits = m(t[0], c["record_len"])
        loss, ins = TR.align_loss(aligned, logits, fn(aligned.shape), c["record_len"]), {"x": t[0]}
        rec["aligned"], rec["logits"] = aligned, logits
    loss.backward()
    for h in hooks:
        h.remove()
    for k, v in ins.items():
        rec["d_" + k] = v.grad
    for k, p in m.named_parameters():
        rec["g:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    if c["mode"] == "train":
        for k, b in m.named_buffers():
            if k.endswith(("running_mean", "running_var")):
                rec["rs:" + k] = b
            if k.endswith("num_batches_tracked"):
                assert int(b) == 1
    return {k: v.detach().numpy().copy() for k, v in rec.items()}, pre


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixtures can only be regenerated in the build container")
    refs = load_reference()
    for tag in TR.TRAIN_CASES:
        r32, pre32 = run(refs, tag, torch.float32)
        r64, pre64 = run(refs, tag, torch.float64)
        assert list(r32) == list(r64) and len(pre32) == len(pre64)
        kink = float("inf")
        for a, b in zip(pre32, pre64):
            assert np.array_equal(a > 0, b > 0), f"case {tag}: a pre-activation changes sign between float32 and float64: change the seed"
            kink = min(kink, float(np.abs(b).min() / np.sqrt((b ** 2).mean())))
        y32s, d64s, worst = {}, {}, ("", 0.0)
        for k in r32:
            y32, y64 = r32[k], r64[k]
            assert y32.dtype == np.float32 and y64.dtype == np.float64 and np.isfinite(y64).all(), k
            d64 = (y32.astype(np.float64) - y64).astype(np.float32)
            y32s["y32/" + k], d64s["d64/" + k] = y32, d64
            if np.abs(y64).max() > 0:
                e = R.rel_rms(y32, y64)
                worst = max(worst, (k, e), key=lambda kv: kv[1])
        print(f"case {tag}: {len(r32)} tensors, {sum(v.size for v in r32.values())} values; {len(pre64)} kink layers, smallest |pre-activation| / rms "
              f"{kink:.3e}; worst float32 error {worst[1]:.3e} ({worst[0]})")
        path = os.path.join(OUT, f"mpda_train_{tag}.npz")
        for stale in (path, path[:-4] + "_f64.npz"):
            if os.path.exists(stale):
                os.remove(stale)
        np.savez_compressed(path, **y32s, **d64s)
        if os.path.getsize(path) > LIMIT:
            np.savez_compressed(path, **y32s)
            np.savez_compressed(path[:-4] + "_f64.npz", **d64s)
        for p in (path, path[:-4] + "_f64.npz"):
            if os.path.exists(p):
                assert os.path.getsize(p) < (1 << 20), p
                print(f"  wrote {os.path.basename(p)} ({os.path.getsize(p) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
