#!/usr/bin/env python3
"""Golden fixture for HEAL's PyramidFusion, from the reference's own module (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_pyramid.py   # writes tests/golden/pyramid.npz and pyramid_keys.json

``PyramidFusion`` (opencood/models/fuse_modules/pyramid_fuse.py:65-168) is imported with the import stubs of oracle/make_golden.py
(plus ``opencood.visualization.debug_plot``, which pyramid_fuse.py imports and never calls) and run in ``.eval()`` in float32 and in
float64 on the same values: the shipped num_filters / strides / upsample filters with ``resnext: true`` and layer_nums [1, 2, 1], so
the grouped 3x3 occurs at 4, 8 and 16 channels per group and at both strides. The million parameters are NOT stored: both sides
generate them from a seed (tests/pyramid_restatement.py: ``fill_params_``; BatchNorm statistics and affine parameters are random).
Stored: inputs, poses, the float64 outputs, every occ_map and, for collab, every level's fused map (what weighted_fuse returned) of

  collab   forward_collab on two scenes: a lone agent under a non-identity matrix (pixels nobody sees must be exactly 0); an identity
           ego with two generic agents and one agent entirely outside the map                                       [strict]
  crop     forward_collab with cam_crop_info (one modality at ratio 2, one at ratio 1) + the reference's crop mask per level (bool)
  single   forward_single on the first agent                                                                         [strict]
  fuse     weighted_fuse itself on random maps, scores with exact zeros inside the map, collab's poses

and per case the MARGIN mask of every level (pyramid_restatement.margin_mask): the output pixels where some agent's scoring taps
weigh in (0, 1e-4) in float64. The share must be 0 for the strict cases and at most 1e-3 for any case; the tool refuses to write a
fixture beyond that."""
from __future__ import annotations

import json
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import pyramid_restatement as R
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")


def load_reference():
    _install_stubs()
    m = types.ModuleType("opencood.visualization.debug_plot")
    m.plot_feature = lambda *a, **k: None
    sys.modules["opencood.visualization.debug_plot"] = m
    sys.path.insert(0, REF)
    import opencood.models.fuse_modules.pyramid_fuse as P
    return P


def run_collab(P, model, x, rl, aff, modalities=None, info=None):
    """The reference's forward_collab in the model's dtype; also every level's score as handed to weighted_fuse and what it returned."""
    scores, levels, orig = [], [], P.weighted_fuse

    def spy(xx, score, *a):
        scores.append(score.detach().clone())
        levels.append(orig(xx, score, *a))
        return levels[-1]

    P.weighted_fuse = spy
    try:
        with torch.no_grad():
            out, occ = model.forward_collab(torch.from_numpy(x).to(next(model.parameters()).dtype), torch.tensor(rl), torch.from_numpy(aff), modalities, info)
    finally:
        P.weighted_fuse = orig
    return out.numpy(), [o.numpy() for o in occ], scores, [v.numpy() for v in levels]


def margins(scores, rl, aff, strict, what):
    masks = [R.margin_mask(s, rl, aff).numpy() for s in scores]
    share = float(sum(int(m.sum()) for m in masks)) / sum(m.size for m in masks)
    print(f"{what}: margin share {share:.3e} ({'strict: must be 0' if strict else f'cap {R.MARGIN_CAP:.0e}'})")
    if share > (0.0 if strict else R.MARGIN_CAP):
        raise SystemExit(f"{what}: choose other poses: the margin share is a condition of the fixture")
    return masks, share


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    P = load_reference()
    cfg = R.cfg()
    torch.manual_seed(0)
    m32 = R.fill_params_(P.PyramidFusion(cfg).eval())
    m64 = R.fill_params_(P.PyramidFusion(cfg).double().eval())
    assert not m32.align_corners
    keys = [[k, list(v.shape)] for k, v in m32.state_dict().items()]
    store = {"seed": np.int64(R.SEED)}

    # ---- collab
    c = R.COLLAB
    rl, n = c["record_len"], sum(c["record_len"])
    x = R.quantised(R.SEED + 1, (n, c["C"], c["H"], c["W"]))
    aff = R.affine_of(R.collab_scenes(c["H"], c["W"]), L=5)
    o32 = run_collab(P, m32, x, rl, aff)[0]
    o64, occ64, sc64, lv64 = run_collab(P, m64, x, rl, aff)
    masks, share = margins(sc64, rl, aff, True, "collab")
    dark = float((lv64[0][0] == 0).all(0).mean())
    print(f"collab: x {x.shape} record_len {rl}; float32 vs float64 rel rms {R.rel_rms(o32, o64):.2e}; scene 0: {dark:.2f} of the pixels see nobody")
    assert o64.dtype == np.float64 and 0.05 < dark < 0.95
    store.update(collab_x=x, collab_record_len=np.asarray(rl, np.int64), collab_affine=aff, collab_out64=o64, collab_share=np.float64(share),
                 collab_rel32=np.float64(R.rel_rms(o32, o64)))
    for i in range(3):
        store[f"collab_occ64_{i}"], store[f"collab_margin_{i}"], store[f"collab_level64_{i}"] = occ64[i], masks[i], lv64[i]

    # ---- crop
    c = R.CROP
    rl, n = c["record_len"], sum(c["record_len"])
    x = R.quantised(R.SEED + 2, (n, c["C"], c["H"], c["W"]))
    aff = R.affine_of(R.crop_scenes(c["H"], c["W"]), L=5)
    o32 = run_collab(P, m32, x, rl, aff, c["modalities"], c["info"])[0]
    o64, occ64, sc64, lv64 = run_collab(P, m64, x, rl, aff, c["modalities"], c["info"])
    masks, share = margins(sc64, rl, aff, False, "crop")
    print(f"crop: x {x.shape} modalities {c['modalities']}; float32 vs float64 rel rms {R.rel_rms(o32, o64):.2e}; kept pixels per level "
          f"{[[int((s[j] != 0).sum()) for j in range(n)] for s in sc64]}")
    store.update(crop_x=x, crop_record_len=np.asarray(rl, np.int64), crop_affine=aff, crop_out64=o64, crop_share=np.float64(share),
                 crop_rel32=np.float64(R.rel_rms(o32, o64)))
    for i in range(3):
        store[f"crop_occ64_{i}"], store[f"crop_margin_{i}"], store[f"crop_mask_{i}"] = occ64[i], masks[i], (sc64[i] != 0).numpy()

    # ---- single
    x1 = store["collab_x"][:1]
    with torch.no_grad():
        s32, _ = m32.forward_single(torch.from_numpy(x1))
        s64, socc = m64.forward_single(torch.from_numpy(x1).double())
    print(f"single: float32 vs float64 rel rms {R.rel_rms(s32.numpy(), s64.numpy()):.2e}")
    store.update(single_out64=s64.numpy())
    for i in range(3):
        store[f"single_occ64_{i}"] = socc[i].numpy()

    # ---- weighted_fuse itself
    c = R.FUSE
    fx, fs = R.fuse_inputs()
    aff = store["collab_affine"]
    f64 = P.weighted_fuse(torch.from_numpy(fx).double(), torch.from_numpy(fs).double(), torch.tensor(c["record_len"]), torch.from_numpy(aff), False).numpy()
    f32 = P.weighted_fuse(torch.from_numpy(fx), torch.from_numpy(fs), torch.tensor(c["record_len"]), torch.from_numpy(aff), False).numpy()
    masks, share = margins([torch.from_numpy(fs)], c["record_len"], aff, False, "fuse")
    print(f"fuse: float32 vs float64 rel rms {R.rel_rms(f32, f64):.2e}")
    store.update(fuse_x=fx, fuse_score=fs, fuse_out64=f64, fuse_margin=masks[0], fuse_share=np.float64(share))

    path = os.path.join(OUT, "pyramid.npz")
    np.savez_compressed(path, **store)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1024:.0f} KiB)")
    assert size < (1 << 20), "the fixture must stay under 1 MiB"
    with open(os.path.join(OUT, "pyramid_keys.json"), "w") as f:
        json.dump({"model_cfg": cfg, "state_dict": keys}, f, indent=0)
    print(f"wrote pyramid_keys.json ({len(keys)} entries)")


if __name__ == "__main__":
    main()
