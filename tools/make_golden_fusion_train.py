#!/usr/bin/env python3
"""Golden fixtures for training the max fusion and for the who2com fusion, from the reference's own modules (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_fusion_train.py   # writes tests/golden/maxfuse_train.npz, who2com.npz and who2com_keys.json

``MaxFusion`` (opencood/models/fuse_modules/fusion_in_one.py:87-124) and ``Who2comFusion`` (:521-574) are imported with the import
stubs of oracle/make_golden.py and run in float32 and in float64 on the same values. Stored: the inputs, ``record_len``, the
normalised pairwise matrices [B, L, L, 2, 3] float64, a probe ``G``, the outputs and the gradients of L = <G, out> with respect to
``x`` (and, for who2com, ``decode_layer``'s weight and bias, which are stored too) in both precisions.

The max fixture also stores the NEAR-TIE SHARE: the fraction of (scene, channel, pixel) where the float64 top two warped values
differ by less than 1e-5 max|x| without being equal. ``G`` is zero exactly there (those elements are excluded from the gradient
comparison); the share may be at most 1e-3 and the tool refuses to write a fixture that exceeds it. Exact ties are not excluded:
the non-ego agents are post-ReLU maps and two agents leave the map, so agents tie at an exact 0 on a good part of it.
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import fusion_train_restatement as R
from gencomm_amd import synth
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")
SEED = 5200


def load_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    from opencood.models.fuse_modules.fusion_in_one import MaxFusion, Who2comFusion
    return MaxFusion, Who2comFusion


def scenes(H, W):
    I = R.theta(H, W)
    return [[I, R.rot(H, W, 0.4, 1.37, -0.61)], [I, R.theta(H, W, 0.0, 1.0, 0.63, 1.29), R.theta(H, W, tx=3.0 * W + 0.37)],
            [I], [I, R.theta(H, W, -1.0, 0.0, -1.63, 0.37), R.rot(H, W, -0.9, 2.21, 1.43), R.theta(H, W, ty=-2.0 * H - 0.37)]]


def run(model, x, rl, aff, G, dtype, params=()):
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = model(xx, torch.tensor(rl), torch.from_numpy(aff))
    assert out.dtype == dtype
    grads = torch.autograd.grad((out * torch.from_numpy(G).to(dtype)).sum(), [xx, *params])
    return [out.detach().numpy()] + [g.numpy() for g in grads]


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixtures can only be regenerated in the build container")
    MaxFusion, Who2comFusion = load_reference()
    rl = [2, 3, 1, 4]
    n = sum(rl)

    # ---- max
    C, H, W = 6, 12, 20
    rng = np.random.RandomState(SEED)
    x = rng.standard_normal((n, C, H, W))
    ego = np.cumsum([0] + rl[:-1])
    keep = x[ego].copy()
    x = np.maximum(x, 0.0)            # the non-ego agents are post-ReLU maps; the egos stay continuous (tests/fusion_train_restatement.py)
    x[ego] = keep
    x = x.astype(np.float32)
    aff = R.affine_of(scenes(H, W), L=5)
    near = R.near_tie_mask(x, rl, aff).numpy()
    share = float(near.mean())
    G = R.probe(SEED + 1, (len(rl), C, H, W)) * ~near
    model = MaxFusion()
    o32, d32 = run(model, x, rl, aff, G, torch.float32)
    o64, d64 = run(model, x, rl, aff, G, torch.float64)
    w = R.warp_to_ego(torch.from_numpy(x).double(), rl, torch.from_numpy(aff))
    ties = sum(int((torch.topk(v, 2, dim=0)[0].diff(dim=0) == 0).sum()) for v in w if v.shape[0] > 1)
    print(f"max: x {x.shape} record_len {rl}; near-tie share {share:.3e} (cap {R.NEAR_TIE_CAP:.0e}), exact ties {ties} of {near.size}; "
          f"float32 vs float64: out {R.rel_rms(o32, o64):.2e}, dx {R.rel_rms(d32, d64):.2e}")
    assert share <= R.NEAR_TIE_CAP, "choose another seed: the near-tie share is a condition of the fixture"
    assert ties > 0.05 * near.size
    assert np.array_equal(R.max_fusion_forward(torch.from_numpy(x), rl, torch.from_numpy(aff)).numpy(), o32)
    path = os.path.join(OUT, "maxfuse_train.npz")
    np.savez_compressed(path, x=x, record_len=np.asarray(rl, np.int64), affine=aff, G=G.astype(np.float32), out32=o32, dx32=d32, out64=o64, dx64=d64,
                        near_tie_share=np.float64(share), exact_ties=np.int64(ties), seed=np.int64(SEED))
    assert os.path.getsize(path) < (1 << 20)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")

    # ---- who2com
    C, H, W = 8, 12, 20
    x = np.maximum(np.random.RandomState(SEED + 2).standard_normal((n, C, H, W)), 0.0).astype(np.float32)
    aff = R.affine_of(scenes(H, W), L=5)
    G = R.probe(SEED + 3, (len(rl), C, H, W))
    torch.manual_seed(0)
    model = Who2comFusion(C)
    synth.fill_params_(model, SEED + 4)
    wt, bs = model.decode_layer.weight.detach().numpy().copy(), model.decode_layer.bias.detach().numpy().copy()
    o32, d32, gw32, gb32 = run(model, x, rl, aff, G, torch.float32, [model.decode_layer.weight, model.decode_layer.bias])
    model = model.double()
    o64, d64, gw64, gb64 = run(model, x, rl, aff, G, torch.float64, [model.decode_layer.weight, model.decode_layer.bias])
    assert list(o32.shape) == [len(rl), C, H, W]
    print(f"who2com: x {x.shape} record_len {rl}; float32 vs float64: out {R.rel_rms(o32, o64):.2e}, dx {R.rel_rms(d32, d64):.2e}, "
          f"d weight {R.rel_rms(gw32, gw64):.2e}, d bias {R.rel_rms(gb32, gb64):.2e}")
    path = os.path.join(OUT, "who2com.npz")
    np.savez_compressed(path, x=x, record_len=np.asarray(rl, np.int64), affine=aff, G=G, weight=wt, bias=bs, out32=o32, dx32=d32, gw32=gw32, gb32=gb32,
                        out64=o64, dx64=d64, gw64=gw64, gb64=gb64, seed=np.int64(SEED))
    assert os.path.getsize(path) < (1 << 20)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    shipped = Who2comFusion(128)   # `who2com: 128`: the reference's shells pass the block itself as feature_dims
    keys = [[k, list(v.shape)] for k, v in shipped.state_dict().items()]
    assert [k for k, _ in keys] == ["decode_layer.weight", "decode_layer.bias"]
    with open(os.path.join(OUT, "who2com_keys.json"), "w") as f:
        json.dump({"args": 128, "state_dict": keys}, f, indent=0)
    print(f"wrote who2com_keys.json ({len(keys)} entries)")


if __name__ == "__main__":
    main()
