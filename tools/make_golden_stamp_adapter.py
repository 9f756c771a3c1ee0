#!/usr/bin/env python3
"""Golden fixture for STAMP's adapter / reverter, from the reference's own modules (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_stamp_adapter.py   # writes tests/golden/stamp_adapter.npz

``Adapter`` / ``Reverter`` (opencood/models/stamp_modules/adapter.py:759-804) are imported with the import stubs of oracle/make_golden.py
plus one more the tool installs itself: ``positional_encodings.torch_encodings`` (``PositionalEncoding2D``,
``PositionalEncodingPermute2D``, ``Summer``), which adapter.py imports and this path never executes. The modules run in ``eval()`` in
float32 and in float64 on the same parameters and inputs for the cases of tests/stamp_adapter_restatement.py (CASES).

* Parameters and inputs are regenerated from seeds by the restatement; the fixture stores the seeds, a float64 checksum of each, and the
  float64 outputs.
* Every parameter is random, ``gamma`` included (the reference's ``gamma = 1e-6`` would hide the whole block behind its residual): the
  tool asserts that the median of what a block adds, |block(x) - x|, exceeds 0.1 of the median |block(x)| for every block of every case.
* The tool refuses to write the fixture unless the reference's own float32 run is within the test tolerance
  (|y32 - y64| <= 1e-5 + 1e-4 |y64|, elementwise) of its float64 run on every case, and prints the worst ratio.
* It also stores the reference's ``state_dict`` key list and shapes for the two shipped configurations.
"""
from __future__ import annotations

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

import stamp_adapter_restatement as R
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")
SEED = 8100


def load_reference():
    _install_stubs()
    pe = types.ModuleType("positional_encodings")
    te = types.ModuleType("positional_encodings.torch_encodings")
    for name in ("PositionalEncoding2D", "PositionalEncodingPermute2D", "Summer"):
        setattr(te, name, type(name, (), {}))
    pe.torch_encodings = te
    sys.modules["positional_encodings"], sys.modules["positional_encodings.torch_encodings"] = pe, te
    sys.path.insert(0, REF)
    import opencood.models.stamp_modules.adapter as ad
    return ad


def build(ad, cls, cfg, sd, dtype):
    model = getattr(ad, cls)(cfg)
    if sd:
        model.load_state_dict(sd, strict=True)
    return model.to(dtype).eval()


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    ad = load_reference()
    store, worst = {}, 0.0
    for ci, name in enumerate(R.CASES):
        seed = SEED + 10 * ci
        cls, cfg, sd, x = R.case_data(name, seed)
        with torch.no_grad():
            y32 = build(ad, cls, cfg, sd, torch.float32)(x)
            y64 = build(ad, cls, cfg, sd, torch.float64)(x.double())
        ok, ratio = R.within(y32, y64)
        worst = max(worst, ratio)
        trace = []
        r64 = R.adapter_forward(cfg, sd, R.prefix_of(cls), x, torch.float64, trace)
        assert tuple(r64.shape) == tuple(y64.shape), (r64.shape, y64.shape)
        assert float((r64 - y64).abs().max()) <= 1e-12 * max(1.0, float(y64.abs().max())), f"{name}: the restatement is not the reference"
        shares = [R.branch_share(a, b) for a, b in trace]
        print(f"case {name}: {cls} {cfg['core_method']} x {list(x.shape)} -> {list(y64.shape)} seed {seed}; max |y| {float(y64.abs().max()):.2f}; "
              f"reference float32 against float64: worst |d| / (1e-5 + 1e-4 |y|) = {ratio:.3f} (max |d| {float((y32.double() - y64).abs().max()):.2e}); "
              f"branch shares {[round(s, 3) for s in shares]}")
        if not ok:
            raise SystemExit(f"{name}: the reference's own float32 run is outside the test tolerance of its float64 run (ratio {ratio:.3f}); "
                             "nothing written")
        assert all(s > R.MIN_BRANCH_SHARE for s in shares), f"{name}: a block adds less than {R.MIN_BRANCH_SHARE} of its output: {shares}"
        if cfg["core_method"] == "identity":
            assert torch.equal(y32, x) and torch.equal(y64, x.double()), "the reference's identity adapter is not the identity at ratio 1"
        p = f"{name}/"
        store.update({p + "seed": np.int64(seed), p + "out64": y64.numpy(), p + "ref32_ratio": np.float64(ratio),
                      p + "branch_shares": np.array(shares, dtype=np.float64),
                      p + "checksum_params": np.float64(R.checksum(sd.values())), p + "checksum_x": np.float64(R.checksum([x]))})
    for key, cfg in R.SHIPPED.items():
        for cls in ("Adapter", "Reverter"):
            ref = getattr(ad, cls)(cfg)
            store[f"keys/{key}/{cls}"] = np.array([f"{k} {list(v.shape)}" for k, v in ref.state_dict().items()])
            assert len(ref.state_dict()) == 33
    print(f"worst float32 / float64 ratio of the reference over the cases: {worst:.3f} (must stay below 1)")
    path = os.path.join(OUT, "stamp_adapter.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < 1000000, os.path.getsize(path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
