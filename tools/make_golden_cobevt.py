#!/usr/bin/env python3
"""Golden fixture of the CoBEVT fusion net, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_cobevt.py      # writes tests/golden/cobevt.npz, cobevt_f64.npz and cobevt_keys.json

The reference's ``CoBEVT`` (opencood/models/fuse_modules/fusion_in_one.py:409-464, blocks in fuse_modules/swap_fusion_modules.py) is
imported with the import stubs of oracle/make_golden.py (``icecream``, ``shapely``, ``timm.models.layers``) and runs in ``eval()``.

Weights are not stored: ``gencomm_amd.synth.fill_params_(module, seed)`` fills the reference module here and the package's module in
the tests (same parameter names, so the same draws). Stored per case of tests/cobevt_restatement.py's table: the inputs (post-ReLU
normals on a 1/16 grid, so float16 holds them exactly), ``record_len``, ``affine_matrix`` [B, L, L, 2, 3] float64 (rotations of a few
tenths of a radian plus translations; the last agent of a scene is warped partly out of the map), and the reference's output twice:
``y32`` from a float32 run and the float64 run of the same module on the same values. Doubles do not compress and the five float64
outputs alone exceed what one committed file may hold, so the float64 output is stored as ``d64 = float32(y64 - y32)``: the tests use
y64 = y32 - d64 in float64, which is the float64 output to within float32 rounding of a difference of about 1e-6 (below 1e-12).
Even so the whole is larger than one committed file may be: ``d64`` goes to a file of its own, ``cobevt_f64.npz``.
``cobevt_keys.json`` is the ordered ``state_dict`` key and shape list at the shipped block (depth 3, 76 entries).
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

from gencomm_amd import synth
from cobevt_restatement import CASES, case_args, make_inputs
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")
SEED = 4100


def load_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    from opencood.models.fuse_modules.fusion_in_one import CoBEVT
    return CoBEVT


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    CoBEVT = load_reference()
    rec, rec64 = {"weight_seed": np.int64(SEED)}, {}
    for n_tag, (tag, c) in enumerate(CASES.items()):
        args = case_args(c)
        torch.manual_seed(0)
        model = CoBEVT(dict(args)).eval()
        synth.fill_params_(model, SEED + n_tag)
        x, aff = make_inputs(c, SEED + 100 + 10 * n_tag)
        x = np.clip(np.round(16 * x) / 16, 0.0, 8.0).astype(np.float32)
        assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
        rl = torch.tensor(c["record_len"])
        with torch.no_grad():
            y32 = model(torch.from_numpy(x), rl, torch.from_numpy(aff))
            y64 = model.double()(torch.from_numpy(x).double(), rl, torch.from_numpy(aff))
        assert y32.dtype == torch.float32 and y64.dtype == torch.float64
        assert list(y32.shape) == [len(c["record_len"]), c["C"], c["H"], c["W"]]
        assert torch.isfinite(y32).all() and torch.isfinite(y64).all()
        y32, y64 = y32.numpy(), y64.numpy()
        d64 = (y32.astype(np.float64) - y64).astype(np.float32)
        assert np.abs((y32.astype(np.float64) - d64.astype(np.float64)) - y64).max() < 1e-12
        rms = float(np.sqrt(np.mean((y32 - y64) ** 2) / np.mean(y64 ** 2)))
        print(f"case {tag}: {args} record_len {c['record_len']} out {y32.shape} |y| max {np.abs(y64).max():.3f}, float32 vs float64: "
              f"max abs {np.abs(y32 - y64).max():.2e}, rms-relative {rms:.2e}")
        rec.update({f"args_{tag}": json.dumps(args), f"x_{tag}": x.astype(np.float16), f"record_len_{tag}": np.asarray(c["record_len"], np.int64),
                    f"affine_{tag}": aff, f"y32_{tag}": y32, f"seed_{tag}": np.int64(SEED + n_tag)})
        rec64[f"d64_{tag}"] = d64
    for name, r in (("cobevt.npz", rec), ("cobevt_f64.npz", rec64)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **r)
        assert os.path.getsize(path) < (1 << 20), "larger than a committed file may be"
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    shipped = CoBEVT({"input_dim": 256, "mlp_dim": 256, "agent_size": 5, "window_size": 4, "dim_head": 32, "drop_out": 0.1, "depth": 3})
    keys = [[k, list(v.shape)] for k, v in shipped.state_dict().items()]
    assert len(keys) == 76
    with open(os.path.join(OUT, "cobevt_keys.json"), "w") as f:
        json.dump({"args": {"input_dim": 256, "mlp_dim": 256, "agent_size": 5, "window_size": 4, "dim_head": 32, "drop_out": 0.1, "depth": 3},
                   "state_dict": keys}, f, indent=0)
    print(f"wrote cobevt_keys.json ({len(keys)} entries)")


if __name__ == "__main__":
    main()
