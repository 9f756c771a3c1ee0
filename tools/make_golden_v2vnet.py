#!/usr/bin/env python3
"""Golden fixtures for the V2VNet fusion, from the reference's own module (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_v2vnet.py   # writes tests/golden/v2vnet.npz and tests/golden/v2vnet_keys.json

``V2VNetFusion`` (opencood/models/fuse_modules/fusion_in_one.py:238-353, with sub_modules/convgru.py) is imported with the import stubs
of oracle/make_golden.py and run in float32 and in float64 on the same values, for the four configurations of
tests/v2vnet_restatement.py (CASES; all with record_len [2, 3, 1, 4], L = 5). The poses fill ALL rows of the pairwise matrix
(synth.make_pairwise_t_matrix -> normalize_pairwise_tfm) and agent 3 of the last scene is moved off the map, so its mask is zero
everywhere. Stored per configuration: the input (once per shape), the ``synth.fill_params_`` weights, ``record_len``, the normalised [B, L, L, 2, 3]
matrices, both outputs, and the reference's own float32-against-float64 error (relative rms and max abs): the GPU tests' yardsticks.

Configuration d is sized so that its three convolutions take the three-term matrix-pipe route; the tool checks it with
gencomm_conv2d_prepared_floats where the HIP library is built.
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

import v2vnet_restatement as R
from gencomm_amd import synth
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")
SEED = 6100
SHIPPED = {"in_channels": 256, "num_iteration": 2, "gru_flag": True, "agg_operator": "avg",
           "conv_gru": {"H": 128, "W": 128, "num_layers": 1, "kernel_size": [[3, 3]]}}


def load_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    from opencood.models.fuse_modules.fusion_in_one import V2VNetFusion
    return V2VNetFusion


def check_matrix_pipe_route(c):
    """Configuration d: the three convolutions (C -> C twice, 2C -> 2C) carry the three-term operand form behind the fp32 matrix."""
    from gencomm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        print("HIP library not built: the matrix-pipe route of configuration d was not checked")
        return
    C = c["C"]
    for cin, cout in ((C, C), (2 * C, 2 * C)):
        floats = _lib.check_size(_lib.lib().gencomm_conv2d_prepared_floats(cin, cout, 3, 3, 0), "gencomm_conv2d_prepared_floats")
        assert floats > cin * cout * 9, f"3x3 {cin} -> {cout} does not take the three-term route: raise C"


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixtures can only be regenerated in the build container")
    V2VNetFusion = load_reference()
    rl = R.RECORD_LEN
    n = sum(rl)
    store = {"record_len": np.asarray(rl, np.int64), "seed": np.int64(SEED)}
    for i, (tag, c) in enumerate(R.CASES.items()):
        args = R.case_args(c)
        seed = SEED + 10 * i
        dseed = SEED + 10 * list(R.CASES).index(c["data"])      # configurations of one shape share the input and the poses
        x = R.make_x(n, c["C"], c["H"], c["W"], dseed)
        aff = R.make_affine(rl, R.L, c["H"], c["W"], dseed + 1, off_map=(3, 3))
        torch.manual_seed(0)
        model = V2VNetFusion(args).eval()
        synth.fill_params_(model, seed + 2)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        with torch.no_grad():
            o32 = model(torch.from_numpy(x), torch.tensor(rl), torch.from_numpy(aff)).numpy()
            o64 = model.double()(torch.from_numpy(x).double(), torch.tensor(rl), torch.from_numpy(aff)).numpy()
            r64 = R.v2vnet_forward(sd, args, torch.from_numpy(x).double(), rl, torch.from_numpy(aff)).numpy()
        assert o32.dtype == np.float32 and o64.dtype == np.float64 and list(o32.shape) == [len(rl), c["C"], c["H"], c["W"]]
        mask = R.warp(torch.ones(n, 1, c["H"], c["W"], dtype=torch.float64),
                      torch.cat([torch.from_numpy(aff)[b, 0, :k] for b, k in enumerate(rl)]))
        frac = float(((mask > 0) & (mask < 1 - 1e-9)).double().mean())
        off_mask = R.warp(torch.ones(4, 1, c["H"], c["W"], dtype=torch.float64), torch.from_numpy(aff)[3, :4, 3])
        assert float(off_mask[:3].abs().max()) == 0.0, "the off-map agent must be invisible to the others"
        e_rms, e_max = R.rel_rms(o32, o64), float(np.abs(o32 - o64).max())
        print(f"case {tag}: {args}\n  x {x.shape}, out rms {np.sqrt((o64 ** 2).mean()):.3f}; reference float32 vs float64: rel rms {e_rms:.3e}, max abs "
              f"{e_max:.3e}; decomposed restatement vs reference in float64: max abs {np.abs(r64 - o64).max():.2e}; fractional-mask share of "
              f"the ego rows {frac:.3f}")
        assert R.rel_rms(r64, o64) < 1e-12
        store.update({f"x_{c['data']}": x, f"affine_{c['data']}": aff, f"out32_{tag}": o32, f"out64_{tag}": o64, f"weight_seed_{tag}": np.int64(seed + 2),
                      f"ref_rel_rms_{tag}": np.float64(e_rms), f"ref_max_abs_{tag}": np.float64(e_max)})
        for k, v in sd.items():
            store[f"w_{tag}/{k}"] = v.numpy()
    check_matrix_pipe_route(R.CASES["d"])
    path = os.path.join(OUT, "v2vnet.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < (1 << 20)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    shipped = V2VNetFusion(SHIPPED)
    keys = [[k, list(v.shape)] for k, v in shipped.state_dict().items()]
    with open(os.path.join(OUT, "v2vnet_keys.json"), "w") as f:
        json.dump({"args": SHIPPED, "state_dict": keys}, f, indent=0)
    print(f"wrote v2vnet_keys.json ({len(keys)} entries)")


if __name__ == "__main__":
    main()
