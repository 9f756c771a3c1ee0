#!/usr/bin/env python3
"""Golden gradients of the CoBEVT fusion net, from the reference's own code and its own autograd (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_cobevt_train.py      # writes tests/golden/cobevt_train.npz and cobevt_train_<k>.npz

As tools/make_golden_cobevt.py: the reference's ``CoBEVT`` (opencood/models/fuse_modules/fusion_in_one.py:409-464) is imported with the
import stubs of oracle/make_golden.py and runs in ``eval()`` (its dropouts are the identity), weights from
``gencomm_amd.synth.fill_params_(module, seed)`` with that tool's seeds, inputs rebuilt exactly as that tool builds them (so
tests/golden/cobevt.npz holds the same ``x``, ``record_len`` and ``affine_matrix``; they are not stored again), cases from the ``CASES``
table of tests/cobevt_restatement.py. The loss is ``(y * g).sum()`` with a stored ``g`` (normals on a 1/16 grid: float16 holds them).

Stored, per case:
  a, b, c, e   the float64 run's ``dx`` and every parameter gradient (``param_names``: the state_dict order without the index buffers),
               each as a float32 pair ``hi = float32(v)``, ``lo = float32(v - hi)``: ``hi + lo`` in float64 is the float64 gradient
               to a relative 2^-48, and doubles do not compress;
               ``yard_<case>``: per gradient (dx first, then the parameters in order) the relative rms ``||g32 - g64|| / ||g64||`` of
               the reference's float32 run against its float64 run -- the yardstick of the GPU tests.
  d            (C 256, depth 3: the full parameter gradients do not fit) ``dx`` as above, and per parameter the float64 norm
               (``norm_d``) and the dot product (``dot_d``) with ``synth.noise_stream(DOT_SEED, i, shape)``; ``yard_d`` holds dx's
               yardstick and, per parameter, the same relative rms.
One committed file may hold 1 MiB, and these gradients need several: the arrays are packed greedily, in a fixed order, into
``cobevt_train.npz`` (which also holds the small entries and the list of the other files) and ``cobevt_train_1.npz``, ``_2`` ...;
``load_golden`` in tests/test_cobevt_train.py reads them back as one dictionary.

Prints, per case, the smallest gradient rms over the parameters, and asserts that no stored parameter gradient is identically zero
(none is expected to be: every parameter reaches the output in ``eval()`` mode).
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
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np
import torch

from gencomm_amd import synth
from cobevt_restatement import CASES, case_args, make_inputs
from make_golden import REF
from make_golden_cobevt import SEED, load_reference

OUT = os.path.join(REPO, "tests", "golden")
G_SEED, DOT_SEED = 4177, 4178
LIMIT = 1000 * 1024           # per file, below the 1 MiB a committed file may hold
FULL = ("a", "b", "c", "e")


def loss_weights(n_tag, shape):
    """g of the loss (y * g).sum(): normals rounded to a 1/16 grid."""
    g = np.clip(np.round(16 * synth.noise_stream(G_SEED, n_tag, shape)) / 16, -8.0, 8.0).astype(np.float32)
    assert np.array_equal(g.astype(np.float16).astype(np.float32), g)
    return g


def dot_vector(i, shape):
    return synth.noise_stream(DOT_SEED, i, shape).astype(np.float64)


def pair(v64):
    hi = v64.astype(np.float32)
    lo = (v64 - hi.astype(np.float64)).astype(np.float32)
    back = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.linalg.norm(back - v64) <= 1e-13 * np.linalg.norm(v64)
    return hi, lo


def run(model, x, rl, aff, g, dtype):
    model = model.to(dtype)
    for p in model.parameters():
        p.grad = None
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = model(xt, rl, torch.from_numpy(aff))
    assert y.dtype == dtype
    (y * torch.from_numpy(g).to(dtype)).sum().backward()
    names = [k for k, v in model.state_dict().items() if v.is_floating_point()]
    params = dict(model.named_parameters())
    assert sorted(names) == sorted(params), "a floating state_dict entry that is no parameter"
    return xt.grad.double().numpy(), [(k, params[k].grad.double().numpy()) for k in names]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    CoBEVT = load_reference()
    small, big = {"weight_seed": np.int64(SEED)}, []
    for n_tag, (tag, c) in enumerate(CASES.items()):
        args = case_args(c)
        torch.manual_seed(0)
        model = CoBEVT(dict(args)).eval()
        synth.fill_params_(model, SEED + n_tag)
        x, aff = make_inputs(c, SEED + 100 + 10 * n_tag)
        x = np.clip(np.round(16 * x) / 16, 0.0, 8.0).astype(np.float32)
        rl = torch.tensor(c["record_len"])
        g = loss_weights(n_tag, (len(c["record_len"]), c["C"], c["H"], c["W"]))
        dx32, p32 = run(model, x, rl, aff, g, torch.float32)
        dx64, p64 = run(model, x, rl, aff, g, torch.float64)
        yard = [rel(dx32, dx64)] + [rel(a[1], b[1]) for a, b in zip(p32, p64)]
        rms = {k: float(np.sqrt(np.mean(v ** 2))) for k, v in p64}
        for k, v in p64:
            assert np.any(v != 0), f"case {tag}: the gradient of {k} is identically zero"
        kmin = min(rms, key=rms.get)
        print(f"case {tag}: {len(p64)} parameter gradients, smallest rms {rms[kmin]:.3e} ({kmin}); dx rms {np.sqrt(np.mean(dx64 ** 2)):.3e}; "
              f"float32 vs float64: dx {yard[0]:.2e}, parameters {min(yard[1:]):.2e} .. {max(yard[1:]):.2e}")
        small[f"g_{tag}"] = g.astype(np.float16)
        small[f"yard_{tag}"] = np.asarray(yard, np.float64)
        small[f"names_{tag}"] = json.dumps([k for k, _ in p64])
        hi, lo = pair(dx64)
        big += [(f"dx_hi_{tag}", hi), (f"dx_lo_{tag}", lo)]
        if tag in FULL:
            for i, (k, v) in enumerate(p64):
                hi, lo = pair(v)
                big += [(f"p{i}_hi_{tag}", hi), (f"p{i}_lo_{tag}", lo)]
        else:
            small[f"norm_{tag}"] = np.asarray([np.linalg.norm(v) for _, v in p64], np.float64)
            small[f"dot_{tag}"] = np.asarray([float((v * dot_vector(i, v.shape)).sum()) for i, (_, v) in enumerate(p64)], np.float64)
    # greedy packing in a fixed order; an array larger than a file is cut along its flattened length
    pieces = []
    for name, v in big:
        flat, nmax = v.reshape(-1), LIMIT // 4 - 4096
        if flat.size <= nmax:
            pieces.append((name, v))
        else:
            small[f"shape_{name}"] = np.asarray(v.shape, np.int64)
            for j, s in enumerate(range(0, flat.size, nmax)):
                pieces.append((f"{name}.part{j}", flat[s:s + nmax]))
    files, cur, cur_bytes = [], dict(small), 64 * 1024
    for name, v in pieces:
        if cur_bytes + v.nbytes + 512 > LIMIT:
            files.append(cur)
            cur, cur_bytes = {}, 0
        cur[name] = v
        cur_bytes += v.nbytes + 512
    files.append(cur)
    names = ["cobevt_train.npz"] + [f"cobevt_train_{k}.npz" for k in range(1, len(files))]
    files[0]["files"] = json.dumps(names)
    for name, rec in zip(names, files):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < (1 << 20), f"{name} is larger than a committed file may be"
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB, {len(rec)} arrays)")


if __name__ == "__main__":
    main()
