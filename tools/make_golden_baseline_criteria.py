#!/usr/bin/env python3
"""Golden fixture of the HEAL and MPDA training criteria, from the reference's own modules (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_baseline_criteria.py      # writes tests/golden/baseline_criteria.npz

Imports the reference's ``PointPillarPyramidLoss`` (opencood/loss/point_pillar_pyramid_loss.py) and ``PointPillarMPDALoss``
(opencood/loss/point_pillar_mpda_loss.py) with the import stubs of oracle/make_golden.py and runs every case of
tests/baseline_criteria_restatement.py (``all_cases``) twice: in float64 (the truth) and in float32 (the yardstick: the tests' error
bar is twice the float32 run's own error).

Stored per case ``<c>``: ``<c>/in/<name>`` every input, ``<c>/args`` and ``<c>/extra`` (json), ``<c>/loss64`` and ``<c>/loss32``,
``<c>/dict64/<key>`` and ``<c>/dict32/<key>`` every ``loss_dict`` entry, ``<c>/grad64/<name>`` the autograd gradient of every logit map
and ``<c>/e32/<name>`` the rms-relative error of its float32 twin; for the occupancy cases also ``<c>/level64/<i>`` and
``<c>/level32/<i>``, the term of level i alone (the criterion built with that one level).
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

import baseline_criteria_restatement as R
import make_golden as MG


def load_criteria():
    import build_ref
    MG._install_stubs()
    sys.path.insert(0, MG.REF)
    assert build_ref.build(), "oracle/_ref/box_overlaps could not be built"   # the loss modules import the post-processor (unused by them)
    import opencood.utils as ou
    sys.modules["opencood.utils.box_overlaps"] = ou.box_overlaps = build_ref.load_box_overlaps()
    from opencood.loss.point_pillar_mpda_loss import PointPillarMPDALoss
    from opencood.loss.point_pillar_pyramid_loss import PointPillarPyramidLoss
    return PointPillarPyramidLoss, PointPillarMPDALoss


def run_reference(Pyr, Mpda, kind, args, inp, extra, dtype):
    """(total, loss_dict, {name: gradient}) of the reference's criterion on a case in `dtype`."""
    t = R.tensors(inp, dtype)
    out, tgt = R.dicts(kind, t, extra.get("record_len"))
    if kind == "mpda":
        crit = Mpda(json.loads(json.dumps(args)))
        total = crit(out, tgt, validate=extra["validate"])
    else:
        crit = Pyr(json.loads(json.dumps(args)))
        total = crit(out, tgt, "_single" if kind == "occ" else "")
    total.backward()
    grads = {k: v.grad.numpy() for k, v in t.items() if v.requires_grad and v.grad is not None}
    return float(total.item()), {k: float(v) for k, v in crit.loss_dict.items()}, grads


def main():
    if not os.path.isdir(MG.REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    torch.set_num_threads(1)   # one summation order: the file regenerates bit for bit
    Pyr, Mpda = load_criteria()
    rec = {}
    for name, (kind, args, inp, extra) in R.all_cases().items():
        rec[f"{name}/args"], rec[f"{name}/extra"], rec[f"{name}/kind"] = json.dumps(args), json.dumps(extra), kind
        for k, v in inp.items():
            rec[f"{name}/in/{k}"] = v
        l64, d64, g64 = run_reference(Pyr, Mpda, kind, args, inp, extra, torch.float64)
        l32, d32, g32 = run_reference(Pyr, Mpda, kind, args, inp, extra, torch.float32)
        assert sorted(d64) == sorted(d32) and sorted(g64) == sorted(g32)
        rec[f"{name}/loss64"], rec[f"{name}/loss32"] = np.float64(l64), np.float64(l32)
        for k in d64:
            rec[f"{name}/dict64/{k}"], rec[f"{name}/dict32/{k}"] = np.float64(d64[k]), np.float64(d32[k])
        for k in g64:
            rec[f"{name}/grad64/{k}"], rec[f"{name}/e32/{k}"] = g64[k], np.float64(R.rms_rel(g32[k], g64[k]))
        if kind == "occ":
            p = args["pyramid"]
            for i, (kk, w) in enumerate(zip(p["relative_downsample"], p["weight"])):
                one = dict(args, pyramid={"relative_downsample": [kk], "weight": [w]})
                sub = {k: v for k, v in inp.items() if not k.startswith("occ") or k == f"occ{i}"}
                sub["occ0"] = sub.pop(f"occ{i}")
                rec[f"{name}/level64/{i}"] = np.float64(run_reference(Pyr, Mpda, kind, one, sub, extra, torch.float64)[0])
                rec[f"{name}/level32/{i}"] = np.float64(run_reference(Pyr, Mpda, kind, one, sub, extra, torch.float32)[0])
        errs = ", ".join("%s %.1e" % (k, rec[f"{name}/e32/{k}"]) for k in g64)
        print(f"{name}: loss {l64:.9f} (float32 {l32:.9f}, rel {R.rel(l32, l64):.2e}), dict {sorted(d64)}, gradient errors {errs}")
    path = R.GOLDEN
    np.savez_compressed(path, **rec)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
