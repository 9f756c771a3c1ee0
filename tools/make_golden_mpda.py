#!/usr/bin/env python3
"""Golden fixture of MPDA's feature aligner, from the reference's own modules (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_mpda.py      # writes tests/golden/mpda.npz and mpda_keys.json

``LearnableResizer``, ``CrossDomainFusionEncoder`` and ``DAImgHead`` are imported from ``opencood.models.mpda_modules`` directly, with
the import stubs of oracle/make_golden.py; the model shell (``heter_model_baseline_w_mpda``) is NOT imported -- it needs torchvision.
The modules need ``einops``. They run in ``eval()`` in float32 and in float64 on the same values.

Weights are not stored: ``gencomm_amd.synth.fill_params_(module, seed)`` and ``fill_bn_stats_(module, seed + 50)`` fill the reference
module here and the package's module in the tests (same parameter names, so the same draws). Inputs are not stored either: both sides
draw them with ``mpda_restatement.case_inputs``. Stored per case of ``mpda_restatement.CASES`` and per output (``resizer``, ``cdt``,
``da``; ``align`` and ``logits`` where the case has a ``record_len``): ``y32`` from the float32 run and ``d64 = float32(y32 - y64)``,
from which the tests rebuild the float64 output (y64 = y32 - d64 in float64, to within 1e-12), and ``e_ref``, the float32 run's
rms-relative error against the float64 run -- the yardstick of the tests' second bar, printed here per case.

The aligner's loop (heter_model_baseline_w_mpda.py:232-262) is restated below around the reference's modules, ego-only branch
included. ``mpda_keys.json`` is the ordered ``state_dict`` key and shape list at the shipped configuration: ``resizer`` and ``cdt``
as in GenComm_yamls/baselines/stage2/MPDA/m1m3_att.yaml, and ``DAImgHead(128)``.
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
import torch.nn as nn

import mpda_restatement as R
from gencomm_amd import synth
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")


def load_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    from opencood.models.mpda_modules.classfier import DAImgHead
    from opencood.models.mpda_modules.resizer import LearnableResizer
    from opencood.models.mpda_modules.wg_fusion_modules import CrossDomainFusionEncoder
    return LearnableResizer, CrossDomainFusionEncoder, DAImgHead


def filled(module, seed):
    module = module.eval()
    synth.fill_params_(module, seed)
    synth.fill_bn_stats_(module, seed + 50)
    return module


class Aligner(nn.Module):
    """The three modules under the shell's attribute names, and lines 232-262 of its forward."""

    def __init__(self, refs, args):
        super().__init__()
        LearnableResizer, CrossDomainFusionEncoder, DAImgHead = refs
        self.resizer = LearnableResizer(args["resizer"])
        self.cdt = CrossDomainFusionEncoder(args["cdt"])
        self.classifier = DAImgHead(args["classifier"]) if "classifier" in args else DAImgHead(128)
        self.rebuttal = args.get("rebuttal", False)

    def forward(self, heter_feature_2d, record_len):
        split = torch.tensor_split(heter_feature_2d, torch.cumsum(torch.tensor(record_len), 0)[:-1])
        class_logits, feats = [], []
        for s in split:
            ego_feature = s[0].unsqueeze(0)
            if s.shape[0] == 1:
                cav_feature = self.resizer(ego_feature, ego_feature)
                cav_feature = self.cdt(ego_feature.clone(), cav_feature)      # computed and discarded, as in the shell
                scene = torch.cat((ego_feature,), dim=0)
            else:
                cav_feature = s[1:]
                if not self.rebuttal:
                    cav_feature = self.resizer(ego_feature, cav_feature)
                    cav_feature = self.cdt(ego_feature.repeat(cav_feature.shape[0], 1, 1, 1), cav_feature)
                scene = torch.cat((ego_feature, cav_feature), dim=0)
            class_logits.append(self.classifier(scene))
            feats.append(scene)
        return torch.cat(feats, dim=0), torch.cat(class_logits, dim=0)


def both(make, seed, run):
    """run(module, dtype) on the float32 module and on its float64 copy -> (tuple of y32, tuple of y64), numpy."""
    torch.manual_seed(0)
    m = filled(make(), seed)
    with torch.no_grad():
        y32 = run(m, torch.float32)
        y64 = run(m.double(), torch.float64)
    tup = lambda y: tuple(t.numpy() for t in (y if isinstance(y, tuple) else (y,)))
    return tup(y32), tup(y64)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    refs = load_reference()
    LearnableResizer, CrossDomainFusionEncoder, DAImgHead = refs
    rec = {"seed": np.int64(R.SEED)}

    def store(tag, name, y32, y64):
        assert y32.dtype == np.float32 and y64.dtype == np.float64 and np.isfinite(y64).all()
        d64 = (y32.astype(np.float64) - y64).astype(np.float32)
        assert np.abs((y32.astype(np.float64) - d64.astype(np.float64)) - y64).max() < 1e-12
        e_ref = R.rel_rms(y32, y64)
        rec[f"{name}_y32_{tag}"], rec[f"{name}_d64_{tag}"], rec[f"{name}_eref_{tag}"] = y32, d64, np.float64(e_ref)
        print(f"case {tag} {name}: out {y32.shape} |y| max {np.abs(y64).max():.3f}; float32 vs float64: max abs {np.abs(y32 - y64).max():.2e}, "
              f"e_ref (rms-relative) {e_ref:.3e}")

    for tag, c in R.CASES.items():
        args = R.case_args(c)
        s_res, s_cdt, s_da, s_al = R.case_seeds(tag)
        ego, cav, cdt_cav, x = (None if a is None else torch.from_numpy(a) for a in R.case_inputs(tag))
        n = cav.shape[0]
        y32, y64 = both(lambda: LearnableResizer(args["resizer"]), s_res, lambda m, dt: m(ego.to(dt), cav.to(dt)))
        assert list(y32[0].shape) == [n, c["C"], c["H"], c["W"]]
        store(tag, "resizer", y32[0], y64[0])
        y32, y64 = both(lambda: CrossDomainFusionEncoder(args["cdt"]), s_cdt, lambda m, dt: m(ego.to(dt).repeat(n, 1, 1, 1), cdt_cav.to(dt)))
        store(tag, "cdt", y32[0], y64[0])
        y32, y64 = both(lambda: DAImgHead(c["C"]), s_da, lambda m, dt: m(cdt_cav.to(dt)))
        assert list(y32[0].shape) == [n, 1, c["H"], c["W"]]
        store(tag, "da", y32[0], y64[0])
        if c["record_len"]:
            y32, y64 = both(lambda: Aligner(refs, args), s_al, lambda m, dt: m(x.to(dt), c["record_len"]))
            store(tag, "align", y32[0], y64[0])
            store(tag, "logits", y32[1], y64[1])
            if c["rebuttal"]:
                assert np.array_equal(y32[0], x.numpy())

    path = os.path.join(OUT, "mpda.npz")
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1024:.0f} KiB)")
    assert size < (1 << 20), "larger than a committed file may be: split d64 into mpda_f64.npz as make_golden_cobevt.py does"

    args = R.shipped_args()
    shipped = Aligner(refs, args)
    keys = {name: [[k, list(v.shape)] for k, v in getattr(shipped, name).state_dict().items()] for name in ("resizer", "cdt", "classifier")}
    with open(os.path.join(OUT, "mpda_keys.json"), "w") as f:
        json.dump({"args": args, "classifier_in_channels": 128, "state_dict": keys}, f, indent=0)
    size = os.path.getsize(os.path.join(OUT, "mpda_keys.json"))
    assert size < (1 << 20)
    print(f"wrote mpda_keys.json ({', '.join(f'{k}: {len(v)} entries' for k, v in keys.items())})")


if __name__ == "__main__":
    main()
