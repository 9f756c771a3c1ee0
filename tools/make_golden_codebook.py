#!/usr/bin/env python3
"""Golden fixture for the CodeFilling codebook codec, from the reference's own UMGMQuantizer (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_codebook.py   # writes tests/golden/codebook.npz

``UMGMQuantizer`` (opencood/models/sub_modules/codebook.py:280) is imported with the import stubs of oracle/make_golden.py and run in
float32 and in float64 on the same parameters, inputs and uniforms for the cases of tests/codebook_restatement.py (CASES).

* The uniforms ``gumbelSoftmax`` draws are data: the tool replaces ``torch.rand_like`` for the duration of a forward by a function that
  hands out recorded float32 draws (already inside float32's [eps, 1 - eps], so the reference's clamp leaves them alone in either
  precision), and wraps ``gumbelSoftmax`` to record the index each sample selects.
* The reference's own ``encode`` / ``decode`` cannot run: ``_multiCodebookDeQuantization.decode`` reads ``self._ix``, and the line that
  registers it is commented out (codebook.py:190). The tool sets ``_ix = arange(m)`` -- the value that line shows -- on every dequantizer
  of the instance at run time. With that attribute the method returns ``[n, m, d]`` where both of its callers (the residual ``z - ...``,
  codebook.py:239, and ``_dequantizationHead(...)``, codebook.py:264) need ``[n, c]``, as the comment above its return says; the tool
  wraps the instance's method with the ``reshape(n, -1)`` that ``forward`` applies to the same lookup (codebook.py:207).
* Parameters, inputs and uniforms are regenerated from seeds by the restatement (they do not fit the committed-file limit at the shipped
  shape); the fixture stores the seeds and a float64 checksum of each.

Near ties. ``logit_err32`` of a case = max over its decisions of |logit32 - logit64| / (the group's largest |logit64 + gumbel|), over the
rows on which the reference's two precisions took the same decisions. A decision is clear when its float64 top-2 gap is at least
16 x logit_err32 x that largest magnitude -- for both decisions, the sampled index and the returned code. Strict cases: the tool searches
for a seed under which every row is clear. Bulk case: unclear rows are excluded as a whole; the tool prints the excluded share and the
share of rows on which the reference's own float32 run flips a decision, and refuses a scaling that excludes 1 % or more.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import codebook_restatement as R
from make_golden import REF, _install_stubs

OUT = os.path.join(REPO, "tests", "golden")
SEED = 7300
MAX_SEED_TRIES = 400


def load_reference():
    _install_stubs()
    sys.path.insert(0, REF)
    import opencood.models.sub_modules.codebook as cb
    return cb


class Recorder:
    """Feeds recorded uniforms to torch.rand_like and records what gumbelSoftmax selects."""

    def __init__(self, cb):
        self.cb, self.orig_gs, self.orig_rand = cb, cb.gumbelSoftmax, torch.rand_like

    def run(self, model, x, uniforms):
        self.sampled, level = [], [0]

        def rand_like(t, **kw):
            u = uniforms[level[0]].to(t.dtype)
            assert u.shape == t.shape
            level[0] += 1
            return u.clone()

        def gumbel_softmax(logits, temperature=1.0, hard=True, dim=-1):
            out = self.orig_gs(logits, temperature, hard, dim)
            self.sampled.append(out.argmax(dim))
            return out

        torch.rand_like, self.cb.gumbelSoftmax = rand_like, gumbel_softmax
        try:
            with torch.no_grad():
                restored, codes, logits, loss = model(x)
        finally:
            torch.rand_like, self.cb.gumbelSoftmax = self.orig_rand, self.orig_gs
        assert level[0] == len(uniforms)
        return dict(restored=restored, codes=codes, logits=logits, loss=loss, sampled=self.sampled)


def build(cb, c, sd, dtype):
    model = cb.UMGMQuantizer(c["C"], c["m"], list(c["k"]), 0.0, R.components(c["C"]))
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype).eval()
    for mod in model.modules():                       # the reference's commented-out buffer (see the module docstring)
        if isinstance(mod, cb._multiCodebookDeQuantization):
            mod._ix = torch.arange(mod._m)
            mod.decode = (lambda code, _f=type(mod).decode, _s=mod: _f(_s, code).reshape(code.shape[0], -1))
    return model


def run_case(cb, rec, name, seed):
    c, sd, x, u = R.case_data(name, seed)
    m32, m64 = build(cb, c, sd, torch.float32), build(cb, c, sd, torch.float64)
    o32, o64 = rec.run(m32, x, u), rec.run(m64, x.double(), u)
    r64 = R.umgm_forward(sd, x, c["m"], c["k"], u, torch.float64)
    agree = torch.ones(c["n"], dtype=torch.bool)
    for l in range(len(c["k"])):
        agree &= ((o32["sampled"][l] == o64["sampled"][l]) & (o32["codes"][l] == o64["codes"][l])).all(-1)
    rel = 0.0
    for l in range(len(c["k"])):
        scale = r64["y"][l].abs().amax(-1, keepdim=True)
        rel = max(rel, float(((o32["logits"][l].double() - o64["logits"][l]).abs() / scale)[agree].max()))
    clear = R.clear_rows(o64["logits"], r64["y"], rel)
    return dict(c=c, sd=sd, x=x, u=u, o32=o32, o64=o64, r64=r64, m32=m32, m64=m64, agree=agree, rel=rel, clear=clear)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    cb = load_reference()
    rec = Recorder(cb)
    store = {}
    for ci, name in enumerate(R.CASES):
        strict = name != "bulk"
        base = SEED + 1000 * ci
        for t in range(MAX_SEED_TRIES if strict else 1):
            r = run_case(cb, rec, name, base + 3 * t)
            if not strict or (bool(r["clear"].all()) and bool(r["agree"].all())):
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEED_TRIES} makes every decision clear; raise the scalings")
        seed, c, o32, o64, r64 = base + 3 * t, r["c"], r["o32"], r["o64"], r["r64"]
        L = len(c["k"])
        excluded, flipped = 1.0 - float(r["clear"].double().mean()), 1.0 - float(r["agree"].double().mean())
        flips_inside = int((~r["agree"] & r["clear"]).sum())
        print(f"case {name}: C {c['C']} m {c['m']} k {c['k']} n {c['n']} seed {seed} (try {t}); logit range "
              f"{min(float(l.min()) for l in o64['logits']):.1f} .. 0; logit_err32 {r['rel']:.3e}; excluded (unclear) share {excluded:.4%}; "
              f"rows the reference's own float32 run flips {flipped:.4%} ({flips_inside} of them among the clear rows)")
        assert flips_inside == 0, "the reference's float32 run flips a decision the margin calls clear: the margin is too small"
        if not strict:
            assert excluded < 0.01, "the scaling leaves 1 % or more of the rows unclear"
        # the restatement is the reference, in float64
        for key in ("restored", "loss"):
            assert float((r64[key] - o64[key]).abs().max()) < 1e-12 * max(1.0, float(o64[key].abs().max())), key
        for l in range(L):
            assert torch.equal(r64["codes"][l], o64["codes"][l]) and torch.equal(r64["sampled"][l], o64["sampled"][l])
            assert float((r64["logits"][l] - o64["logits"][l]).abs().max()) < 1e-10
        # encode / decode of the reference (noise-free), both precisions
        with torch.no_grad():
            enc32, enc64 = r["m32"].encode(r["x"]), r["m64"].encode(r["x"].double())
            dec64 = r["m64"].decode(enc64)
        keep = slice(None) if strict else slice(0, c["n"], c["n"] // R.BULK_KEPT_ROWS)
        p = f"{name}/"
        store.update({
            p + "seed": np.int64(seed), p + "logit_err32": np.float64(r["rel"]), p + "excluded_share": np.float64(excluded),
            p + "ref32_flipped_share": np.float64(flipped), p + "clear": r["clear"].numpy(),
            p + "checksum_params": np.float64(R.checksum(r["sd"].values())), p + "checksum_x": np.float64(R.checksum([r["x"]])),
            p + "checksum_uniforms": np.float64(R.checksum(r["u"])),
            p + "restored64": o64["restored"][keep].numpy(), p + "restored32": o32["restored"][keep].numpy(),
            p + "loss64": np.float64(float(o64["loss"])), p + "loss32": np.float32(float(o32["loss"])),
            p + "decode64": dec64[keep].numpy(),
        })
        for l in range(L):
            store.update({
                f"{p}codes64_{l}": o64["codes"][l].numpy().astype(np.uint8), f"{p}codes32_{l}": o32["codes"][l].numpy().astype(np.uint8),
                f"{p}sampled64_{l}": o64["sampled"][l].numpy().astype(np.uint8), f"{p}sampled32_{l}": o32["sampled"][l].numpy().astype(np.uint8),
                f"{p}encode64_{l}": enc64[l].numpy().astype(np.uint8), f"{p}encode32_{l}": enc32[l].numpy().astype(np.uint8),
                f"{p}logits64_{l}": o64["logits"][l][keep].numpy(), f"{p}logits32_{l}": o32["logits"][l][keep].numpy(),
            })
        if strict:
            ref = cb.UMGMQuantizer(c["C"], c["m"], list(c["k"]), 0.0, R.components(c["C"]))
            store[p + "keys"] = np.array([f"{k} {list(v.shape)}" for k, v in ref.state_dict().items()])
    path = os.path.join(OUT, "codebook.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
