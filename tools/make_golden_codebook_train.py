#!/usr/bin/env python3
"""Golden fixture for TRAINING the CodeFilling codebook codec: gradients of the reference's own UMGMQuantizer (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_codebook_train.py   # writes tests/golden/codebook_train.npz

Same mechanics as tools/make_golden_codebook.py: ``torch.rand_like`` is replaced by recorded uniforms for the duration of a forward,
``gumbelSoftmax`` is wrapped to record the index each sample selects, and the reference's module runs in float32 and in float64 on the
same parameters, inputs and uniforms -- here with autograd on. The objective is ``sum(restored * G) + 3 * code_loss``; gradients are
taken with respect to x and every parameter (a level's tied codebook is one parameter and receives one summed gradient).

Parameters, inputs, uniforms and G are regenerated from stored seeds by tests/codebook_train_restatement.py; the fixture stores a
float64 checksum of each. Per gradient tensor it stores a strided subsample (<= 256 elements) of the reference's float64 values, the
float64 sum and sum of squares of the whole tensor, and the relative rms error of the reference's OWN float32 gradient against its
float64 one: the yardstick of the GPU tests.

Strict cases: every row's decisions are clear by codebook_restatement.clear_rows with the case's own measured logit_err32, and the
seed is the first under which that holds -- no row may be excluded from a gradient case, a weight gradient sums over all rows. Soft
case (default initialisation): the fixture stores the reference's float64 sampled indices; the tests force them.
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

import codebook_restatement as R
import codebook_train_restatement as T
from make_golden import REF
from make_golden_codebook import build, load_reference

OUT = os.path.join(REPO, "tests", "golden")
SEED = 9100
MAX_SEED_TRIES = 60


class GradRecorder:
    """make_golden_codebook.Recorder with autograd on."""

    def __init__(self, cb):
        self.cb, self.orig_gs, self.orig_rand = cb, cb.gumbelSoftmax, torch.rand_like

    def run(self, model, x, uniforms, G):
        self.sampled, level = [], [0]

        def rand_like(t, **kw):
            u = uniforms[level[0]].to(t.dtype)
            assert u.shape == t.shape
            level[0] += 1
            return u.clone()

        def gumbel_softmax(logits, temperature=1.0, hard=True, dim=-1):
            out = self.orig_gs(logits, temperature, hard, dim)
            self.sampled.append(out.detach().argmax(dim))
            return out

        x = x.detach().clone().requires_grad_(True)
        model.zero_grad(set_to_none=True)
        torch.rand_like, self.cb.gumbelSoftmax = rand_like, gumbel_softmax
        try:
            restored, codes, logits, loss = model(x)
        finally:
            torch.rand_like, self.cb.gumbelSoftmax = self.orig_rand, self.orig_gs
        assert level[0] == len(uniforms)
        ((restored * G.to(restored.dtype)).sum() + T.LOSS_WEIGHT * loss).backward()
        grads = {"x": x.grad.detach()}
        for key, p in model.named_parameters():          # named_parameters lists a tied parameter once, under its first name
            grads[key] = torch.zeros_like(p) if p.grad is None else p.grad.detach()
        return dict(restored=restored.detach(), codes=codes, logits=[l.detach() for l in logits], loss=loss.detach(), sampled=self.sampled,
                    grads=grads)


def run_case(cb, rec, name, seed):
    c, sd, x, u, G = T.case_data(name, seed)
    m32, m64 = build(cb, c, sd, torch.float32).train(), build(cb, c, sd, torch.float64).train()
    o32, o64 = rec.run(m32, x, u, G), rec.run(m64, x.double(), u, G)
    r64 = R.umgm_forward(sd, x, c["m"], c["k"], u, torch.float64)
    agree = torch.ones(c["n"], dtype=torch.bool)
    for l in range(len(c["k"])):
        agree &= ((o32["sampled"][l] == o64["sampled"][l]) & (o32["codes"][l] == o64["codes"][l])).all(-1)
    rel = 0.0
    for l in range(len(c["k"])):
        scale = r64["y"][l].abs().amax(-1, keepdim=True)
        e = ((o32["logits"][l].double() - o64["logits"][l]).abs() / scale)[agree]
        rel = max(rel, float(e.max()) if e.numel() else 0.0)
    clear = R.clear_rows(o64["logits"], r64["y"], rel)
    return dict(c=c, sd=sd, x=x, u=u, G=G, o32=o32, o64=o64, agree=agree, rel=rel, clear=clear)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    cb = load_reference()
    rec = GradRecorder(cb)
    store = {}
    for ci, name in enumerate(T.CASES):
        strict = name in T.STRICT
        base = SEED + 1000 * ci
        for t in range(MAX_SEED_TRIES if strict else 1):
            r = run_case(cb, rec, name, base + 4 * t)
            if not strict or (bool(r["clear"].all()) and bool(r["agree"].all())):
                break
        else:
            raise SystemExit(f"{name}: no seed in {MAX_SEED_TRIES} makes every decision clear")
        seed, c, o32, o64 = base + 4 * t, r["c"], r["o32"], r["o64"]
        keys = T.param_keys(r["sd"])
        assert sorted(keys + ["x"]) == sorted(o64["grads"]), (sorted(keys), sorted(o64["grads"]))
        # the restatement is the reference, in float64 (with the reference's indices forced on the soft case)
        g64, _ = T.gradients(r["sd"], r["x"], c["m"], c["k"], r["u"], None if strict else o64["sampled"], r["G"], T.LOSS_WEIGHT, torch.float64)
        p = f"{name}/"
        store.update({
            p + "seed": np.int64(seed), p + "logit_err32": np.float64(r["rel"]),
            p + "checksum_params": np.float64(R.checksum(r["sd"].values())), p + "checksum_x": np.float64(R.checksum([r["x"]])),
            p + "checksum_uniforms": np.float64(R.checksum(r["u"])), p + "checksum_G": np.float64(R.checksum([r["G"]])),
            p + "loss64": np.float64(float(o64["loss"])),
            p + "keys": np.array(sorted(o64["grads"])),
        })
        for l in range(len(c["k"])):
            store[f"{p}sampled64_{l}"] = o64["sampled"][l].numpy().astype(np.uint8)
        worst = ("", 0.0, 0.0)
        for key in sorted(o64["grads"]):
            a64, a32 = o64["grads"][key], o32["grads"][key]
            dev = float((g64[key] - a64).abs().max()) / max(float(a64.abs().max()), 1e-300)
            assert dev < 1e-10, (name, key, dev)
            yard = T.rel_rms(a32, a64) if bool(r["agree"].all()) else float("nan")
            of_max = float((a32.double() - a64).abs().max() / a64.abs().max())
            if of_max > worst[1]:
                worst = (key, of_max, yard)
            store.update({
                f"{p}grad64/{key}": T.subsample(a64).numpy(), f"{p}sum64/{key}": np.float64(float(a64.sum())),
                f"{p}sumsq64/{key}": np.float64(float((a64 ** 2).sum())), f"{p}yard32/{key}": np.float64(yard),
            })
        print(f"case {name}: C {c['C']} m {c['m']} k {c['k']} n {c['n']} seed {seed} (try {t}); logit_err32 {r['rel']:.3e}; clear rows "
              f"{float(r['clear'].double().mean()):.2%}; float32 run agrees on {float(r['agree'].double().mean()):.2%} of rows; worst float32 gradient "
              f"{worst[0]}: {worst[1]:.2e} of its maximum (rel rms {worst[2]:.2e})")
    path = os.path.join(OUT, "codebook_train.npz")
    np.savez_compressed(path, **store)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
