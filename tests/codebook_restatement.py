"""The CodeFilling codebook codec (opencood/models/sub_modules/codebook.py, UMGMQuantizer.forward / encode / decode) restated in plain
torch, in any dtype, from a state_dict with the reference's keys. Used by the CPU tests against tests/golden/codebook.npz (written by
tools/make_golden_codebook.py from the reference's own module), by the GPU tests for the shapes the fixture does not hold, and as the
torch baseline of tools/codebook_bench.py.

The fixture stores generator seeds, not the parameters and inputs themselves (the 16 matrices of the shipped shape alone are 1 MB):
``make_params`` / ``make_x`` / ``make_uniforms`` regenerate them bit for bit from numpy's PCG64 streams, and the fixture carries a
float64 checksum of each to prove it.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

HEADS = ("_latentStageEncoder", "_quantizationHead", "_latentHead")       # encoder side, in the order they are drawn
DEC_HEADS = ("_dequantizationHead", "_sideHead", "_restoreHead")

# The fixture's cases. cb_scale / w_scale spread the logits (default initialisation leaves the deeper levels' logits in a band 0.3
# wide, where 26-44 % of rows have a top-2 gap under 1e-3): codebooks times cb_scale, encoder-side Linear weights times w_scale.
CASES = {
    "strict_a": dict(C=64, m=2, k=[16, 16, 16], n=128, cb_scale=4.0, w_scale=2.0),
    "strict_b": dict(C=64, m=4, k=[32, 16], n=64, cb_scale=4.0, w_scale=2.0),
    "bulk": dict(C=128, m=2, k=[16, 16, 16], n=4096, cb_scale=4.0, w_scale=2.0),
}
BULK_KEPT_ROWS = 64           # rows of the bulk case whose restored rows and logits the fixture holds (every 64th)
CLEAR_FACTOR = 16.0           # a decision is clear when its float64 top-2 gap is at least this many times the reference's own fp32 logit error
MAX_EXCLUDED = 0.02


def components(C):
    import torch.nn as nn
    return {key: (lambda: nn.Linear(C, C)) for key in ("latentStageEncoder", "quantizationHead", "latentHead", "dequantizationHead", "sideHead", "restoreHead")}


def make_params(C, m, ks, seed, cb_scale=1.0, w_scale=1.0):
    """A state_dict with the reference's keys (float32): nn.Linear's default uniform(+-1/sqrt(C)) and the reference's codebook normal,
    then the scalings above."""
    rng = np.random.default_rng(seed)
    sd, bound, L = {}, 1.0 / math.sqrt(C), len(ks)

    def lin(prefix, scale):
        sd[prefix + ".weight"] = torch.from_numpy((rng.uniform(-bound, bound, (C, C)) * scale).astype(np.float32))
        sd[prefix + ".bias"] = torch.from_numpy(rng.uniform(-bound, bound, (C,)).astype(np.float32))

    for i, k in enumerate(ks):
        cb = torch.from_numpy((rng.normal(0.0, math.sqrt(2 / (5 * C / m)), (m, k, C // m)) * cb_scale).astype(np.float32))
        sd[f"_encoders.{i}._quantizer._codebook"] = cb
        sd[f"_encoders.{i}._quantizer._temperature"] = torch.from_numpy(rng.uniform(0.8, 1.25, (m, 1)).astype(np.float32))
        sd[f"_encoders.{i}._quantizer._bound.bound"] = torch.tensor([1e-6], dtype=torch.float32)
        sd[f"_encoders.{i}._dequantizer._codebook"] = cb
        sd[f"_decoders.{i}._dequantizer._codebook"] = cb
        for h in HEADS:
            if h == "_latentHead" and i == L - 1:
                continue
            lin(f"_encoders.{i}.{h}", w_scale)
        for h in DEC_HEADS:
            if h == "_sideHead" and i == L - 1:
                continue
            lin(f"_decoders.{i}.{h}", 1.0)
    return sd


def make_x(n, C, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(0.0, 1.0, (n, C)).astype(np.float32))


def make_uniforms(n, m, ks, seed):
    """float32 draws already inside [eps, 1 - eps] of float32, so that the reference's clamp leaves them alone in either precision."""
    rng, eps = np.random.default_rng(seed), float(np.finfo(np.float32).eps)
    return [torch.from_numpy(np.clip(rng.random((n, m, k), dtype=np.float32), eps, np.float32(1.0 - eps)).astype(np.float32)) for k in ks]


def checksum(tensors):
    return float(sum(t.double().sum() + (t.double() ** 2).sum() for t in tensors))


def _logits(sd, i, h, m, k):
    cb = sd[f"_encoders.{i}._quantizer._codebook"]
    n = h.shape[0]
    hg = h.reshape(n, m, -1)
    x2 = (hg ** 2).sum(2, keepdim=True)
    c2 = (cb ** 2).sum(-1, keepdim=False)
    inter = torch.einsum("nmd,mkd->nmk", hg, cb)
    distance = x2 + c2 - 2 * inter
    temp = torch.max(sd[f"_encoders.{i}._quantizer._temperature"], sd[f"_encoders.{i}._quantizer._bound.bound"])
    return distance, (-1 * distance) / math.sqrt(k) * temp


def _lin(sd, prefix, x):
    return F.linear(x, sd[prefix + ".weight"], sd[prefix + ".bias"])


def gumbels(u, dtype):
    eps = torch.finfo(dtype).eps
    u = u.to(dtype).clamp(eps, 1 - eps)
    return -((-(u.log())).log())


def umgm_forward(sd, x, m, ks, uniforms=None, dtype=None):
    """-> dict(restored, codes, logits, loss, sampled, y): the reference's forward; uniforms None = no noise (the sampled index is the
    code). `y` = logit + gumbel per level (what the sampled index is the argmax of)."""
    dtype = dtype or x.dtype
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    x_gt, L = x, len(ks)
    qs, codes, logits, sampled, ys = [], [], [], [], []
    for i, k in enumerate(ks):
        z = _lin(sd, f"_encoders.{i}._latentStageEncoder", x)
        _, logit = _logits(sd, i, _lin(sd, f"_encoders.{i}._quantizationHead", z), m, k)
        cb = sd[f"_encoders.{i}._quantizer._codebook"]
        if uniforms is None:
            y = logit
            sample = torch.zeros_like(logit).scatter_(-1, logit.argmax(-1, keepdim=True), 1.0)
        else:
            y = logit + gumbels(uniforms[i], dtype)
            y_soft = y.softmax(-1)
            y_hard = torch.zeros_like(logit).scatter_(-1, y_soft.max(-1, keepdim=True)[1], 1.0)
            sample = y_hard - y_soft + y_soft
        q = torch.einsum("nmk,mkd->nmd", sample, cb).reshape(x.shape[0], -1)
        qs.append(q)
        codes.append(logit.argmax(-1))
        logits.append(logit)
        sampled.append(sample.argmax(-1))
        ys.append(y)
        if i < L - 1:
            x = _lin(sd, f"_encoders.{i}._latentHead", z) - q
    f = None
    for i in reversed(range(L)):
        t = _lin(sd, f"_decoders.{i}._dequantizationHead", qs[i])
        if i < L - 1:
            t = t + _lin(sd, f"_decoders.{i}._sideHead", f)
        f = _lin(sd, f"_decoders.{i}._restoreHead", t)
    return dict(restored=f, codes=codes, logits=logits, loss=F.mse_loss(f, x_gt), sampled=sampled, y=ys)


def umgm_encode(sd, x, m, ks, dtype=None):
    dtype = dtype or x.dtype
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x, L, codes = x.to(dtype), len(ks), []
    for i, k in enumerate(ks):
        z = _lin(sd, f"_encoders.{i}._latentStageEncoder", x)
        distance, _ = _logits(sd, i, _lin(sd, f"_encoders.{i}._quantizationHead", z), m, k)
        code = distance.argmin(-1)
        codes.append(code)
        if i < L - 1:
            cb = sd[f"_encoders.{i}._quantizer._codebook"]
            x = _lin(sd, f"_encoders.{i}._latentHead", z) - cb[torch.arange(m).expand_as(code), code].reshape(x.shape[0], -1)
    return codes


def umgm_decode(sd, codes, m, ks, dtype=torch.float32):
    sd = {k: v.to(dtype) for k, v in sd.items()}
    L, f = len(ks), None
    for i in reversed(range(L)):
        cb = sd[f"_encoders.{i}._quantizer._codebook"]
        q = cb[torch.arange(m).expand_as(codes[i]), codes[i]].reshape(codes[i].shape[0], -1)
        t = _lin(sd, f"_decoders.{i}._dequantizationHead", q)
        if i < L - 1:
            t = t + _lin(sd, f"_decoders.{i}._sideHead", f)
        f = _lin(sd, f"_decoders.{i}._restoreHead", t)
    return f


def top2_gap(v):
    t = v.topk(2, dim=-1).values
    return t[..., 0] - t[..., 1]


def clear_rows(logits64, ys64, rel_err):
    """[n] bool: every decision of the row (the sampled index and the code, every level and group) has a float64 top-2 gap of at least
    CLEAR_FACTOR * rel_err * (the group's largest |logit + gumbel|). A flipped index changes the row from that level on, so a row is
    clear only as a whole."""
    ok = torch.ones(logits64[0].shape[0], dtype=torch.bool)
    for logit, y in zip(logits64, ys64):
        margin = CLEAR_FACTOR * rel_err * y.abs().amax(-1)
        ok &= ((top2_gap(y) >= margin) & (top2_gap(logit) >= margin)).all(-1)
    return ok


def case_data(name, seed):
    c = CASES[name]
    sd = make_params(c["C"], c["m"], c["k"], seed, c["cb_scale"], c["w_scale"])
    return c, sd, make_x(c["n"], c["C"], seed + 1), make_uniforms(c["n"], c["m"], c["k"], seed + 2)

