"""The CodeFilling codec's TRAINING forward restated in plain torch, differentiable, in any dtype: codebook_restatement.umgm_forward
with the reference's straight-through sample ``onehot(s) - p.detach() + p`` (utils/codebook_utils.py:71) -- the inference restatement
writes ``y_hard - y_soft + y_soft``, whose gradient cancels to zero -- and ``LowerBound``'s gradient rule (codebook_utils.py:19-31).

``forced``: an optional list of sampled indices (L x [n, m]). With forced indices the function is smooth in every input, so gradients
can be compared at any shape, with no near-tie margin and no excluded rows. Used by the CPU tests against tests/golden/codebook_train.npz
(written by tools/make_golden_codebook_train.py from the reference's own module), as truth (float64) and yardstick (float32) of the GPU
tests, and as the torch baseline of tools/codebook_train_bench.py.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import codebook_restatement as R

LOSS_WEIGHT = 3.0            # the fixture's objective: sum(restored * G) + LOSS_WEIGHT * code_loss
SUBSAMPLE = 256              # elements of a gradient tensor the fixture stores (7 cases x ~40 tensors must stay under 1 MiB)

# strict: cb_scale 4 / w_scale 2 spread the logits so that every row's decisions are clear; soft: the default initialisation, where
# the softmax adjoint dominates (forced indices)
CASES = {
    "strict_a": dict(C=64, m=2, k=[16, 16, 16], n=128, cb_scale=4.0, w_scale=2.0),
    "strict_b": dict(C=64, m=4, k=[32, 16], n=64, cb_scale=4.0, w_scale=2.0),
    "c128_three_tiles": dict(C=128, m=2, k=[16, 16, 16], n=192, cb_scale=4.0, w_scale=2.0),
    "c256": dict(C=256, m=2, k=[16, 16, 16], n=128, cb_scale=4.0, w_scale=2.0),
    "c256_m1_k256": dict(C=256, m=1, k=[256], n=100, cb_scale=4.0, w_scale=2.0),
    "c128_m4": dict(C=128, m=4, k=[64, 32], n=100, cb_scale=4.0, w_scale=2.0),
    "soft": dict(C=64, m=2, k=[16, 16, 16], n=128, cb_scale=1.0, w_scale=1.0),
}
STRICT = tuple(name for name in CASES if name != "soft")


class _LowerBound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_, bound):
        ctx.save_for_backward(input_, bound)
        return torch.max(input_, bound)

    @staticmethod
    def backward(ctx, grad_output):
        input_, bound = ctx.saved_tensors
        return ((input_ >= bound) | (grad_output < 0)).type(grad_output.dtype) * grad_output, None


def param_keys(sd):
    """The trainable tensors of a state_dict, each once: a level's codebook under its quantizer key only."""
    return [k for k in sd if not k.endswith("_bound.bound") and "_dequantizer._codebook" not in k]


def case_data(name, seed):
    c = CASES[name]
    sd = R.make_params(c["C"], c["m"], c["k"], seed, c["cb_scale"], c["w_scale"])
    g = torch.from_numpy(np.random.default_rng(seed + 3).normal(0.0, 1.0, (c["n"], c["C"])).astype(np.float32))
    return c, sd, R.make_x(c["n"], c["C"], seed + 1), R.make_uniforms(c["n"], c["m"], c["k"], seed + 2), g


def train_forward(P, x, m, ks, uniforms=None, forced=None, x_gt=None):
    """P: {key: tensor} over param_keys (leaves that may require grad) plus the bound buffers; x may require grad.
    -> dict(restored, loss, sampled, logits, y). ``x_gt``: the loss target (default x.detach())."""
    L, n = len(ks), x.shape[0]
    x_gt = x.detach() if x_gt is None else x_gt
    lin = lambda prefix, v: F.linear(v, P[prefix + ".weight"], P[prefix + ".bias"])
    qs, sampled, logits, ys = [], [], [], []
    for i, k in enumerate(ks):
        cb = P[f"_encoders.{i}._quantizer._codebook"]
        z = lin(f"_encoders.{i}._latentStageEncoder", x)
        hg = lin(f"_encoders.{i}._quantizationHead", z).reshape(n, m, -1)
        distance = (hg ** 2).sum(2, keepdim=True) + (cb ** 2).sum(-1) - 2 * torch.einsum("nmd,mkd->nmk", hg, cb)
        temp = _LowerBound.apply(P[f"_encoders.{i}._quantizer._temperature"], P[f"_encoders.{i}._quantizer._bound.bound"])
        logit = (-1 * distance) / math.sqrt(k) * temp
        y = logit if uniforms is None else logit + R.gumbels(uniforms[i], logit.dtype)
        p = y.softmax(-1)
        s = p.max(-1, keepdim=True)[1] if forced is None else forced[i].unsqueeze(-1)
        sample = torch.zeros_like(logit).scatter_(-1, s, 1.0) - p.detach() + p
        q = torch.einsum("nmk,mkd->nmd", sample, cb).reshape(n, -1)
        qs.append(q)
        sampled.append(s[..., 0])
        logits.append(logit)
        ys.append(y)
        if i < L - 1:
            x = lin(f"_encoders.{i}._latentHead", z) - q
    f = None
    for i in reversed(range(L)):
        t = lin(f"_decoders.{i}._dequantizationHead", qs[i])
        if i < L - 1:
            t = t + lin(f"_decoders.{i}._sideHead", f)
        f = lin(f"_decoders.{i}._restoreHead", t)
    return dict(restored=f, loss=F.mse_loss(f, x_gt), sampled=sampled, logits=logits, y=ys)


def gradients(sd, x, m, ks, uniforms, forced, G, loss_weight, dtype, x_gt=None, keep_rows=None):
    """Gradients of sum(restored_out * G) + loss_weight * code_loss, restored_out = restored with the rows of ``keep_rows`` (bool [n])
    replaced by x -> (dict key -> gradient over param_keys plus "x", the forward's dict)."""
    P = {k: v.detach().to(dtype) for k, v in sd.items()}
    keys = param_keys(sd)
    for k in keys:
        P[k].requires_grad_(True)
    for i in range(len(ks)):        # the tied uses of a codebook are the quantizer's tensor
        P[f"_encoders.{i}._dequantizer._codebook"] = P[f"_decoders.{i}._dequantizer._codebook"] = P[f"_encoders.{i}._quantizer._codebook"]
    xx = x.detach().to(dtype).requires_grad_(True)
    out = train_forward(P, xx, m, ks, None if uniforms is None else uniforms, forced, None if x_gt is None else x_gt.to(dtype))
    restored = out["restored"]
    if keep_rows is not None:
        restored = torch.where(keep_rows[:, None], xx, restored)
    obj = loss_weight * out["loss"]
    if G is not None:
        obj = obj + (restored * G.to(dtype)).sum()
    grads = torch.autograd.grad(obj, [xx] + [P[k] for k in keys], allow_unused=True)
    res = {"x": grads[0]}
    for k, g in zip(keys, grads[1:]):
        res[k] = torch.zeros_like(P[k]) if g is None else g
    return res, out


def rel_rms(a, b):
    """relative rms error of a against the truth b"""
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-300))


def subsample(t):
    flat = t.reshape(-1)
    step = max(1, (flat.numel() + SUBSAMPLE - 1) // SUBSAMPLE)
    return flat[::step]
