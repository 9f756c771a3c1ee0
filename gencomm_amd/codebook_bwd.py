"""Backward of ``UMGMQuantizer`` on the HIP kernels (training the CodeFilling codec, and the stage-2 pattern where a frozen codec must
still pass gradients back to its input). Opt-in: ``UMGMQuantizer(..., trainable=True)``.

``UMGMFunction`` wraps the whole codec. Its forward is the inference entry ``gencomm_umgm_fwd`` with the sampled indices requested, so
its outputs are the ``no_grad`` outputs bit for bit. It saves ``x``, the sampled indices and the noise source (the uniforms tensor, or
the Philox seed) -- nothing else; ``gencomm_umgm_bwd`` recomputes the intermediates per 64-row tile, takes the one-hot from the saved
indices and never re-decides an argmax. The straight-through estimator is the reference's ``onehot(s) - p.detach() + p`` with
``p = softmax(logit + gumbel)``; with ``noise=False`` every gumbel is 0.

Differentiable outputs: ``restored`` and ``code_loss``. ``codes``, ``logits`` and the sampled indices are marked non-differentiable (the
baseline's shell discards codes and logits, heter_model_baseline_w_codebook.py:275). The backward returns one gradient blob in the
parameter blob's order, sliced here into per-parameter gradients: a level's tied codebook receives ONE gradient, the sum of its three
uses; the temperature's has gone through ``LowerBound``'s rule in the kernel. A parameter with ``requires_grad=False`` gets ``None``;
if none requires a gradient the kernel's ``dx``-only flag skips all parameter-gradient work. No float atomics: two backward runs give
the same bits in ``dx`` and every gradient.
Reference: sub_modules/codebook.py:147-249, 375-408; utils/codebook_utils.py:19-76.
"""
from __future__ import annotations

import torch

from . import _lib
from .runtime import f32c, ptr, stream_ptr, workspaces


def _unique_params(mod):
    """The parameters in blob order, each once (the blob holds a level's tied codebook once)."""
    return [t for t in mod._blob_tensors() if t is not None]


def _slice_grads(mod, blob):
    """gradient blob -> one gradient per entry of ``_unique_params`` (views of the blob)."""
    C, out, off = mod._channel, [], 0
    for t in mod._blob_tensors():
        if t is None:                                   # the unread latentHead / sideHead slot of the last level
            off += C * C + C
        elif t.dim() == 2 and t.shape[1] == 1:          # temperature [m, 1], padded to 4 in the blob
            out.append(blob[off:off + t.numel()].view_as(t))
            off += 4
        else:
            out.append(blob[off:off + t.numel()].view_as(t))
            off += t.numel()
    assert off == blob.numel(), (off, blob.numel())
    return out


class UMGMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, HW, keep, noise_args, with_logits, *params):
        rows = x.shape[0] if HW == 0 else x.shape[0] * HW
        with torch.no_grad():
            restored, codes, logits, loss, sampled = mod._run(x, rows, HW, keep, None, None, True, with_logits, True, noise_args)
            blob = mod._params(x.device)
        ints = (*codes, *sampled, *(logits or ()))
        ctx.mod, ctx.HW, ctx.keep, ctx.noise_args, ctx.rows = mod, HW, keep, noise_args, rows
        ctx.save_for_backward(x, torch.stack(sampled), blob)                   # [L, rows, m], as the kernel reads it
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*ints)
        return (restored, loss, *ints)

    @staticmethod
    def backward(ctx, g_restored, g_loss, *_):
        mod = ctx.mod
        x, sampled, blob = ctx.saved_tensors
        dev, l = x.device, _lib.lib()
        mode, u, seed = ctx.noise_args
        want = [p.requires_grad for p in _unique_params(mod)]
        dx_only = not any(ctx.needs_input_grad[6:])
        with torch.no_grad():
            dx = torch.empty_like(x)
            dblob = None if dx_only else torch.empty_like(blob)
            if g_restored is None and g_loss is None:
                dx.zero_()
                return (None, dx if ctx.needs_input_grad[1] else None, None, None, None, None,
                        *[torch.zeros_like(p) if w else None for p, w in zip(_unique_params(mod), want)])
            g_restored = None if g_restored is None else f32c(g_restored)
            g_loss = None if g_loss is None else f32c(g_loss)
            need = _lib.check_size(l.gencomm_umgm_bwd_workspace_bytes(ctx.rows, mod._channel, mod._m, mod._k_arr, len(mod._k)),
                                   "gencomm_umgm_bwd_workspace_bytes")
            ws = workspaces.get(dev, need, "umgm_bwd")
            _lib.check(l.gencomm_umgm_bwd(ptr(blob), ptr(x), ptr(ctx.keep), ptr(u), seed, mode, ptr(sampled), ptr(g_restored), ptr(g_loss), ptr(dx),
                                          ptr(dblob), int(dx_only), x.shape[0], ctx.HW, mod._channel, mod._m, mod._k_arr, len(mod._k), ptr(ws),
                                          ws.numel(), stream_ptr(dev)), "gencomm_umgm_bwd")
            grads = [None] * len(want)
            if not dx_only:
                grads = [g if w else None for g, w in zip(_slice_grads(mod, dblob), want)]
        return (None, dx if ctx.needs_input_grad[1] else None, None, None, None, None, *grads)


def run_trainable(mod, x, HW, keep, uniforms, seed, noise, with_logits, with_sampled):
    """The grad-enabled forward of a trainable module: the tuple ``forward`` / ``forward_map`` return."""
    rows = x.shape[0] if HW == 0 else x.shape[0] * HW
    noise_args = mod._noise_args(rows, uniforms, seed, noise, x.device)
    restored, loss, *ints = UMGMFunction.apply(mod, x, HW, keep, noise_args, with_logits, *_unique_params(mod))
    L = len(mod._k)
    out = (restored, ints[:L], ints[2 * L:] if with_logits else None, loss)
    return out + (ints[L:2 * L],) if with_sampled else out
