"""Backward of ``CoBEVT`` on the HIP kernels (training with ``fusion_method: cobevt``: stage 1, and stage 2 where the frozen fusion net
must still pass gradients back to the new agent's message extractor). Opt-in: ``CoBEVT(args, trainable=True)``.

``CoBEVTFunction`` wraps the whole fusion. Its forward is ``CoBEVT._forward_hip`` with a tape: the same kernel calls as inference, the
attention through ``gencomm_swap_attn_train_fwd`` (the same ``out`` bits plus the per-query log-sum-exp), so while dropout is inactive the
output equals the ``no_grad`` output bit for bit. The tape keeps, per attention, its input, ``qkv``, the attention output and ``lse``;
per FeedForward, its input and the (dropped-out) GELU output; and the agent mean. LayerNorm outputs and the GELU pre-activation are
recomputed in the backward. Backward, in reverse:
  head                  Linear (input gradient = the 1x1 convolution with the transposed weight, weight gradient on
                        gencomm_conv2d_wgrad), LayerNorm (gencomm_ln_nchw_bwd), agent mean (g / L to all L rows: padded agents are rows like any other)
  FeedForward           Linear, gencomm_gelu_bwd on the recomputed pre-activation, Linear, LayerNorm
  attention             to_out, gencomm_swap_attn_bwd (dq, dk, dv and the relative-position table's gradient), to_qkv, LayerNorm
  warp to ego           gencomm_warp_affine_bwd per scene over the valid rows; gradient rows of padded agents are dropped
``dx`` is produced whenever ``x.requires_grad``, also with every parameter frozen; a frozen parameter gets ``None`` and its weight
gradient is not computed.

Dropout (``train()`` mode, ``drop_out > 0``): masks ``(torch.rand_like(y) >= p) / (1 - p)`` drawn through ``v2xvit_bwd._Masks``, each in
the shape of the tensor it multiplies (the padded NCHW batch ``[B L, C, H, W]``), per block in this order: window ``to_out``, window FFN
after the GELU, window FFN after the last Linear, then the same three for grid. The backward replays them. No dropout on the attention
probabilities (swap_fusion_modules.py:87-128 has none). The residual additions then run unfused.

Order of additions: the output and the gradient in front of the warp (dq, dk, dv of ``gencomm_swap_attn_bwd`` included) are summed in a
fixed order: two identical steps give the same bits. Every parameter gradient meets in float atomics -- the table in
``gencomm_swap_attn_bwd``, the Linears in ``gencomm_conv2d_wgrad`` (as in ``v2xvit_bwd.py``; the fixed-order
``gencomm_conv2d_wgrad_fixed`` is four times slower at the shipped shapes, ``profiles/cobevt_train_bench.json``), the LayerNorms in
``gencomm_ln_nchw_bwd`` -- and may differ in the last bits between two steps; so may ``dx`` through the warp's scatter
(``gencomm_warp_affine_bwd``), except under identity poses, where one warped pixel with a non-zero weight lands on each input pixel.
Reference: fusion_in_one.py:409-464, fuse_modules/swap_fusion_modules.py:13-192, sub_modules/base_transformer.py:17-40.
"""
from __future__ import annotations

import torch

from . import _lib, train_ops as T
from .runtime import f32c, ptr, stream_ptr
from .v2xvit_bwd import _Masks


def _lin_bwd(dy, x, lin, has_bias):
    """(dx, dW [out, in] or None, db or None) of y = W x + b over NCHW pixels; the weight gradient only where a parameter wants it."""
    dx = T.conv2d(dy, lin.weight.detach().t().contiguous()[:, :, None, None], None, 0)
    if not (lin.weight.requires_grad or (has_bias and lin.bias.requires_grad)):
        return dx, None, None
    dw, db = T.conv2d_wgrad(dy, x, 1, 0, has_bias)
    return dx, dw[:, :, 0, 0], db


class CoBEVTFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, lens, affine_matrix, *params):
        masks = _Masks(mod.training and mod.drop_out > 0)
        tape = []
        with torch.no_grad():
            y = mod._forward_hip(f32c(x), lens, affine_matrix, tape, masks)
        ctx.mod, ctx.lens, ctx.tape, ctx.x_shape = mod, lens, tape, tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, gout):
        mod, lens, tape = ctx.mod, ctx.lens, ctx.tape
        if tape is None:
            raise RuntimeError("CoBEVTFunction: backward through the same forward twice (the tape is released after the first)")
        ctx.tape = None
        l, dev = _lib.lib(), gout.device
        st = stream_ptr(dev)
        n, C, H, W = ctx.x_shape
        L, ws = mod.agent_size, mod.window_size
        B = len(lens)
        grads = {}

        def acc(p, g):
            if g is not None and p.requires_grad:
                grads[p] = g if p not in grads else grads[p] + g

        def unmask(g_, m_):
            return g_ if m_ is None else g_ * m_

        with torch.no_grad():
            _, mean, hn, theta, nvalid = tape.pop()
            norm, lin = mod.mlp_head[2], mod.mlp_head[3]
            dhn, dw, db = _lin_bwd(f32c(gout), hn, lin, True)
            acc(lin.weight, dw); acc(lin.bias, db)
            dmean, dgm, dbt = T.ln_bwd(mean, norm.weight, dhn, norm.eps)
            acc(norm.weight, dgm); acc(norm.bias, dbt)
            g = (dmean / L)[:, None].expand(B, L, C, H, W).reshape(B * L, C, H, W).contiguous()   # the mean's adjoint, to all L rows
            while tape:
                entry = tape.pop()
                pre = entry[1]
                if entry[0] == "ff":
                    _, _, h_in, mid, m_mid, m_out = entry
                    l0, l3 = pre.fn.net[0], pre.fn.net[3]
                    c_ = T.ln_fwd(h_in, pre.norm.weight, pre.norm.bias, pre.norm.eps, False)
                    act_in = T.conv2d(c_, l0.weight.detach()[:, :, None, None], l0.bias, 0)      # the GELU's pre-activation, recomputed
                    dmid, dw3, db3 = _lin_bwd(unmask(g, m_out), mid, l3, True)
                    acc(l3.weight, dw3); acc(l3.bias, db3)
                    dpre = T.gelu_bwd(act_in, unmask(dmid, m_mid))
                    dc, dw0, db0 = _lin_bwd(dpre, c_, l0, True)
                    acc(l0.weight, dw0); acc(l0.bias, db0)
                else:
                    _, _, grid_mode, h_in, qkv, out, lse, table, m = entry
                    att = pre.fn
                    do, dwo, _ = _lin_bwd(unmask(g, m), out, att.to_out[0], False)
                    acc(att.to_out[0].weight, dwo)
                    dqkv = torch.empty_like(qkv)
                    dtable = torch.zeros_like(table)
                    _lib.check(l.gencomm_swap_attn_bwd(ptr(qkv), ptr(table), ptr(nvalid), ptr(out), ptr(lse), ptr(f32c(do)), ptr(dqkv), ptr(dtable),
                                                       B, L, att.heads, att.dim_head, ws, H, W, grid_mode, st), "gencomm_swap_attn_bwd")
                    acc(att.relative_position_bias_table.weight, dtable)
                    c_ = T.ln_fwd(h_in, pre.norm.weight, pre.norm.bias, pre.norm.eps, False)
                    dc, dwq, _ = _lin_bwd(dqkv, c_, att.to_qkv, False)
                    acc(att.to_qkv.weight, dwq)
                dh, dgm, dbt = T.ln_bwd(h_in, pre.norm.weight, dc, pre.norm.eps)
                acc(pre.norm.weight, dgm); acc(pre.norm.bias, dbt)
                g = g + dh
                del entry
            dx = None
            if ctx.needs_input_grad[1]:
                dx = torch.empty(n, C, H, W, dtype=torch.float32, device=dev)
                off = 0
                for b, k in enumerate(lens):   # rows b L + k .. b L + L - 1 belong to padded agents: no input behind them
                    _lib.check(l.gencomm_warp_affine_bwd(ptr(theta[off:]), ptr(g[b * L:]), ptr(dx[off:]), k, C, H, W, st), "gencomm_warp_affine_bwd")
                    off += k
        return (None, dx, None, None, *[grads.get(p) if p.requires_grad else None for p in mod.parameters()])
