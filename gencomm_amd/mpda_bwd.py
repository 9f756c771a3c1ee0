"""Backward of MPDA's feature aligner on the HIP kernels. Opt-in: ``MPDAAlign(args, trainable=True)`` (and the same flag on
``LearnableResizer``, ``SwapFusionEncoder``, ``CrossDomainFusionEncoder``, ``DAImgHead``). In an MPDA run the resizer, ``cdt`` and the
domain classifier are the only trained parts, and the gradient-reversal layer exists only in the backward.

Several ``torch.autograd.Function``s that torch composes; the ``+``, slicing and concatenation of ``LearnableResizer`` / ``MPDAAlign``
stay plain torch:
  SwapEncoderFunction    one per SwapFusionEncoder call. Per window / grid half-block: LN -> to_qkv -> gencomm_quad_attn_train_fwd (self
                         form, rel_pos_bias) -> to_out -> dropout -> skip; LN -> Linear + GELU -> dropout -> Linear -> dropout -> skip;
                         then mlp_head. The attention's adjoint is gencomm_quad_attn_bwd: dq | dk | dv land as the channel blocks of
                         one dqkv that to_qkv's backward reads directly, dbias [9][heads] is rel_pos_bias.weight's gradient as it is
                         (nn.Embedding(9, heads): the same layout).
  CrossDomainFunction    one per CrossDomainFusionEncoder call (no dropout in the reference). The ego is projected once per block
                         (Nkv = 1): dk / dv are the kernel's fixed-order sums over the collaborators' maps, and both the k side and
                         the v side (each through its own LayerNorm) contribute to d ego.
  ResidualBlockFunction  train(): conv3x3 (+ bias) -> bn2d_train_fwd (batch statistics; running statistics and num_batches_tracked
                         updated as nn.BatchNorm2d does) -> gencomm_leaky_relu_fwd -> conv3x3 -> BatchNorm -> + x. eval() with
                         gradients: the folded layers of the inference path, gradients to the convolutions and the BatchNorm affine
                         parameters through the fold. Backward on conv2d_dgrad / conv2d_wgrad_fixed, bn2d_train_bwd and
                         gencomm_leaky_relu_bwd.
  ResizeFunction         gencomm_resize_bilinear_fwd / gencomm_resize_bilinear_bwd.
  DAHeadFunction         two 1x1 convolutions and a ReLU (its adjoint is gencomm_leaky_relu_bwd at slope 0). The gradient that leaves
                         the head towards the features is multiplied by rgl.weight (-9.1: the gradient-reversal layer, folded into the
                         transposed weight of the last input-gradient GEMM); the head's own parameter gradients are unscaled.
The resizer's 1x1 ``channel_selector`` goes through ``bev_backbone.conv2d_hip``, which has its own HIP backward.

As ``cobevt_bwd.py``: each Function keeps a tape that is released after the first backward (a second backward through the same forward
raises ``RuntimeError``; double backward is not built: the backward runs under ``no_grad``); LayerNorm outputs and GELU pre-activations
are recomputed; a frozen parameter gets ``None`` and its weight-gradient launch is skipped; the input gradient is produced whenever the
input requires it, also with every parameter frozen. While dropout is inactive and the BatchNorms are in eval mode the forward is
the inference path's kernel calls: the same bits.

Dropout (``train()`` mode, ``drop_out > 0``), drawn through ``v2xvit_bwd._Masks`` per SwapFusionEncoder call, per block, for window
then grid, in this order:
  1. the attention's keep mask: ``torch.rand(n, heads, X Y, 16, device) >= p`` (element 4 i + j: query token i, key token j of the
     2 x 2 group x Y + y), packed by ``mpda.pack_keep`` into the kernel's uint16 words, surviving probabilities scaled by 1 / (1 - p);
  2. after to_out, 3. after the GELU, 4. after the FeedForward's last Linear: ``(torch.rand_like(y) >= p) / (1 - p)`` in the shape of
     the tensor each multiplies.
A test re-seeds torch's generator, draws the same sequence itself and feeds it to the restatement.

Order of additions: everything the new kernels write (dq, dk, dv, dbias, the resize adjoint) is a fixed-order sum; the residual
block's weight gradients go through ``gencomm_conv2d_wgrad_fixed``. The Linears' weight gradients (``gencomm_conv2d_wgrad``) and the
LayerNorm parameter gradients (``gencomm_ln_nchw_bwd``) meet in float atomics, as in ``cobevt_bwd.py``, and may differ in the last bits
between two steps.
Reference: opencood/models/mpda_modules/{wg_fusion_modules,resizer,classfier,gradient_layer}.py, heter_model_baseline_w_mpda.py:232-262.
"""
from __future__ import annotations

import torch

from . import train_ops as T
from .bev_backbone import conv2d_hip
from .cobevt_bwd import _lin_bwd
from .mpda import _conv_bn_act, leaky_relu, leaky_relu_bwd, quad_attention_bwd, resize_bilinear, resize_bilinear_bwd
from .runtime import f32c
from .v2xvit_bwd import _Masks


def _take_tape(ctx, name):
    tape = ctx.tape
    if tape is None:
        raise RuntimeError(f"{name}: backward through the same forward twice (the tape is released after the first)")
    ctx.tape = None
    return tape


class _Grads:
    """Gradients per parameter; a frozen parameter is never stored."""

    def __init__(self):
        self.g = {}

    def acc(self, p, g):
        if p is not None and g is not None and p.requires_grad:
            self.g[p] = g if p not in self.g else self.g[p] + g

    def out(self, mod):
        return [self.g.get(p) if p.requires_grad else None for p in mod.parameters()]


def _unmask(g, m):
    return g if m is None else g * m


def _ln_lin_bwd(G, x_in, norm, lin, dy):
    """Adjoint of lin(LN(x_in)) -> d x_in; the LayerNorm output is recomputed."""
    c = T.ln_fwd(x_in, norm.weight, norm.bias, norm.eps, False)
    dc, dw, db = _lin_bwd(dy, c, lin, lin.bias is not None)
    G.acc(lin.weight, dw); G.acc(lin.bias, db)
    dx, dg, dbt = T.ln_bwd(x_in, norm.weight, dc, norm.eps)
    G.acc(norm.weight, dg); G.acc(norm.bias, dbt)
    return dx


def _mlp_bwd(G, g, x_in, mid, norm, l0, l1, m_mid=None, m_out=None):
    """Adjoint of x + drop(l1(drop(GELU(l0(LN(x)))))) without the skip -> d x_in through the LayerNorm."""
    c = T.ln_fwd(x_in, norm.weight, norm.bias, norm.eps, False)
    act_in = T.conv2d(c, l0.weight.detach()[:, :, None, None], l0.bias, 0)       # the GELU's pre-activation, recomputed
    dmid, dw1, db1 = _lin_bwd(_unmask(g, m_out), mid, l1, True)
    G.acc(l1.weight, dw1); G.acc(l1.bias, db1)
    dpre = T.gelu_bwd(act_in, _unmask(dmid, m_mid))
    dc, dw0, db0 = _lin_bwd(dpre, c, l0, True)
    G.acc(l0.weight, dw0); G.acc(l0.bias, db0)
    dx, dg, dbt = T.ln_bwd(x_in, norm.weight, dc, norm.eps)
    G.acc(norm.weight, dg); G.acc(norm.bias, dbt)
    return dx


def _head_bwd(G, gout, h, mlp_head):
    return _ln_lin_bwd(G, h, mlp_head[1], mlp_head[2], f32c(gout))


class SwapEncoderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, *params):
        masks = _Masks(mod.training and mod.dropout_p() > 0)
        tape = []
        with torch.no_grad():
            y = mod._forward_hip(x, tape, masks)
        ctx.mod, ctx.tape = mod, tape
        return y

    @staticmethod
    def backward(ctx, gout):
        mod, tape = ctx.mod, _take_tape(ctx, "SwapEncoderFunction")
        G = _Grads()
        with torch.no_grad():
            g = _head_bwd(G, gout, tape.pop()[1], mod.mlp_head)
            while tape:
                entry = tape.pop()
                pre = entry[1]
                if entry[0] == "ff":
                    _, _, h_in, mid, m_mid, m_out = entry
                    dh = _mlp_bwd(G, g, h_in, mid, pre.norm, pre.fn.net[0], pre.fn.net[3], m_mid, m_out)
                else:
                    _, _, grid_mode, h_in, qkv, out, table, keep, ks, m = entry
                    att = pre.fn
                    inner = att.heads * att.dim_head
                    do, dwo, _ = _lin_bwd(_unmask(g, m), out, att.to_out[0], False)
                    G.acc(att.to_out[0].weight, dwo)
                    dqkv, _, _, dtable = quad_attention_bwd(qkv, qkv, qkv, table, f32c(do), att.heads, att.dim_head, grid_mode, 0, inner, 2 * inner,
                                                            keep, ks, self_form=True)
                    G.acc(att.rel_pos_bias.weight, dtable)
                    dh = _ln_lin_bwd(G, h_in, pre.norm, att.to_qkv, dqkv)
                g = g + dh
                del entry
        return (None, g if ctx.needs_input_grad[1] else None, *G.out(mod))


class CrossDomainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, ego, cav, *params):
        tape = []
        with torch.no_grad():
            ego_c = f32c(ego)
            y = mod._forward_hip(ego_c, cav, tape)
        ctx.mod, ctx.tape, ctx.ego = mod, tape, ego_c
        return y

    @staticmethod
    def backward(ctx, gout):
        mod, tape, ego = ctx.mod, _take_tape(ctx, "CrossDomainFunction"), ctx.ego
        ctx.ego = None
        G = _Grads()
        dego = None
        with torch.no_grad():
            g = _head_bwd(G, gout, tape.pop()[1], mod.mlp_head)
            while tape:
                entry = tape.pop()
                if entry[0] == "ln":
                    _, norm, x_in = entry
                    g, dg, dbt = T.ln_bwd(x_in, norm.weight, g, norm.eps)
                    G.acc(norm.weight, dg); G.acc(norm.bias, dbt)
                elif entry[0] == "mlp":
                    _, norm, mlp, x_in, mid = entry
                    g = g + _mlp_bwd(G, g, x_in, mid, norm, mlp[0], mlp[2])
                else:
                    _, att, grid_mode, x_in, q, k, v, a = entry
                    da, dwp, dbp = _lin_bwd(g, a, att.proj, True)
                    G.acc(att.proj.weight, dwp); G.acc(att.proj.bias, dbp)
                    dq, dk, dv, _ = quad_attention_bwd(q, k, v, None, f32c(da), att.heads, att.dim_head, grid_mode)
                    g = g + _ln_lin_bwd(G, x_in, att.to_q[0], att.to_q[1], dq)
                    de = _ln_lin_bwd(G, ego, att.to_k[0], att.to_k[1], dk) + _ln_lin_bwd(G, ego, att.to_v[0], att.to_v[1], dv)
                    dego = de if dego is None else dego + de
                del entry
        return (None, dego if ctx.needs_input_grad[1] else None, g if ctx.needs_input_grad[2] else None, *G.out(mod))


def _conv3_bwd(G, x, g, conv, need_x):
    """Adjoint of the bare 3x3 convolution (stride 1, pad 1) given d(conv output): fixed-order weight gradient, dgrad."""
    if conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad):
        dw, db = T.conv2d_wgrad_fixed(g, x, 3, conv.bias is not None)
        G.acc(conv.weight, dw); G.acc(conv.bias, db)
    return T.conv2d_dgrad(g, conv.weight, 1) if need_x else None


def _conv_bn_eval_bwd(G, x, g, conv, bn, need_x):
    """Adjoint of BN_eval(conv(x)), y = s (conv + bias - mean) + beta with s = gamma / sqrt(var + eps), through the fold."""
    rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
    if bn.weight.requires_grad or bn.bias.requires_grad:
        pre = T.conv2d(x, conv.weight, conv.bias, 1)                          # the convolution's own output, unfused
        dots = T.nc_dot(g, pre).sum(0), T.nc_dot(g, None).sum(0)              # per channel: sum g pre, sum g
        G.acc(bn.weight, (dots[0] - bn.running_mean.float() * dots[1]) * rstd)
        G.acc(bn.bias, dots[1])
    n = g.shape[0]
    gs = T.nc_scale(g, (bn.weight.detach().float() * rstd)[None].expand(n, -1).contiguous(), None)
    return _conv3_bwd(G, x, gs, conv, need_x)


class ResidualBlockFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, *params):
        m = mod.module
        with torch.no_grad():
            x = f32c(x)
            if T.bn_batch_statistics(m[1]):
                c1 = T.conv2d(x, m[0].weight, m[0].bias, 1)
                y1, save1 = T.bn2d_train_fwd(c1, m[1], False)
                a = leaky_relu(y1, m[2].negative_slope)
                c2 = T.conv2d(a, m[3].weight, m[3].bias, 1)
                y2, save2 = T.bn2d_train_fwd(c2, m[4], False)
                out = y2 + x
                ctx.tape = ("batch", x, c1, y1, save1, a, c2, y2, save2)
            else:
                a = _conv_bn_act(x, m[0], m[1], 4)
                out = _conv_bn_act(a, m[3], m[4], 0, residual=x)
                ctx.tape = ("folded", x, a)
        ctx.mod = mod
        return out

    @staticmethod
    def backward(ctx, gout):
        mod, tape = ctx.mod, _take_tape(ctx, "ResidualBlockFunction")
        m, G = mod.module, _Grads()
        need_x = ctx.needs_input_grad[1]
        slope = m[2].negative_slope
        with torch.no_grad():
            g = f32c(gout)
            if tape[0] == "batch":
                _, x, c1, y1, save1, a, c2, y2, save2 = tape
                dc2, dg4, db4 = T.bn2d_train_bwd(c2, y2, g, save2, m[4].weight, False)
                G.acc(m[4].weight, dg4); G.acc(m[4].bias, db4)
                da = _conv3_bwd(G, a, dc2, m[3], True)
                dc1, dg1, db1 = T.bn2d_train_bwd(c1, y1, leaky_relu_bwd(a, da, slope), save1, m[1].weight, False)
                G.acc(m[1].weight, dg1); G.acc(m[1].bias, db1)
                dx = _conv3_bwd(G, x, dc1, m[0], need_x)
            else:
                _, x, a = tape
                da = _conv_bn_eval_bwd(G, a, g, m[3], m[4], True)
                dx = _conv_bn_eval_bwd(G, x, leaky_relu_bwd(a, da, slope), m[0], m[1], need_x)
            dx = dx + g if need_x else None
        return (None, dx, *G.out(mod))


class ResizeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.in_size = tuple(x.shape[2:])
        with torch.no_grad():
            return resize_bilinear(x, size)

    @staticmethod
    def backward(ctx, gout):
        with torch.no_grad():
            return resize_bilinear_bwd(gout, ctx.in_size), None


class DAHeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, *params):
        with torch.no_grad():
            x = f32c(x)
            h = conv2d_hip(x, mod.conv1_da, None, relu=True)
            y = conv2d_hip(h, mod.conv2_da, None, relu=False)
        ctx.mod, ctx.tape = mod, (x, h)
        return y

    @staticmethod
    def backward(ctx, gout):
        mod = ctx.mod
        x, h = _take_tape(ctx, "DAHeadFunction")
        c1, c2 = mod.conv1_da, mod.conv2_da
        G = _Grads()
        with torch.no_grad():
            g = f32c(gout)
            if c2.weight.requires_grad or c2.bias.requires_grad:
                dw, db = T.conv2d_wgrad(g, h, 1, 0, True)
                G.acc(c2.weight, dw); G.acc(c2.bias, db)
            dh = T.conv2d(g, c2.weight.detach()[:, :, 0, 0].t().contiguous()[:, :, None, None], None, 0)
            dpre = leaky_relu_bwd(h, dh, 0.0)                                      # the ReLU's adjoint, from its output
            if c1.weight.requires_grad or c1.bias.requires_grad:
                dw, db = T.conv2d_wgrad(dpre, x, 1, 0, True)
                G.acc(c1.weight, dw); G.acc(c1.bias, db)
            dx = None
            if ctx.needs_input_grad[1]:
                # the gradient-reversal layer (x -> rgl(x) in front of conv1_da): its factor rides on the transposed weight
                wt = (c1.weight.detach()[:, :, 0, 0].t() * float(mod.rgl.weight)).contiguous()
                dx = T.conv2d(dpre, wt[:, :, None, None], None, 0)
        return (None, dx, *G.out(mod))
