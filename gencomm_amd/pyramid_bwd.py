"""Training HEAL's PyramidFusion: the host side of ``csrc/pyramid_bwd_kernels.h``.

Four ``torch.autograd.Function``s behind the opt-in ``trainable=True`` keyword of ``bev_backbone.gconv3x3_hip``,
``pyramid_fuse.score_head`` / ``weighted_fuse`` and ``PyramidFusion``:

  GconvEvalFn       act(BN_eval(grouped 3x3)): the inference launch forward; ReLU mask from the output, BatchNorm affine gradients as
                    ``bev_backbone._hip_backward`` computes them, then ``gencomm_gconv3x3_dgrad`` / ``gencomm_gconv3x3_wgrad_fixed``.
                    With every parameter frozen only ``dx`` is computed (HEAL's new-agent stage).
  GconvBnTrainFn    act(BN_batch(grouped 3x3)): the bare grouped convolution, then ``train_ops.bn2d_train_fwd`` / ``bn2d_train_bwd`` around
                    it (running statistics and the counter updated as ``nn.BatchNorm2d`` does).
  ScoreHeadFn       (occ, score) of one level; backward = one launch of ``gencomm_pyramid_score_bwd`` from whichever of the two
                    cotangents arrived.
  WeightedFuseFn    saves x, score, theta and the scene table; ``gencomm_warp_weightfuse_bwd`` recomputes cells and shares.

The training paths pack the grouped weight on every call (no per-module cache: a stale pack after an optimizer step cannot happen).
Every backward runs under ``no_grad`` and is ``once_differentiable`` (double backward raises); the tape is released after the first
backward, so a second backward through the same forward raises ``RuntimeError``. Every sum the new kernels make has a fixed order.
Reference: opencood/models/fuse_modules/pyramid_fuse.py, sub_modules/resblock.py:67-122."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import train_ops as T
from .runtime import f32c, ptr, stream_ptr


def _take_tape(ctx, name):
    tape = ctx.tape
    if tape is None:
        raise RuntimeError(f"{name}: backward through the same forward twice (the tape is released after the first)")
    ctx.tape = None
    return tape


# ------------------------------------------------------------------------------------------- the grouped 3x3
def gconv3x3_raw(x: torch.Tensor, w: torch.Tensor, cpg: int, stride: int) -> torch.Tensor:
    """The bare grouped convolution (no norm, no activation) with a freshly packed weight."""
    x, w = f32c(x), f32c(w)
    n, c, H, W = x.shape
    l, st = _lib.lib(), stream_ptr(x.device)
    packed = torch.empty(w.numel(), dtype=torch.float32, device=x.device)
    _lib.check(l.gencomm_gconv3x3_prepare(ptr(w), ptr(packed), cpg, st), "gencomm_gconv3x3_prepare")
    unit = T._unit_scale_shift(c, x.device)
    y = torch.empty(n, c, (H - 1) // stride + 1, (W - 1) // stride + 1, dtype=torch.float32, device=x.device)
    _lib.check(l.gencomm_gconv3x3_fwd(ptr(x), ptr(packed), ptr(unit[0]), ptr(unit[1]), ptr(y), n, c, cpg, H, W, stride, 0, st), "gencomm_gconv3x3_fwd")
    return y


def gconv3x3_dgrad(dy: torch.Tensor, w: torch.Tensor, cpg: int, stride: int, in_hw) -> torch.Tensor:
    """dx [n, C, H, W] of the grouped 3x3 from dy [n, C, Ho, Wo] and the forward weight; ``in_hw`` = (H, W) of the forward input."""
    dy, w = f32c(dy), f32c(w)
    n, c = dy.shape[:2]
    H, W = in_hw
    if tuple(dy.shape[2:]) != ((H - 1) // stride + 1, (W - 1) // stride + 1):
        raise ValueError(f"gconv3x3_dgrad: dy {tuple(dy.shape)} does not belong to a {H} x {W} input at stride {stride}")
    l, st, dev = _lib.lib(), stream_ptr(dy.device), dy.device
    packed = torch.empty(w.numel(), dtype=torch.float32, device=dev)
    _lib.check(l.gencomm_gconv3x3_prepare_t(ptr(w), ptr(packed), cpg, st), "gencomm_gconv3x3_prepare_t")
    unit = T._unit_scale_shift(c, dev)
    dx = torch.empty(n, c, H, W, dtype=torch.float32, device=dev)
    spread = torch.empty(n, c, H, W, dtype=torch.float32, device=dev) if stride == 2 else None
    _lib.check(l.gencomm_gconv3x3_dgrad(ptr(dy), ptr(packed), ptr(unit[0]), ptr(unit[1]), ptr(dx), ptr(spread), n, c, cpg, H, W, stride, st),
               "gencomm_gconv3x3_dgrad")
    return dx


def gconv3x3_wgrad(x: torch.Tensor, dy: torch.Tensor, cpg: int, stride: int) -> torch.Tensor:
    """dw [C, cpg, 3, 3] of the grouped 3x3 (fixed order of additions)."""
    x, dy = f32c(x), f32c(dy)
    n, c, H, W = x.shape
    l = _lib.lib()
    need = _lib.check_size(l.gencomm_gconv3x3_wgrad_fixed_scratch_floats(n, cpg, H, W, stride), "gencomm_gconv3x3_wgrad_fixed_scratch_floats")
    scratch = torch.empty(need, dtype=torch.float32, device=x.device)
    dw = torch.empty(c, cpg, 3, 3, dtype=torch.float32, device=x.device)
    _lib.check(l.gencomm_gconv3x3_wgrad_fixed(ptr(x), ptr(dy), ptr(dw), n, c, cpg, H, W, stride, ptr(scratch), need, stream_ptr(x.device)),
               "gencomm_gconv3x3_wgrad_fixed")
    return dw


def _gconv_backward(x, g, conv, cpg, need_x):
    """(dx, dw) of the bare grouped convolution given d(conv output); either is None when nobody asks for it."""
    s = conv.stride[0]
    dx = gconv3x3_dgrad(g, conv.weight.detach(), cpg, s, (x.shape[2], x.shape[3])) if need_x else None
    dw = gconv3x3_wgrad(x, g, cpg, s) if conv.weight.requires_grad else None
    return dx, dw


def _layer_params(conv, bn):
    return [p for p in (conv.weight,) + ((bn.weight, bn.bias) if bn is not None else ()) if p is not None]


class GconvEvalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, conv, bn, relu, cpg, *params):
        from .bev_backbone import gconv3x3_hip
        ctx.conv, ctx.bn, ctx.relu, ctx.cpg = conv, bn, relu, cpg
        with torch.no_grad():
            xc = f32c(x)
            y = gconv3x3_hip(xc, conv, bn, relu)      # the inference launch (cached pack and fold, keyed by the parameters' versions)
        ctx.tape = (xc, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y = _take_tape(ctx, "GconvEvalFn")
        conv, bn, cpg = ctx.conv, ctx.bn, ctx.cpg
        grads = {}
        with torch.no_grad():
            g = gy.float().contiguous()
            if ctx.relu:
                g = g * (y > 0)
            if bn is not None:   # eval-mode BatchNorm: y = scale (conv - mean) + beta
                rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
                if bn.weight.requires_grad or bn.bias.requires_grad:
                    pre = gconv3x3_raw(x, conv.weight.detach(), cpg, conv.stride[0])
                    grads[bn.weight] = (g * (pre - bn.running_mean.float().view(1, -1, 1, 1))).sum((0, 2, 3)) * rstd
                    grads[bn.bias] = g.sum((0, 2, 3))
                g = g * (bn.weight.detach().float() * rstd).view(1, -1, 1, 1)
            dx, dw = _gconv_backward(x, g, conv, cpg, ctx.needs_input_grad[0])
        grads[conv.weight] = dw
        return (dx, None, None, None, None, *[grads.get(p) if p.requires_grad else None for p in _layer_params(conv, bn)])


class GconvBnTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, conv, bn, relu, cpg, *params):
        ctx.conv, ctx.bn, ctx.relu, ctx.cpg = conv, bn, relu, cpg
        with torch.no_grad():
            xc = f32c(x)
            pre = gconv3x3_raw(xc, conv.weight.detach(), cpg, conv.stride[0])
            y, save = T.bn2d_train_fwd(pre, bn, relu)
        ctx.tape = (xc, pre, y, save)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, pre, y, save = _take_tape(ctx, "GconvBnTrainFn")
        conv, bn = ctx.conv, ctx.bn
        with torch.no_grad():
            dpre, dg, db = T.bn2d_train_bwd(pre, y, gy.float().contiguous(), save, bn.weight.detach(), ctx.relu)
            dx, dw = _gconv_backward(x, dpre, conv, ctx.cpg, ctx.needs_input_grad[0])
        grads = {conv.weight: dw, bn.weight: dg, bn.bias: db}
        return (dx, None, None, None, None, *[grads.get(p) if p.requires_grad else None for p in _layer_params(conv, bn)])


def gconv3x3_train(x, conv, bn, relu, cpg, grad, stats):
    """What ``gconv3x3_hip(..., trainable=True)`` does beyond inference: the autograd path, or batch statistics under ``no_grad``."""
    if grad:
        fn = GconvBnTrainFn if stats else GconvEvalFn
        return fn.apply(x, conv, bn, relu, cpg, *_layer_params(conv, bn))
    y, _ = T.bn2d_train_fwd(gconv3x3_raw(x, conv.weight.detach(), cpg, conv.stride[0]), bn, relu)
    return y


# ------------------------------------------------------------------------------------------- the score head
def score_head_bwd(x, weight, occ, rect, d_occ, d_score, need_x, need_w):
    """(dx, dw [1, C, 1, 1], db [1]) of ``score_head``; d_occ / d_score: either may be None, dx / (dw, db) are None unless asked for."""
    n, C, H, W = x.shape
    l, dev = _lib.lib(), x.device
    dx = torch.empty_like(x) if need_x else None
    dw = db = scratch = None
    need = 0
    if need_w:
        need = _lib.check_size(l.gencomm_pyramid_score_bwd_scratch_floats(n, C, H, W), "gencomm_pyramid_score_bwd_scratch_floats")
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
        dw = torch.empty(1, C, 1, 1, dtype=torch.float32, device=dev)
        db = torch.empty(1, dtype=torch.float32, device=dev)
    d_occ = f32c(d_occ) if d_occ is not None else None
    d_score = f32c(d_score) if d_score is not None else None
    _lib.check(l.gencomm_pyramid_score_bwd(ptr(x), ptr(weight), ptr(occ), ptr(rect), ptr(d_occ), ptr(d_score), ptr(dx), ptr(dw), ptr(db), n, C, H, W,
                                           ptr(scratch), need, stream_ptr(dev)), "gencomm_pyramid_score_bwd")
    return dx, dw, db


class ScoreHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rect, weight, bias):
        with torch.no_grad():
            xc, wc = f32c(x), f32c(weight)
            n, C, H, W = xc.shape
            occ = torch.empty((n, 1, H, W), dtype=torch.float32, device=xc.device)
            score = torch.empty_like(occ)
            _lib.check(_lib.lib().gencomm_pyramid_score_fwd(ptr(xc), ptr(wc), ptr(f32c(bias)), ptr(rect), ptr(occ), ptr(score), n, C, H, W,
                                                            stream_ptr(xc.device)), "gencomm_pyramid_score_fwd")
        ctx.tape = (xc, wc, occ, rect)
        ctx.set_materialize_grads(False)
        return occ, score

    @staticmethod
    @once_differentiable
    def backward(ctx, d_occ, d_score):
        x, w, occ, rect = _take_tape(ctx, "ScoreHeadFn")
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        if (d_occ is None and d_score is None) or not (need_x or need_w):
            return None, None, None, None
        with torch.no_grad():
            dx, dw, db = score_head_bwd(x, w, occ, rect, d_occ, d_score, need_x, need_w)
        return dx, None, dw if ctx.needs_input_grad[2] else None, db if ctx.needs_input_grad[3] else None


# ------------------------------------------------------------------------------------------- the weighted fuse
def weighted_fuse_bwd(x, score, theta, off_dev, dout, B):
    """(dx, dscore) of ``weighted_fuse`` from what its forward was given."""
    n, C, H, W = x.shape
    l, dev = _lib.lib(), x.device
    need = _lib.check_size(l.gencomm_warp_weightfuse_bwd_scratch_floats(n, H, W), "gencomm_warp_weightfuse_bwd_scratch_floats")
    scratch = torch.empty(need, dtype=torch.float32, device=dev)
    dx, dscore = torch.empty_like(x), torch.empty_like(score)
    _lib.check(l.gencomm_warp_weightfuse_bwd(ptr(x), ptr(score), ptr(theta), ptr(off_dev), ptr(f32c(dout)), ptr(dx), ptr(dscore), ptr(scratch), need,
                                             B, n, C, H, W, stream_ptr(dev)), "gencomm_warp_weightfuse_bwd")
    return dx, dscore


class WeightedFuseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, score, theta, off_dev, B):
        with torch.no_grad():
            xc, sc = f32c(x), f32c(score)
            n, C, H, W = xc.shape
            out = torch.empty((B, C, H, W), dtype=torch.float32, device=xc.device)
            _lib.check(_lib.lib().gencomm_warp_weightfuse_fwd(ptr(xc), ptr(sc), ptr(theta), ptr(off_dev), ptr(out), B, n, C, H, W,
                                                              stream_ptr(xc.device)), "gencomm_warp_weightfuse_fwd")
        ctx.tape, ctx.B = (xc, sc, theta, off_dev), B
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, score, theta, off_dev = _take_tape(ctx, "WeightedFuseFn")
        with torch.no_grad():
            dx, dscore = weighted_fuse_bwd(x, score, theta, off_dev, dout, ctx.B)
        return dx if ctx.needs_input_grad[0] else None, dscore if ctx.needs_input_grad[1] else None, None, None, None
