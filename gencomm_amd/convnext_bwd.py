"""Backward of the fused ConvNeXt block and of the modules built from it (training STAMP's adapter and reverter, the only trained parts
of a STAMP run). Opt-in: ``Adapter(args, trainable=True)`` / ``Reverter(args, trainable=True)``.

``convnext_block_bwd`` is ``gencomm_convnext_block_bwd`` (csrc/convnext_bwd_kernels.h): from the block's INPUT map, ``dy`` and the nine
parameters it writes ``dx`` and every parameter gradient in at most ``LAUNCHES`` launches (``LAUNCHES_DX_ONLY`` with ``dx_only``); the
``[pixels, 4 dim]`` pre-activation and activation are recomputed tile by tile and never stored. No float atomics: two runs give the
same bits.

``ConvNextFunction`` wraps one call of an ``adapterconvnext`` module. Its forward is the inference path's five launches (the blocks write
fresh maps instead of ping-ponging, because each block's input is the tape); it saves the module input and ``num_of_blocks + 1`` maps of
``[n, dim, H, W]``. The two 1x1 convolutions go back through ``train_ops.conv2d_dgrad`` / ``conv2d_wgrad_fixed``; ``early_scale``
multiplies ``channel_convert1``'s weight gradient and input gradient; the input gradient is skipped when the input does not require
one (the adapter-training step: the feature map comes from a frozen backbone). ``smoothing`` is not an input of the function and gets
no gradient, as in the reference, whose forward never uses it. A block none of whose parameters requires a gradient runs ``dx_only``.
``ConvFunction`` is ``adapterconv``: the 1x1 adjoints through the crop of ``BaseAdapter``'s zero padding.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib, train_ops
from .runtime import f32c, ptr, require_gpu, stream_ptr, workspaces

LAUNCHES = 6            # kCnxBwdLaunches: prepare, pixel pass, weight pass, depthwise pass, reduce, final
LAUNCHES_DX_ONLY = 3    # kCnxBwdLaunchesDxOnly: prepare, pixel pass, depthwise pass
BLOCK_PARAMS = 9


def workspace_bytes(n, C, H, W, dx_only=False, slabs=0):
    return _lib.check_size(_lib.lib().gencomm_convnext_block_bwd_workspace_bytes(n, C, H, W, int(dx_only), int(slabs)),
                           "gencomm_convnext_block_bwd_workspace_bytes")


def convnext_block_bwd(x, dy, params, dx_only=False, slabs=0, out=None):
    """(dx, grads) of one ConvNeXtBlock: ``x`` the block's input, ``dy`` the gradient of its output (both [n, C, H, W], contiguous
    float32 on the GPU), ``params`` in ``_ConvNeXtBlock.tensors()`` order (gamma may be None). ``grads`` is a list in the same order
    (None for a None gamma), or None with ``dx_only``. ``out`` may be ``dy`` itself; it must not share memory with ``x``."""
    require_gpu(x, "convnext_block_bwd")
    n, C, H, W = x.shape
    if len(params) != BLOCK_PARAMS:
        raise ValueError(f"convnext_block_bwd: {BLOCK_PARAMS} parameters expected, got {len(params)}")
    shapes = [(C, 1, 7, 7), (C,), (C,), (C,), (4 * C, C), (4 * C,), (C, 4 * C), (C,), (C,)]
    dx = torch.empty_like(x) if out is None else out
    for name, t, shape in [("x", x, (n, C, H, W)), ("dy", dy, (n, C, H, W)), ("out", dx, (n, C, H, W))] + \
            [(f"params[{i}]", t, s) for i, (t, s) in enumerate(zip(params, shapes))]:
        if t is None and name == "params[8]":
            continue
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"convnext_block_bwd: {name} must be a contiguous float32 tensor of shape {list(shape)} on {x.device}")
    grads = None
    if not dx_only:
        grads = [None if p is None else torch.empty_like(p) for p in params]
    need = workspace_bytes(n, C, H, W, dx_only, slabs)
    ws = workspaces.get(x.device, need, "convnext_bwd")
    _lib.check(_lib.lib().gencomm_convnext_block_bwd(ptr(x), ptr(dy), *[ptr(p) for p in params], ptr(dx),
                                                     *([0] * BLOCK_PARAMS if dx_only else [ptr(g) for g in grads]), int(dx_only), int(slabs),
                                                     n, C, H, W, ptr(ws), ws.numel(), stream_ptr(x.device)), "gencomm_convnext_block_bwd")
    return dx, grads


def _pick(grads, needs):
    return [g if w else None for g, w in zip(grads, needs)]


class ConvNextFunction(torch.autograd.Function):
    """One call of an ``_AdapterConvNext``: inputs (core, x, convert1.weight, convert1.bias, 9 tensors per block .., convert2.weight,
    convert2.bias)."""

    @staticmethod
    def forward(ctx, core, x, *params):
        from .stamp_adapter import _conv1x1, convnext_block
        dev = x.device
        xin = f32c(x)
        scale = float(core.submodule_args.get("early_scale", 1.0))
        h = _conv1x1(core._cache, "convert1", core.channel_convert1, xin, scale)
        tape, block_params = [], []
        for i, blk in enumerate(core.conv.model):
            src = blk.tensors()
            bp = core._cache.get(("block", i), src, dev, lambda: [None if t is None else f32c(t.detach()) for t in src])
            tape.append(h)
            block_params.append(bp)
            h = convnext_block(h, *bp)
        tape.append(h)
        y = _conv1x1(core._cache, "convert2", core.channel_convert2, h)
        ctx.scale, ctx.blocks = scale, len(block_params)
        flat = [t for bp in block_params for t in bp]
        ctx.gamma_none = [bp[8] is None for bp in block_params]
        ctx.save_for_backward(xin, *tape, f32c(core.channel_convert1.weight.detach()), f32c(core.channel_convert2.weight.detach()),
                              *[t for t in flat if t is not None])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        nb = ctx.blocks
        saved = list(ctx.saved_tensors)
        xin, tape, w_c1, w_c2, rest = saved[0], saved[1:nb + 2], saved[nb + 2], saved[nb + 3], saved[nb + 4:]
        needs = ctx.needs_input_grad   # (core, x, c1.w, c1.b, blocks .., c2.w, c2.b)
        need_x, need_c1 = needs[1], needs[2:4]
        need_blocks = [needs[4 + BLOCK_PARAMS * i:4 + BLOCK_PARAMS * (i + 1)] for i in range(nb)]
        need_c2 = needs[4 + BLOCK_PARAMS * nb:6 + BLOCK_PARAMS * nb]
        out = [None, None] + [None] * (len(needs) - 2)
        g = f32c(g)
        if any(need_c2):
            dw, db = train_ops.conv2d_wgrad_fixed(g, tape[nb], 1, True)
            out[4 + BLOCK_PARAMS * nb:6 + BLOCK_PARAMS * nb] = _pick([dw, db], need_c2)
        upstream = any(need_c1) or need_x or any(any(nbk) for nbk in need_blocks)
        if not upstream:
            return tuple(out)
        dh = train_ops.conv2d_dgrad(g, w_c2, 0)
        # the saved block parameters, None re-inserted where a block has no gamma
        params, k = [], 0
        for i in range(nb):
            take = BLOCK_PARAMS - 1 if ctx.gamma_none[i] else BLOCK_PARAMS
            bp = rest[k:k + take]
            k += take
            params.append(bp + [None] if ctx.gamma_none[i] else bp)
        for i in reversed(range(nb)):
            below = any(need_c1) or need_x or any(any(nbk) for nbk in need_blocks[:i])
            want = any(need_blocks[i])
            if not want and not below:
                break
            dh, grads = convnext_block_bwd(tape[i], dh, params[i], dx_only=not want, out=dh)   # dx takes dy's place
            if want:
                out[4 + BLOCK_PARAMS * i:4 + BLOCK_PARAMS * (i + 1)] = _pick(grads, need_blocks[i])
        if any(need_c1):
            dw, db = train_ops.conv2d_wgrad_fixed(dh, xin, 1, True)
            out[2:4] = _pick([dw * ctx.scale if ctx.scale != 1.0 else dw, db], need_c1)
        if need_x:
            dx = train_ops.conv2d_dgrad(dh, w_c1, 0)
            out[1] = dx * ctx.scale if ctx.scale != 1.0 else dx
        return tuple(out)


class ConvFunction(torch.autograd.Function):
    """One call of an ``_AdapterConv``: inputs (core, x, conv.weight, conv.bias)."""

    @staticmethod
    def forward(ctx, core, x, weight, bias):
        from .stamp_adapter import _conv1x1
        xin = f32c(x)
        y = _conv1x1(core._cache, "conv", core.conv, xin)
        ctx.pad, ctx.hw = core.pad, tuple(y.shape[2:])
        ctx.save_for_backward(xin, f32c(weight.detach()))
        return core._padded(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xin, w = ctx.saved_tensors
        left, _, top, _ = ctx.pad
        H, W = ctx.hw
        g = f32c(f32c(g)[:, :, top:top + H, left:left + W])   # the adjoint of zero padding is the crop
        out = [None, None, None, None]
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dw, db = train_ops.conv2d_wgrad_fixed(g, xin, 1, True)
            out[2:4] = _pick([dw, db], ctx.needs_input_grad[2:4])
        if ctx.needs_input_grad[1]:
            out[1] = train_ops.conv2d_dgrad(g, w, 0)
        return tuple(out)


def run_trainable(core, x):
    """The grad-enabled forward of a trainable module's core (``_AdapterConvNext``, ``_AdapterConv`` or ``_AdapterIdentity``)."""
    from . import stamp_adapter as S
    if isinstance(core, S._AdapterIdentity):
        return x
    if isinstance(core, S._AdapterConv):
        return ConvFunction.apply(core, x, core.conv.weight, core.conv.bias)
    params = [core.channel_convert1.weight, core.channel_convert1.bias]
    for blk in core.conv.model:
        params += blk.tensors()
    params += [core.channel_convert2.weight, core.channel_convert2.bias]
    return ConvNextFunction.apply(core, x, *params)
