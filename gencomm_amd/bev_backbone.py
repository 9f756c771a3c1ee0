"""``BaseBEVBackbone`` / ``DownsampleConv`` / 1x1 heads -- host-side mirrors of the dense 2-D conv stacks
on either side of the hot path:

  BaseBEVBackbone   opencood/models/sub_modules/base_bev_backbone.py:6-156
  DownsampleConv    opencood/models/sub_modules/downsample_conv.py:7-49
  heads             opencood/models/heter_model_baseline_w_gencomm_stage1.py:137-142

The modules own their parameters in the reference's ``nn.Sequential`` layout, so ``state_dict`` keys are
identical (``blocks.0.1.weight``, ``blocks.0.2.running_mean``, ``deblocks.1.0.weight``,
``layers.0.double_conv.2.bias`` ...). ``forward`` never calls the torch layers: every conv (+ folded
eval-mode BatchNorm + ReLU) is one launch of the implicit-GEMM HIP kernel through the C ABI; deblocks write
straight into their channel slice of the concatenated output. In training mode BatchNorm uses batch statistics
(HIP statistics / normalisation kernels, running statistics updated as nn.BatchNorm2d does) and every layer has a HIP backward.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .runtime import conv2d_prepare, f32c, ptr, require_gpu, stream_ptr
from .train_ops import bn_batch_statistics


def _versions(*tensors):
    return tuple((t.data_ptr(), t._version) if t is not None else None for t in tensors)


_SIZES: dict = {}


def _prepared_floats(cin, cout, k, transposed):
    key = ("p", cin, cout, k, transposed)
    if key not in _SIZES:
        _SIZES[key] = _lib.check_size(_lib.lib().gencomm_conv2d_prepared_floats(cin, cout, k, k, transposed), "gencomm_conv2d_prepared_floats")
    return _SIZES[key]


def _wgrad_scratch_floats(n, cin, H, W, cout, k, pad):
    key = ("w", n, cin, H, W, cout, k, pad)
    if key not in _SIZES:
        _SIZES[key] = _lib.check_size(_lib.lib().gencomm_conv2d_wgrad_scratch_floats(n, cin, H, W, cout, k, 1, pad), "gencomm_conv2d_wgrad_scratch_floats")
    return _SIZES[key]


def _conv_backward(x, g, conv, pad, need_x):
    """(dx, {parameter: gradient}) of the bare convolution given d(conv output) on the HIP primitives: nn.Conv2d 1x1 / 3x3 with stride
    1 or 2 (stride 2: dy spread onto the stride-1 grid, then the stride-1 input-gradient kernel), nn.ConvTranspose2d with kernel ==
    stride (pixel-unshuffled dy, 1x1 GEMMs), and the weight gradient of the 7x7 stride-2 pad-3 ResNet stem (no input gradient: raises).
    None when the layer is outside that set."""
    import torch.nn.functional as F
    from . import train_ops as T
    grads = {}
    if isinstance(conv, nn.ConvTranspose2d):
        s = conv.stride[0]
        if conv.kernel_size != (s, s) or conv.stride != (s, s) or conv.padding != (0, 0):
            return None
        cin, cout = conv.weight.shape[:2]
        gu = F.pixel_unshuffle(g, s).contiguous()                                    # [n, cout s^2, H, W], channel = co s^2 + dy s + dx
        wm = conv.weight.detach().reshape(cin, cout * s * s)
        if conv.weight.requires_grad:
            dwt, _ = T.conv2d_wgrad(gu, x, 1, 0, False)                              # [cout s^2, cin, 1, 1]
            grads[conv.weight] = dwt[:, :, 0, 0].t().reshape(cin, cout, s, s)
        if conv.bias is not None and conv.bias.requires_grad:
            grads[conv.bias] = g.sum((0, 2, 3))
        dx = T.conv2d(gu, wm[:, :, None, None], None, 0) if need_x else None          # dx[ci] = sum_j W[ci][j] gu[j]
        return dx, grads
    if (conv.kernel_size == (7, 7) and conv.stride == (2, 2) and (conv.padding[0] if pad is None else pad) == 3 and conv.padding[0] == conv.padding[1]
            and conv.groups == 1 and conv.dilation == (1, 1) and conv.bias is None and conv.in_channels <= 3 and conv.out_channels % 64 == 0):
        # the ResNet stem (7x7 stride 2 pad 3 on the images): weight gradient only -- the images need no gradient
        if need_x:
            raise NotImplementedError(f"input gradient of the 7x7 stride-2 pad-3 stem (Conv2d {conv.in_channels} -> {conv.out_channels}, kernel (7, 7), "
                                      "stride (2, 2)) is not implemented: its input is the image")
        if conv.weight.requires_grad:
            grads[conv.weight] = T.stem7x7_wgrad(g, x, conv.out_channels)
        return None, grads
    if conv.kernel_size not in ((1, 1), (3, 3)) or conv.stride not in ((1, 1), (2, 2)) or conv.groups != 1 or conv.dilation != (1, 1):
        return None
    k, st = conv.kernel_size[0], conv.stride[0]
    p = conv.padding[0] if pad is None else pad
    from .runtime import overlap
    with overlap(x.device, x.shape[0] * x.shape[2] * x.shape[3] if need_x else 0) as ov:   # the weight gradient beside the input gradient
        if conv.weight.requires_grad or (conv.bias is not None and conv.bias.requires_grad):
            dw, db = ov.run(lambda: T.conv2d_wgrad(g, x, k, p, conv.bias is not None, st))
            grads[conv.weight] = dw
            if conv.bias is not None:
                grads[conv.bias] = db
        dx = T.conv2d_dgrad_strided(g, conv.weight, p, st, (x.shape[2], x.shape[3])) if need_x else None
    return dx, grads


def _hip_backward(x, y, gy, conv, bn, relu, pad, need_x):
    """Backward of act(BN_eval(conv(x))) on the HIP primitives; None when the convolution is outside what `_conv_backward` covers."""
    from . import train_ops as T
    g = gy.float().contiguous()
    if relu:
        g = g * (y > 0)
    grads = {}
    if bn is not None:   # eval-mode BatchNorm: y = scale (conv + bias - mean) + beta
        rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
        scale = bn.weight.detach().float() * rstd
        if bn.weight.requires_grad or bn.bias.requires_grad:
            pre = conv2d_hip_raw(x, conv, pad)                                  # the convolution's own output, unfused
            grads[bn.weight] = (g * (pre - bn.running_mean.float().view(1, -1, 1, 1))).sum((0, 2, 3)) * rstd
            grads[bn.bias] = g.sum((0, 2, 3))
        g = g * scale.view(1, -1, 1, 1)
    r = _conv_backward(x, g, conv, pad, need_x)
    if r is None:
        return None
    dx, cg = r
    grads.update(cg)
    return dx, grads


def conv2d_hip_raw(x, conv, pad):
    """The bare convolution (bias included, no norm, no activation) on the HIP kernel, without touching autograd."""
    with torch.no_grad():
        return conv2d_hip(x.detach(), conv, None, relu=False, pad=pad)


class _ConvBnTrainFn(torch.autograd.Function):
    """act(BatchNorm2d_batch(conv(x))) in TRAINING mode (stage 1 trains the backbone: base_bev_backbone.py:40-92): HIP convolution,
    HIP batch statistics / normalisation (running statistics updated as nn.BatchNorm2d does), HIP backward (BatchNorm backward
    kernels, then the convolution's dgrad / wgrad)."""

    @staticmethod
    def _fusable(conv, bn, x) -> bool:
        """one foreign call per direction (gencomm_convbn_train_fwd / _bwd): plain square 1x1 / 3x3 Conv2d, stride 1 | 2, fp32 contiguous input,
        momentum-style running statistics with the counter on the device"""
        if not (isinstance(conv, nn.Conv2d) and conv.kernel_size in ((1, 1), (3, 3)) and conv.stride in ((1, 1), (2, 2)) and conv.groups == 1
                and conv.dilation == (1, 1) and conv.padding[0] == conv.padding[1]):
            return False
        if x.dtype != torch.float32 or not x.is_contiguous() or conv.weight.dtype != torch.float32 or bn.weight is None or bn.momentum is None:
            return False
        nbt = bn.num_batches_tracked
        return (not bn.track_running_stats) or (bn.running_mean is not None and nbt is not None and nbt.is_cuda and nbt.dtype == torch.int64)

    @staticmethod
    def forward(ctx, x, conv, bn, relu, pad, *params):
        from . import train_ops as T
        ctx.conv, ctx.bn, ctx.relu, ctx.pad = conv, bn, relu, pad
        if _ConvBnTrainFn._fusable(conv, bn, x):
            from .runtime import zeros as pool_zeros
            w = conv.weight.detach().contiguous()
            cout, cin, k, _ = w.shape
            n, _, H, W = x.shape
            st_, p = conv.stride[0], conv.padding[0] if pad is None else pad
            Ho, Wo = (H + 2 * p - k) // st_ + 1, (W + 2 * p - k) // st_ + 1
            l, dev = _lib.lib(), x.device
            unit = T._unit_scale_shift(cout, dev)
            prepared = torch.empty(_prepared_floats(cin, cout, k, 0), dtype=torch.float32, device=dev)
            pre = torch.empty(n, cout, Ho, Wo, dtype=torch.float32, device=dev)
            y = torch.empty_like(pre)
            save = torch.empty(cout, 2, dtype=torch.float32, device=dev)
            scratch = pool_zeros(2 * cout, torch.float64, dev)
            T.check_batch_size(n * Ho * Wo, pre.shape)
            track, momentum, nbt = T.bn_train_update(bn)         # _fusable: momentum set, the counter (if any) on the device
            b = conv.bias.detach().contiguous() if conv.bias is not None else None
            _lib.check(l.gencomm_convbn_train_fwd(ptr(x), ptr(w), ptr(b), ptr(unit[0]), ptr(unit[1]), ptr(bn.weight.detach()), ptr(bn.bias.detach()),
                                                  ptr(bn.running_mean) if track else 0, ptr(bn.running_var) if track else 0,
                                                  ptr(nbt), momentum, float(bn.eps), int(relu),
                                                  ptr(prepared), ptr(pre), ptr(y), ptr(save), ptr(scratch), n, cin, H, W, cout, k, st_, p,
                                                  stream_ptr(dev)), "gencomm_convbn_train_fwd")
            ctx.save_for_backward(x, pre, y, save)
            return y
        pre = conv2d_hip_raw(x, conv, pad)
        with torch.no_grad():
            y, save = T.bn2d_train_fwd(pre, bn, relu)
        ctx.save_for_backward(x, pre, y, save)
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import train_ops as T
        x, pre, y, save = ctx.saved_tensors
        conv, bn = ctx.conv, ctx.bn
        params = [p for p in (conv.weight, conv.bias, bn.weight, bn.bias) if p is not None]
        from .runtime import SIDE_MIN_PIXELS, zeros as pool_zeros
        mode = _lib.lib().gencomm_get_mode(_lib.MODE_BWD_STREAMS)
        side = ctx.needs_input_grad[0] and (mode == 2 or (mode == 1 and x.shape[0] * x.shape[2] * x.shape[3] >= SIDE_MIN_PIXELS))
        if (_ConvBnTrainFn._fusable(conv, bn, x) and conv.stride == (1, 1) and not side and gy.dtype == torch.float32
                and conv.weight.requires_grad and bn.weight.requires_grad and bn.bias.requires_grad and (conv.bias is None or conv.bias.requires_grad)):
            # stride 1, no side stream wanted for this map size: BatchNorm backward + weight gradient + input gradient as ONE foreign call
            w = conv.weight.detach().contiguous()
            cout, cin, k, _ = w.shape
            n, _, H, W = x.shape
            p = conv.padding[0] if ctx.pad is None else ctx.pad
            l, dev = _lib.lib(), x.device
            gyc = gy.contiguous()
            unit = T._unit_scale_shift(cin, dev)
            need_x = bool(ctx.needs_input_grad[0])
            dpre = torch.empty_like(pre)
            dx = torch.empty_like(x) if need_x else None
            blob = pool_zeros(cout * cin * k * k + (cout if conv.bias is not None else 0), torch.float32, dev)
            dw = blob[:cout * cin * k * k].view(cout, cin, k, k)
            dbias = blob[cout * cin * k * k:] if conv.bias is not None else None
            dg, db = torch.empty(2, cout, dtype=torch.float32, device=dev).unbind(0)
            scratch = pool_zeros(2 * cout, torch.float64, dev)
            prepared = torch.empty(_prepared_floats(cout, cin, k, 2), dtype=torch.float32, device=dev) if need_x else None
            need = _wgrad_scratch_floats(n, cin, H, W, cout, k, p)
            wscr = torch.empty(need, dtype=torch.float32, device=dev) if need else None
            _lib.check(l.gencomm_convbn_train_bwd(ptr(x), ptr(w), ptr(pre), ptr(y), ptr(gyc), ptr(save), ptr(bn.weight.detach()), ptr(unit[0]), ptr(unit[1]),
                                                  int(ctx.relu), ptr(dpre), ptr(dx), ptr(dw), ptr(dbias), ptr(dg), ptr(db), ptr(scratch), ptr(prepared),
                                                  ptr(wscr), need, n, cin, H, W, cout, k, p, stream_ptr(dev)), "gencomm_convbn_train_bwd")
            grads = {conv.weight: dw, bn.weight: dg, bn.bias: db}
            if conv.bias is not None:
                grads[conv.bias] = dbias
            return (dx, None, None, None, None, *[grads.get(q) if q.requires_grad else None for q in params])
        with torch.no_grad():
            dpre, dg, db = T.bn2d_train_bwd(pre, y, gy.float().contiguous(), save, bn.weight, ctx.relu)
            r = _conv_backward(x.detach().float().contiguous(), dpre, conv, ctx.pad, ctx.needs_input_grad[0])
        if r is None:
            raise NotImplementedError("training this convolution shape on the HIP path is not implemented")
        dx, grads = r
        grads[bn.weight], grads[bn.bias] = dg, db
        return (dx, None, None, None, None, *[grads.get(p) if p.requires_grad else None for p in params])


class _Conv2dHipFn(torch.autograd.Function):
    """act(BN_eval(conv(x))) with gradients: HIP forward; HIP backward (dgrad / wgrad kernels; stride-2 and transposed convolutions
    included); a shape the HIP backward does not cover raises (no torch / MIOpen fallback).
    Gradients reach the input and the conv / BatchNorm-affine parameters: the graph is never cut."""

    @staticmethod
    def forward(ctx, x, conv, bn, relu, pad, *params):
        ctx.conv, ctx.bn, ctx.relu, ctx.pad = conv, bn, relu, pad
        with torch.no_grad():
            y = conv2d_hip(x, conv, bn, relu=relu, pad=pad)
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        params = [p for p in (ctx.conv.weight, ctx.conv.bias) + ((ctx.bn.weight, ctx.bn.bias) if ctx.bn is not None else ()) if p is not None]
        with torch.no_grad():
            hip = _hip_backward(x.detach().float().contiguous(), y, gy, ctx.conv, ctx.bn, ctx.relu, ctx.pad, ctx.needs_input_grad[0])
        if hip is not None:
            dx, grads = hip
            return (dx, None, None, None, None, *[grads.get(p) if p.requires_grad else None for p in params])
        # no torch / MIOpen fallback in the product path: a layer shape the HIP backward does not cover is an error
        raise NotImplementedError(
            f"HIP backward of this convolution is not implemented ({type(ctx.conv).__name__} kernel {tuple(ctx.conv.kernel_size)} stride "
            f"{tuple(ctx.conv.stride)}); covered: 1x1 / 3x3 stride 1, 3x3 stride 2, ConvTranspose2d with kernel == stride")


def _stride1_view(conv: nn.Conv2d) -> nn.Conv2d:
    """A 1x1 convolution with stride s reads every s-th pixel: the same layer with stride 1 on the subsampled input. The shadow module
    shares the Parameter objects (gradients land on the original) and is cached on it."""
    sh = getattr(conv, "_gc_stride1", None)
    if sh is None or sh.weight is not conv.weight or sh.bias is not conv.bias:
        sh = nn.Conv2d(conv.in_channels, conv.out_channels, 1, stride=1, bias=conv.bias is not None)
        sh.weight, sh.bias = conv.weight, conv.bias
        object.__setattr__(conv, "_gc_stride1", sh)
    return sh


def conv2d_hip(x: torch.Tensor, conv: nn.Module, bn: Optional[nn.BatchNorm2d] = None, relu: bool = False,
               pad: Optional[int] = None, out: Optional[torch.Tensor] = None, out_coff: int = 0,
               residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(BN(conv(x))) as one HIP launch. ``conv`` is an ``nn.Conv2d`` (3x3 stride 1|2, or 1x1) or an
    ``nn.ConvTranspose2d`` whose kernel equals its stride; ``pad`` overrides ``conv.padding`` (ZeroPad2d(1)
    in front of a padding-0 conv). ``out``/``out_coff``: write into a channel slice of a larger tensor.
    With gradients enabled and anything differentiable among the input and the layer's parameters the call goes
    through ``_Conv2dHipFn`` (eval-mode BatchNorm) or ``_ConvBnTrainFn`` (batch statistics), HIP forward and HIP backward: the graph
    is never cut silently."""
    require_gpu(x, "conv2d_hip")
    if isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride[0] > 1 and conv.stride[0] == conv.stride[1]:
        s_ = conv.stride[0]
        return conv2d_hip(x[:, :, ::s_, ::s_].contiguous(), _stride1_view(conv), bn, relu, pad, out, out_coff, residual)
    if residual is not None:
        # `residual` is added to BN(conv(x)) and the ReLU (if any) comes AFTER the sum (ResNet BasicBlock, resblock.py:48-62)
        grad_path = torch.is_grad_enabled() and (x.requires_grad or residual.requires_grad or any(
            p is not None and p.requires_grad for p in (conv.weight, conv.bias) + ((bn.weight, bn.bias) if bn is not None else ())))
        if grad_path or (bn is not None and bn_batch_statistics(bn)) or out is not None:
            y = conv2d_hip(x, conv, bn, False, pad) + residual
            return torch.relu(y) if relu else y
    if torch.is_grad_enabled():
        params = [p for p in (conv.weight, conv.bias) + ((bn.weight, bn.bias) if bn is not None else ()) if p is not None]
        if x.requires_grad or any(p.requires_grad for p in params):
            fn = _ConvBnTrainFn if (bn is not None and bn_batch_statistics(bn)) else _Conv2dHipFn
            y = fn.apply(x, conv, bn, relu, pad, *params)
            if out is None:
                return y
            out[:, out_coff:out_coff + y.shape[1]] = y  # differentiable slice assignment (training only)
            return out
    x = f32c(x)
    transposed = isinstance(conv, nn.ConvTranspose2d)
    w = conv.weight
    if transposed:
        cin, cout, kh, kw = w.shape
        s = conv.stride[0]
        if not (kh == kw == s == conv.stride[1]) or conv.padding != (0, 0) or conv.output_padding != (0, 0):
            raise NotImplementedError("ConvTranspose2d is supported with kernel == stride, no padding")
        stride, p, ups, gkh, gkw = 1, 0, s, 1, 1
    else:
        cout, cin, kh, kw = w.shape
        if conv.groups != 1 or conv.dilation != (1, 1) or conv.stride[0] != conv.stride[1] or conv.padding[0] != conv.padding[1]:
            raise NotImplementedError("grouped / dilated / anisotropic Conv2d is not supported")
        stride, ups, gkh, gkw = conv.stride[0], 1, kh, kw
        p = conv.padding[0] if pad is None else pad
    if bn is not None and bn_batch_statistics(bn):   # batch statistics without gradients (e.g. a training-mode forward under no_grad)
        from . import train_ops as T
        y, _ = T.bn2d_train_fwd(conv2d_hip(x, conv, None, relu=False, pad=pad), bn, relu)
        if out is None:
            return y
        out[:, out_coff:out_coff + y.shape[1]] = y
        return out
    n, c, H, W = x.shape
    if c != cin:
        raise ValueError(f"expected {cin} input channels, got {c}")
    l = _lib.lib()
    st = stream_ptr(x.device)
    bnp = (bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else (None,) * 4
    # num_batches_tracked is part of the key: the HIP training kernels update running_mean / running_var through raw pointers, which
    # does not bump those tensors' versions -- the counter is incremented by a torch op on the same paths (train_ops.bn2d_train_fwd)
    key = _versions(w, conv.bias, *bnp, getattr(bn, "num_batches_tracked", None)) + (str(x.device),)
    cache = getattr(conv, "_gc_cache", None)
    if cache is None or cache[0] != key:
        wd = f32c(w.detach())
        prepared = conv2d_prepare(wd, cin, cout, kh, kw, int(transposed), x.device)
        b = f32c(conv.bias.detach()) if conv.bias is not None else None
        if bn is None:   # scale 1, shift = bias: nothing to fold -- a cached unit row and the bias itself (training re-prepares every step)
            from .train_ops import _unit_scale_shift
            unit = _unit_scale_shift(cout, x.device)
            ss = (unit[0], b if b is not None else unit[1])
        else:
            ss = torch.empty(2, cout, dtype=torch.float32, device=x.device)
            d = [f32c(t.detach()) if t is not None else None for t in bnp]
            _lib.check(l.gencomm_conv2d_fold(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(b), float(bn.eps), cout, ptr(ss[0]), ptr(ss[1]), st),
                       "gencomm_conv2d_fold")
        cache = (key, prepared, ss)
        conv._gc_cache = cache
    _, prepared, ss = cache
    Ho = ((H + 2 * p - gkh) // stride + 1) * ups
    Wo = ((W + 2 * p - gkw) // stride + 1) * ups
    if out is None:
        out = torch.empty(n, cout, Ho, Wo, dtype=torch.float32, device=x.device)
        out_coff = 0
    if tuple(out.shape[2:]) != (Ho, Wo) or out.shape[0] != n or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError(f"output buffer must be contiguous f32 [n, *, {Ho}, {Wo}], got {tuple(out.shape)}")
    if residual is not None:   # inference: conv + folded BatchNorm + identity + ReLU in one launch
        res = f32c(residual)
        if tuple(res.shape) != (n, cout, Ho, Wo) or ups != 1:
            raise ValueError(f"residual must be [n, {cout}, {Ho}, {Wo}], got {tuple(res.shape)}")
        _lib.check(l.gencomm_conv2d_act_res_fwd(ptr(x), ptr(prepared), ptr(ss[0]), ptr(ss[1]), ptr(res), ptr(out), n, cin, H, W, cout, gkh, gkw,
                                                stride, p, 3 if relu else 0, st), "gencomm_conv2d_act_res_fwd")
        return out
    _lib.check(l.gencomm_conv2d_fwd(ptr(x), ptr(prepared), ptr(ss[0]), ptr(ss[1]), ptr(out), n, cin, H, W, cout, gkh, gkw,
                                    stride, p, int(relu), ups, out.shape[1], out_coff, st), "gencomm_conv2d_fwd")
    return out


GCONV_GROUPS = 32
GCONV_WIDTHS = (4, 8, 16)


def gconv3x3_check(conv: nn.Module) -> int:
    """Channels per group of a grouped 3x3 layer the HIP kernel covers (Conv2d(C, C, 3, padding=1, groups=32), 4 / 8 / 16 channels
    per group, stride 1 | 2); anything else raises naming it. No device is needed for the check."""
    if not isinstance(conv, nn.Conv2d) or conv.kernel_size != (3, 3) or conv.padding != (1, 1) or conv.dilation != (1, 1) \
            or conv.stride not in ((1, 1), (2, 2)) or conv.padding_mode != "zeros":
        raise NotImplementedError(f"grouped convolution: only Conv2d 3x3, padding 1, dilation 1, stride 1 | 2 is built (got {conv})")
    cpg = conv.in_channels // conv.groups
    if conv.groups != GCONV_GROUPS or cpg not in GCONV_WIDTHS or conv.in_channels != conv.groups * cpg:
        raise NotImplementedError(f"grouped convolution: unsupported group width ({conv.groups} groups x {conv.in_channels / conv.groups:g} "
                                  f"channels; built: {GCONV_GROUPS} groups x {GCONV_WIDTHS} channels)")
    if conv.out_channels != conv.in_channels:
        raise NotImplementedError(f"grouped convolution: C_in != C_out ({conv.in_channels} -> {conv.out_channels}) is not built")
    return cpg


def gconv3x3_hip(x: torch.Tensor, conv: nn.Conv2d, bn: Optional[nn.BatchNorm2d] = None, relu: bool = False,
                 trainable: bool = False) -> torch.Tensor:
    """act(BN(conv(x))) for the grouped 3x3 of the ResNeXt ``Bottleneck`` as one launch of ``gencomm_gconv3x3_fwd``: the same
    per-module cache of the prepared weight and the folded BatchNorm as ``conv2d_hip``. By default inference only: batch statistics and
    gradients through this layer raise. ``trainable=True`` opts in to both (``pyramid_bwd.GconvEvalFn`` / ``GconvBnTrainFn``, chosen by
    ``bn_batch_statistics(bn)`` as ``conv2d_hip`` chooses); under ``no_grad`` with eval-mode BatchNorm it is the launch below."""
    cpg = gconv3x3_check(conv)
    params = [p for p in (conv.weight, conv.bias) + ((bn.weight, bn.bias) if bn is not None else ()) if p is not None]
    grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    stats = bn is not None and bn_batch_statistics(bn)
    if trainable:
        require_gpu(x, "gconv3x3_hip")
        if conv.bias is not None:
            raise NotImplementedError("grouped convolution: training a layer with a conv bias is not built (no layer of the pyramid has one)")
        if grad or stats:
            from .pyramid_bwd import gconv3x3_train
            return gconv3x3_train(x, conv, bn, relu, cpg, grad, stats)
    if grad:
        raise NotImplementedError("grouped convolution: the backward is not built (pyramid training is a later change)")
    if stats:
        raise NotImplementedError("grouped convolution: BatchNorm batch statistics (train() mode) are not built")
    require_gpu(x, "gconv3x3_hip")
    x = f32c(x)
    n, c, H, W = x.shape
    if c != conv.in_channels:
        raise ValueError(f"expected {conv.in_channels} input channels, got {c}")
    l, st, w = _lib.lib(), stream_ptr(x.device), conv.weight
    bnp = (bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else (None,) * 4
    key = _versions(w, conv.bias, *bnp, getattr(bn, "num_batches_tracked", None)) + (str(x.device),)
    cache = getattr(conv, "_gc_cache", None)
    if cache is None or cache[0] != key:
        packed = torch.empty(w.numel(), dtype=torch.float32, device=x.device)
        _lib.check(l.gencomm_gconv3x3_prepare(ptr(f32c(w.detach())), ptr(packed), cpg, st), "gencomm_gconv3x3_prepare")
        b = f32c(conv.bias.detach()) if conv.bias is not None else None
        if bn is None:
            from .train_ops import _unit_scale_shift
            unit = _unit_scale_shift(c, x.device)
            ss = (unit[0], b if b is not None else unit[1])
        else:
            ss = torch.empty(2, c, dtype=torch.float32, device=x.device)
            d = [f32c(t.detach()) if t is not None else None for t in bnp]
            _lib.check(l.gencomm_conv2d_fold(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(b), float(bn.eps), c, ptr(ss[0]), ptr(ss[1]), st),
                       "gencomm_conv2d_fold")
        cache = (key, packed, ss)
        conv._gc_cache = cache
    _, packed, ss = cache
    s = conv.stride[0]
    out = torch.empty(n, c, (H - 1) // s + 1, (W - 1) // s + 1, dtype=torch.float32, device=x.device)
    _lib.check(l.gencomm_gconv3x3_fwd(ptr(x), ptr(packed), ptr(ss[0]), ptr(ss[1]), ptr(out), n, c, cpg, H, W, s, int(relu), st), "gencomm_gconv3x3_fwd")
    return out


class BaseBEVBackbone(nn.Module):
    """Constructor mirrors base_bev_backbone.py:7-92 (same Sequential indices => same checkpoint keys)."""

    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        if 'layer_nums' in model_cfg:
            assert len(model_cfg['layer_nums']) == len(model_cfg['layer_strides']) == len(model_cfg['num_filters'])
            layer_nums, layer_strides, num_filters = model_cfg['layer_nums'], model_cfg['layer_strides'], model_cfg['num_filters']
        else:
            layer_nums = layer_strides = num_filters = []
        if 'upsample_strides' in model_cfg:
            assert len(model_cfg['upsample_strides']) == len(model_cfg['num_upsample_filter'])
            num_upsample_filters, upsample_strides = model_cfg['num_upsample_filter'], model_cfg['upsample_strides']
        else:
            upsample_strides = num_upsample_filters = []
        num_levels = len(layer_nums)
        self.num_levels = num_levels
        c_in_list = [input_channels, *num_filters[:-1]]
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(num_levels):
            cur = [nn.ZeroPad2d(1),
                   nn.Conv2d(c_in_list[idx], num_filters[idx], kernel_size=3, stride=layer_strides[idx], padding=0, bias=False),
                   nn.BatchNorm2d(num_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()]
            for _ in range(layer_nums[idx]):
                cur.extend([nn.Conv2d(num_filters[idx], num_filters[idx], kernel_size=3, padding=1, bias=False),
                            nn.BatchNorm2d(num_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()])
            self.blocks.append(nn.Sequential(*cur))
            if len(upsample_strides) > 0:
                stride = upsample_strides[idx]
                if stride >= 1:
                    self.deblocks.append(nn.Sequential(
                        nn.ConvTranspose2d(num_filters[idx], num_upsample_filters[idx], upsample_strides[idx],
                                           stride=upsample_strides[idx], bias=False),
                        nn.BatchNorm2d(num_upsample_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()))
                else:
                    stride = int(np.round(1 / stride))
                    self.deblocks.append(nn.Sequential(
                        nn.Conv2d(num_filters[idx], num_upsample_filters[idx], stride, stride=stride, bias=False),
                        nn.BatchNorm2d(num_upsample_filters[idx], eps=1e-3, momentum=0.01), nn.ReLU()))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > num_levels:
            self.deblocks.append(nn.Sequential(
                nn.ConvTranspose2d(c_in, c_in, upsample_strides[-1], stride=upsample_strides[-1], bias=False),
                nn.BatchNorm2d(c_in, eps=1e-3, momentum=0.01), nn.ReLU()))
        self.num_bev_features = c_in

    # ---- HIP path
    @staticmethod
    def _run_block(seq: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
        mods = list(seq)
        x = conv2d_hip(x, mods[1], mods[2], relu=True, pad=1)  # ZeroPad2d(1) + padding-0 conv
        for j in range(4, len(mods), 3):
            x = conv2d_hip(x, mods[j], mods[j + 1], relu=True)
        return x

    @staticmethod
    def _run_deblock(seq: nn.Sequential, x: torch.Tensor, out=None, coff=0) -> torch.Tensor:
        conv, bn = seq[0], seq[1]
        if isinstance(conv, nn.Conv2d) and conv.kernel_size != (1, 1):
            raise NotImplementedError("deblocks with upsample_stride < 1 (strided k x k conv) are not supported")
        return conv2d_hip(x, conv, bn, relu=True, out=out, out_coff=coff)

    def _decode(self, feats):
        if len(self.deblocks) == 0:
            ups = list(feats)
            x = torch.cat(ups, dim=1) if len(ups) > 1 else ups[0]
        else:
            chans = [seq[1].num_features for seq in list(self.deblocks)[:len(feats)]]
            s0 = self.deblocks[0][0].stride[0] if isinstance(self.deblocks[0][0], nn.ConvTranspose2d) else 1
            n, _, h0, w0 = feats[0].shape
            if torch.is_grad_enabled():
                # gradient path: ONE concatenation whose backward hands out views.  Writing each deblock into its slice of a shared
                # buffer is a differentiable slice assignment per deblock, and the backward of each of those clones the WHOLE 201-MB
                # gradient of the concat and zero-fills a slice of it (three clones + three fills per step on the stage-1 leg)
                x = torch.cat([self._run_deblock(self.deblocks[i], f) for i, f in enumerate(feats)], dim=1)
            else:
                x = torch.empty(n, sum(chans), h0 * s0, w0 * s0, dtype=torch.float32, device=feats[0].device)
                off = 0
                for i, f in enumerate(feats):
                    self._run_deblock(self.deblocks[i], f, out=x, coff=off)  # writes its slice of the concat
                    off += chans[i]
        if len(self.deblocks) > len(self.blocks):
            x = self._run_deblock(self.deblocks[-1], x)
        return x

    def forward(self, data_dict):
        spatial_features = data_dict['spatial_features']
        x = spatial_features
        feats = []
        for i in range(len(self.blocks)):
            x = self._run_block(self.blocks[i], x)
            feats.append(x)  # (the reference's per-stride entries go to a local dict that is dropped, :100-108)
        data_dict['spatial_features_2d'] = self._decode(feats)
        return data_dict

    def get_multiscale_feature(self, spatial_features):
        feats, x = [], spatial_features
        for i in range(len(self.blocks)):
            x = self._run_block(self.blocks[i], x)
            feats.append(x)
        return feats

    def decode_multiscale_feature(self, x):
        return self._decode(list(x)[:self.num_levels])


class DoubleConv(nn.Module):  # downsample_conv.py:7-27
    def __init__(self, in_channels, out_channels, kernel_size, stride, padding):
        super().__init__()
        self.double_conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, stride=stride, padding=padding),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, kernel_size=3, padding=1),
            nn.ReLU(inplace=True))

    def forward(self, x):
        x = conv2d_hip(x, self.double_conv[0], None, relu=True)
        return conv2d_hip(x, self.double_conv[2], None, relu=True)


class DownsampleConv(nn.Module):  # downsample_conv.py:30-49 ('kernal_size' is the reference's spelling)
    def __init__(self, config):
        super().__init__()
        self.layers = nn.ModuleList([])
        input_dim = config['input_dim']
        for (ksize, dim, stride, padding) in zip(config['kernal_size'], config['dim'], config['stride'], config['padding']):
            self.layers.append(DoubleConv(input_dim, dim, kernel_size=ksize, stride=stride, padding=padding))
            input_dim = dim

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


class NaiveCompressor(nn.Module):
    """opencood/models/sub_modules/naive_compress.py:5-35 (channel squeeze / expand, three conv3x3 + BN + ReLU); eval-mode
    BatchNorm only. `compress_raito` is the reference's spelling."""

    def __init__(self, input_dim, compress_raito):
        super().__init__()
        mid = input_dim // compress_raito
        self.encoder = nn.Sequential(nn.Conv2d(input_dim, mid, kernel_size=3, stride=1, padding=1),
                                     nn.BatchNorm2d(mid, eps=1e-3, momentum=0.01), nn.ReLU())
        self.decoder = nn.Sequential(nn.Conv2d(mid, input_dim, kernel_size=3, stride=1, padding=1),
                                     nn.BatchNorm2d(input_dim, eps=1e-3, momentum=0.01), nn.ReLU(),
                                     nn.Conv2d(input_dim, input_dim, kernel_size=3, stride=1, padding=1),
                                     nn.BatchNorm2d(input_dim, eps=1e-3, momentum=0.01), nn.ReLU())

    def forward(self, x):
        x = conv2d_hip(x, self.encoder[0], self.encoder[1], relu=True)
        x = conv2d_hip(x, self.decoder[0], self.decoder[1], relu=True)
        return conv2d_hip(x, self.decoder[3], self.decoder[4], relu=True)


class HipConv2d(nn.Conv2d):
    """``nn.Conv2d`` whose forward is the HIP kernel (detection heads: 1x1, bias, no activation)."""

    def forward(self, x):
        return conv2d_hip(x, self, None, relu=False)
