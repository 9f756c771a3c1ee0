"""STAMP's adapter and reverter (opencood/models/stamp_modules/adapter.py:759-804) on a fused ConvNeXt-block HIP kernel.

In STAMP every non-protocol agent pushes its BEV map through an ``Adapter`` into the protocol feature space and every receiver pulls it
back through a ``Reverter``; both are built from the same constructor dict, ``{"core_method": ..., "args": {...}}``. This module is the
component; the baseline's shell and its ``adapter_loss`` criterion are not here.

Training is opt-in: ``Adapter(args, trainable=True)`` / ``Reverter(args, trainable=True)`` send a grad-enabled call that has something
to differentiate through ONE ``torch.autograd.Function`` per call (``convnext_bwd.py``): the same forward launches and bits, a tape of
the module input and ``num_of_blocks + 1`` maps of ``[n, dim, H, W]``, and per block the six launches of ``gencomm_convnext_block_bwd``
(csrc/convnext_bwd_kernels.h), which recompute the hidden tensor tile by tile instead of keeping it. The default constructors refuse a
grad-enabled call as before; under ``torch.no_grad()``, or with nothing to differentiate, both run the inference path. ``smoothing``
gets no gradient (the reference's forward never uses it). The ``state_dict`` is the same either way.

``core_method``:

``adapterconvnext``  (AdapterConvNext, adapter.py:120-144) ``1x1 conv -> num_of_blocks ConvNeXt blocks -> 1x1 conv``. The two 1x1
                     convolutions run on ``gencomm_conv2d_fwd`` (``early_scale`` rides in that entry's per-channel ``scale``, the bias in
                     ``shift``: ``conv(s x) + b = s conv(x) + b``); each block is ONE launch of ``gencomm_convnext_block_fwd``
                     (csrc/convnext_kernels.h: depthwise 7x7, LayerNorm, Linear, GELU, Linear, layer scale and residual, the
                     ``[pixels, 4 dim]`` hidden tensor never in memory), ping-ponging two buffers. ``dim`` 64 | 128.
``identity``         (AdapterIdentity) returns its input: with equal channels and feature ratio 1 -- every shipped use -- the reference's
                     trilinear resize is the identity bit for bit.
``adapterconv``      (AdapterConv) the 1x1 convolution on the same entry, then ``BaseAdapter``'s zero padding.
``adapterfc`` / ``adapterdsa`` / ``adapteratt``  are not implemented and say so.

The ``state_dict`` has the reference's keys and shapes (33 per ``adapterconvnext`` module, under ``adapter.`` / ``reverter.``; the
``smoothing`` convolution is created and never used by the reference's forward -- it is kept so that a checkpoint loads with
``strict=True``). ``BaseAdapter``'s range and shape arithmetic (adapter.py:62-92) is restated; a configuration whose feature ratio is not
(1, 1) would need the bilinear resize and is refused (no shipped yaml resizes; at ratio 1 ``nn.Upsample`` is the identity, so
``late_upsample`` changes nothing).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .runtime import conv2d_prepare, f32c, ptr, require_gpu, stream_ptr

BLOCK_DIMS = (64, 128)
NOT_IMPLEMENTED = ("adapterfc", "adapterdsa", "adapteratt")


def _versions(*tensors):
    return tuple(None if t is None else (t.data_ptr(), t._version) for t in tensors)


class _Cache:
    """Kernel-side copies of parameters, rebuilt only when a source parameter's storage or version counter changed."""

    def __init__(self):
        self._hit = {}

    def get(self, key, sources, device, make):
        ver = _versions(*sources) + (str(device),)
        hit = self._hit.get(key)
        if hit is None or hit[0] != ver:
            with torch.no_grad():
                hit = self._hit[key] = (ver, make())
        return hit[1]


def _conv1x1(cache, key, conv, x, scale=1.0):
    """conv(scale * x) of an nn.Conv2d(kernel_size=1) as scale * (W x) + bias on gencomm_conv2d_fwd (x: contiguous float32)."""
    dev = x.device

    def make():
        w = f32c(conv.weight.detach())
        cout, cin = w.shape[:2]
        prepared = conv2d_prepare(w, cin, cout, 1, 1, 0, dev)
        ss = torch.empty(2, cout, dtype=torch.float32, device=dev)
        bias = f32c(conv.bias.detach()) if conv.bias is not None else None
        _lib.check(_lib.lib().gencomm_conv2d_fold(None, None, None, None, ptr(bias), 0.0, cout, ptr(ss[0]), ptr(ss[1]), stream_ptr(dev)),
                   "gencomm_conv2d_fold")
        if scale != 1.0:
            ss[0].mul_(float(scale))
        return prepared, ss, cin, cout

    prepared, ss, cin, cout = cache.get(key, [conv.weight, conv.bias], dev, make)
    n, c, H, W = x.shape
    if c != cin:
        raise ValueError(f"stamp adapter: input has {c} channels, the module was built with in_channels {cin}")
    y = torch.empty(n, cout, H, W, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().gencomm_conv2d_fwd(ptr(x), ptr(prepared), ptr(ss[0]), ptr(ss[1]), ptr(y), n, cin, H, W, cout, 1, 1, 1, 0, 0, 1, cout, 0,
                                             stream_ptr(dev)), "gencomm_conv2d_fwd")
    return y


def convnext_block(x, dw_weight, dw_bias, ln_weight, ln_bias, w1, b1, w2, b2, gamma, out=None):
    """One ConvNeXtBlock over x [n, C, H, W] (contiguous float32 on the GPU) in one launch; the parameters as the reference stores them
    (``dwconv.weight [C, 1, 7, 7]``, ``pwconv1.weight [4 C, C]``, ``pwconv2.weight [C, 4 C]``), ``gamma`` None where the reference has
    none. ``out`` must not share memory with ``x``."""
    require_gpu(x, "convnext_block")
    n, C, H, W = x.shape
    y = torch.empty_like(x) if out is None else out
    shapes = {"dwconv.weight": (dw_weight, (C, 1, 7, 7)), "dwconv.bias": (dw_bias, (C,)), "norm.weight": (ln_weight, (C,)), "norm.bias": (ln_bias, (C,)),
              "pwconv1.weight": (w1, (4 * C, C)), "pwconv1.bias": (b1, (4 * C,)), "pwconv2.weight": (w2, (C, 4 * C)), "pwconv2.bias": (b2, (C,)),
              "gamma": (gamma, (C,)), "x": (x, (n, C, H, W)), "out": (y, (n, C, H, W))}
    for name, (t, shape) in shapes.items():   # the kernel trusts these extents
        if t is None and name == "gamma":
            continue
        if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"convnext_block: {name} must be a contiguous float32 tensor of shape {list(shape)} on {x.device}")
    _lib.check(_lib.lib().gencomm_convnext_block_fwd(ptr(x), ptr(dw_weight), ptr(dw_bias), ptr(ln_weight), ptr(ln_bias), ptr(w1), ptr(b1), ptr(w2),
                                                     ptr(b2), ptr(gamma), ptr(y), n, C, H, W, stream_ptr(x.device)), "gencomm_convnext_block_fwd")
    return y


# ----------------------------------------------------------------------------------------- parameter containers (the reference's tree)
class _ConvNeXtBlock(nn.Module):     # feature_alignnet_modules.py:317-330
    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(1e-6 * torch.ones(dim))

    def tensors(self):
        return [self.dwconv.weight, self.dwconv.bias, self.norm.weight, self.norm.bias, self.pwconv1.weight, self.pwconv1.bias,
                self.pwconv2.weight, self.pwconv2.bias, self.gamma]


class _ConvNeXt(nn.Module):          # feature_alignnet_modules.py:350-364
    def __init__(self, args):
        super().__init__()
        dim, blocks = int(args["dim"]), int(args["num_of_blocks"])
        if args.get("kernel_size", 7) != 7:
            raise NotImplementedError(f"stamp adapter: submodule_args.kernel_size {args['kernel_size']} is not supported (the fused block "
                                      "kernel is the 7x7 one; no shipped yaml sets kernel_size)")
        if args.get("deform", False):
            raise NotImplementedError("stamp adapter: submodule_args.deform is not supported (mmcv's DeformConv2dPack in front of every "
                                      "block; no shipped yaml sets deform)")
        if dim not in BLOCK_DIMS:
            raise NotImplementedError(f"stamp adapter: submodule_args.dim {dim} is not supported (one of {list(BLOCK_DIMS)}, the shipped values)")
        self.model = nn.Sequential(*[_ConvNeXtBlock(dim) for _ in range(blocks)])


class _BaseAdapter(nn.Module):       # adapter.py:41-92
    def __init__(self, in_channels, out_channels, in_cav_lidar_range, out_cav_lidar_range, in_feature_shape, out_feature_shape, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        in_range_lidar = np.array([in_cav_lidar_range[3] - in_cav_lidar_range[0], in_cav_lidar_range[4] - in_cav_lidar_range[1]])
        out_range_lidar = np.array([out_cav_lidar_range[3] - out_cav_lidar_range[0], out_cav_lidar_range[4] - out_cav_lidar_range[1]])
        self.ratio = out_range_lidar / in_range_lidar
        in_ratio = np.array([in_feature_shape[1], in_feature_shape[0]]) / in_range_lidar
        out_ratio = np.array([out_feature_shape[1], out_feature_shape[0]]) / out_range_lidar
        self.feat_ratio = out_ratio / in_ratio
        left = in_cav_lidar_range[0] * in_ratio[0] * self.feat_ratio[0] - out_cav_lidar_range[0] * out_ratio[0]
        right = out_cav_lidar_range[3] * out_ratio[0] - in_cav_lidar_range[3] * in_ratio[0] * self.feat_ratio[0]
        top = in_cav_lidar_range[1] * in_ratio[1] * self.feat_ratio[1] - out_cav_lidar_range[1] * out_ratio[1]
        bottom = out_cav_lidar_range[4] * out_ratio[1] - in_cav_lidar_range[4] * in_ratio[1] * self.feat_ratio[1]
        self.pad = (int(round(left)), int(round(right)), int(round(top)), int(round(bottom)))   # nn.ZeroPad2d's (left, right, top, bottom)
        if not (self.feat_ratio[0] == 1.0 and self.feat_ratio[1] == 1.0):
            raise NotImplementedError(f"stamp adapter: in_feature_shape/out_feature_shape {list(in_feature_shape)} / {list(out_feature_shape)} with "
                                      f"these lidar ranges give a feature ratio of {self.feat_ratio.tolist()}; only (1, 1) is supported (the "
                                      "bilinear resize is not implemented; no shipped yaml resizes)")
        self._cache = _Cache()

    def _padded(self, y):
        return F.pad(y, self.pad) if any(self.pad) else y


class _AdapterIdentity(_BaseAdapter):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.in_channels != self.out_channels:
            raise NotImplementedError(f"stamp adapter: identity with in_channels {self.in_channels} != out_channels {self.out_channels} is not "
                                      "supported (the trilinear resize over the channel axis; no shipped yaml uses it)")

    def run(self, x):
        return x


class _AdapterConv(_BaseAdapter):    # adapter.py:220-244
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.conv = nn.Conv2d(self.in_channels, self.out_channels, kernel_size=1)
        nn.init.kaiming_normal_(self.conv.weight)
        nn.init.constant_(self.conv.bias, 0)

    def run(self, x):
        return self._padded(_conv1x1(self._cache, "conv", self.conv, f32c(x)))


class _AdapterConvNext(_BaseAdapter):   # adapter.py:120-144
    def __init__(self, submodule_args, **kwargs):
        super().__init__(**kwargs)
        self.submodule_args = dict(submodule_args)
        hidden = int(self.submodule_args.get("dim", 64))
        self.channel_convert1 = nn.Conv2d(self.in_channels, hidden, kernel_size=1)
        self.conv = _ConvNeXt(self.submodule_args)
        self.channel_convert2 = nn.Conv2d(hidden, self.out_channels, kernel_size=1)
        self.smoothing = nn.Conv2d(self.out_channels, self.out_channels, kernel_size=3, padding=1)   # never used by the reference's forward

    def run(self, x):
        dev = x.device
        h = _conv1x1(self._cache, "convert1", self.channel_convert1, f32c(x), float(self.submodule_args.get("early_scale", 1.0)))
        other = torch.empty_like(h) if len(self.conv.model) else None
        for i, blk in enumerate(self.conv.model):
            src = blk.tensors()
            params = self._cache.get(("block", i), src, dev, lambda: [None if t is None else f32c(t.detach()) for t in src])
            convnext_block(h, *params, out=other)
            h, other = other, h
        return _conv1x1(self._cache, "convert2", self.channel_convert2, h)


_CORES = {"adapterconvnext": _AdapterConvNext, "adapterconv": _AdapterConv, "identity": _AdapterIdentity}


def _build_core(args, what):
    name = args["core_method"]
    if name in NOT_IMPLEMENTED:
        raise NotImplementedError(f"stamp {what}: core_method {name} is not implemented (adapterconvnext, adapterconv and identity are)")
    if name not in _CORES:
        raise NotImplementedError(f"{what.capitalize()} {name} not implemented")
    return _CORES[name](**args["args"])


class _Wrapper(nn.Module):
    _child = None
    trainable = False   # True: a grad-enabled call goes through convnext_bwd.run_trainable (one autograd Function per call)

    def _core(self):
        return getattr(self, self._child)

    def forward(self, x):
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if grad and not self.trainable:
            raise NotImplementedError("stamp adapter training is not implemented (the backward of the fused ConvNeXt block is missing): call under "
                                      "torch.no_grad(), or freeze the parameters and detach the input")
        require_gpu(x, f"stamp {self._child}")
        if x.dim() != 4 or x.shape[0] < 1 or x.shape[2] * x.shape[3] < 1:
            raise ValueError(f"stamp {self._child}: x must be [agents, channels, H, W], got {list(x.shape)}")
        core = self._core()
        if x.shape[1] != core.in_channels:
            raise ValueError(f"stamp {self._child}: input has {x.shape[1]} channels, the module was built with in_channels {core.in_channels}")
        if grad and (x.requires_grad or any(p.requires_grad for n, p in core.named_parameters() if not n.startswith("smoothing."))):
            from .convnext_bwd import run_trainable
            return run_trainable(core, x)
        with torch.no_grad():   # nothing to differentiate (smoothing is not part of the forward): the inference path
            return core.run(x)


class Adapter(_Wrapper):
    """``Adapter(args)(x)``: x [agents, in_channels, H, W] -> [agents, out_channels, H, W] in the protocol space."""
    _child = "adapter"

    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.adapter = _build_core(args, "adapter")


class Reverter(_Wrapper):
    """``Reverter(args)(x)``: the protocol-space map back into the receiver's feature space."""
    _child = "reverter"

    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.reverter = _build_core(args, "reverter")
