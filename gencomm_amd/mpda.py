"""``MPDAAlign`` and its parts -- host-side mirror of MPDA's feature aligner (``opencood/models/mpda_modules``): the ``LearnableResizer``
(``resizer.py:27-72``) built from unmasked ``SwapFusionEncoder`` stacks (``wg_fusion_modules.py:177-206, 341-376``), the
``CrossDomainFusionEncoder`` (``:209-338``) and the domain classifier ``DAImgHead`` (``classfier.py:36-65``), with the reference's
class names, constructor arguments and ``state_dict`` keys (``tests/golden/mpda_keys.json``). ``MPDAAlign(args)`` holds them as
``resizer`` / ``cdt`` / ``classifier`` and reproduces ``heter_model_baseline_w_mpda.py:232-262``: the compute core of the MPDA
baseline, as components. The model shell and ``point_pillar_mpda_loss`` are not part of this package.

The ``torch.nn`` classes are parameter containers; every forward runs on the HIP kernels through the C ABI:
  LayerNorm                      gencomm_ln_nchw_fwd
  to_qkv / to_q / to_k / to_v, to_out and proj (+ skip), Linear + GELU, Linear + skip, the heads' Linear, channel_selector, DAImgHead
                                 1x1 convolutions on the implicit-GEMM kernel (gencomm_conv2d_act_res_fwd / conv2d_hip)
  window / grid attention        gencomm_quad_attn_fwd: 2 x 2 groups by index arithmetic on the NCHW maps; self form (q | k | v blocks
                                 of one to_qkv output, rel_pos_bias read in the kernel) and cross form (queries from the collaborator's
                                 map, keys / values from the ego's: the ego is projected ONCE and broadcast, where the reference
                                 repeats it per collaborator)
  F.interpolate(bilinear)        gencomm_resize_bilinear_fwd
  residual_block                 conv3x3 + folded BatchNorm + LeakyReLU(0.01) (act 4), conv3x3 + folded BatchNorm + the block's skip

The default constructors infer only: ``train()`` mode, and a grad-enabled call with a trainable parameter or input, raise
``NotImplementedError`` naming ``mpda training``. ``trainable=True`` (on ``MPDAAlign``, ``LearnableResizer``, ``SwapFusionEncoder``,
``CrossDomainFusionEncoder`` and ``DAImgHead``, passed down to children; no parameter or buffer is added, the ``state_dict`` is the
same) sends those calls through the ``torch.autograd.Function``s of ``mpda_bwd.py``: the same kernel calls with a tape, the attention
through ``gencomm_quad_attn_train_fwd``, dropout and BatchNorm batch statistics in ``train()`` mode, and the HIP backward. A
``no_grad`` call in ``eval()`` mode runs the inference path on a trainable module too. ``wg_att.window_size`` other than 2 and
odd H or W raise naming the key / the dimension. ``CrossDomainSwapFusionBlock`` hard-codes ``win_size = 2`` whatever the yaml's
``window_size`` says, as the reference does."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, train_ops as T
from .bev_backbone import conv2d_hip
from .cobevt import PreNormResidual
from .runtime import f32c, ptr, record_len_list, require_gpu, stream_ptr
from .v2xvit import FeedForward, _linear, _LinearCache

DIM_HEADS = (16, 32, 64)    # what gencomm_quad_attn_fwd has kernels for


# ----------------------------------------------------------------------------------------- guards and kernel wrappers
def _refuse_training(module: nn.Module, what: str, tensors) -> None:
    if module.training:
        raise NotImplementedError(f"{what}: train() mode is not built (mpda training -- dropout, BatchNorm batch statistics and every "
                                  "backward kernel -- is a later change): call .eval()")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [*tensors, *module.parameters()]):
        raise NotImplementedError(f"{what}: mpda training is not built (no backward kernels): call it under torch.no_grad(), or with "
                                  "nothing that requires a gradient")


def _training_path(module: nn.Module, what: str, tensors) -> bool:
    """True: the call goes through mpda_bwd.py (a trainable module in train() mode, or with gradients to produce). False: inference;
    a default module refuses what it cannot do, in the words it always used."""
    if getattr(module, "trainable", False):
        if module.training:
            return True
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [*tensors, *module.parameters()]):
            return True
        return False
    _refuse_training(module, what, tensors)
    return False


def _check_even(what: str, H: int, W: int) -> None:
    if H % 2 or H < 2:
        raise ValueError(f"{what}: H must be even and >= 2 (2 x 2 windows), got H = {H}")
    if W % 2 or W < 2:
        raise ValueError(f"{what}: W must be even and >= 2 (2 x 2 windows), got W = {W}")


def _check_dim_head(what: str, dim_head: int) -> None:
    if dim_head not in DIM_HEADS:
        raise ValueError(f"{what}: dim_head {dim_head} is not supported (the quad-attention kernel has dim_head in {DIM_HEADS})")


def quad_attention(q, k, v, bias_table, heads: int, dim_head: int, grid_mode: int, q_coff: int = 0, k_coff: int = 0, v_coff: int = 0):
    """``gencomm_quad_attn_fwd``: q [N, q_ct, H, W], k and v [Nkv, kv_ct, H, W] (the same channel total; Nkv == N or 1), each read from
    its channel offset on; bias_table [9, heads] or None -> [N, heads dim_head, H, W]."""
    N, q_ct, H, W = q.shape
    Nkv, kv_ct = k.shape[:2]
    if tuple(v.shape) != tuple(k.shape) or tuple(k.shape[2:]) != (H, W):
        raise ValueError(f"quad_attention: k {tuple(k.shape)} and v {tuple(v.shape)} must agree and share the queries' {H}x{W} map")
    inner, hw = heads * dim_head, H * W
    if max(k_coff, v_coff) + inner > kv_ct or q_coff + inner > q_ct:
        raise ValueError("quad_attention: channel offset + heads dim_head exceeds the tensor's channels")
    out = torch.empty(N, inner, H, W, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().gencomm_quad_attn_fwd(ptr(q) + 4 * q_coff * hw, ptr(k) + 4 * k_coff * hw, ptr(v) + 4 * v_coff * hw, ptr(bias_table), ptr(out),
                                                N, Nkv, heads, dim_head, H, W, q_ct, kv_ct, int(grid_mode),
                                                stream_ptr(q.device)), "gencomm_quad_attn_fwd")
    return out


def pack_keep(keep):
    """bool [N, heads, G, 16] (element 4 i + j: probability (query token i, key token j) survives) -> the kernel's packed words
    [N, heads, G], bit 4 i + j, as int16 holding the uint16 bit pattern."""
    w = (keep.to(torch.int32) << torch.arange(16, dtype=torch.int32, device=keep.device)).sum(dim=-1)
    return torch.where(w >= 32768, w - 65536, w).to(torch.int16).contiguous()


def draw_keep(masks, N: int, heads: int, G: int, p: float, device):
    """The attention's keep mask, bool [N, heads, G, 16], drawn as ``torch.rand(N, heads, G, 16, device=device) >= p`` at its position
    in the order of a ``v2xvit_bwd._Masks`` (recorded there as the bool tensor; replayed from it)."""
    if masks.replay:
        keep = masks.recorded[masks.pos]
        masks.pos += 1
    else:
        keep = torch.rand(N, heads, G, 16, device=device) >= p
        masks.recorded.append(keep)
    return keep


def unpack_keep(words):
    """The inverse of pack_keep: int16 [N, heads, G] -> bool [N, heads, G, 16]."""
    w = words.to(torch.int32) & 0xFFFF
    return ((w[..., None] >> torch.arange(16, dtype=torch.int32, device=words.device)) & 1).bool()


def quad_attention_train(q, k, v, bias_table, heads: int, dim_head: int, grid_mode: int, q_coff: int = 0, k_coff: int = 0, v_coff: int = 0,
                         keep=None, keep_scale: float = 1.0):
    """``gencomm_quad_attn_train_fwd``: ``quad_attention`` with an optional packed keep mask (``pack_keep``) on the probabilities."""
    N, q_ct, H, W = q.shape
    Nkv, kv_ct = k.shape[:2]
    if tuple(v.shape) != tuple(k.shape) or tuple(k.shape[2:]) != (H, W):
        raise ValueError(f"quad_attention_train: k {tuple(k.shape)} and v {tuple(v.shape)} must agree and share the queries' {H}x{W} map")
    inner, hw = heads * dim_head, H * W
    if max(k_coff, v_coff) + inner > kv_ct or q_coff + inner > q_ct:
        raise ValueError("quad_attention_train: channel offset + heads dim_head exceeds the tensor's channels")
    if keep is not None and (keep.dtype != torch.int16 or tuple(keep.shape) != (N, heads, (H // 2) * (W // 2)) or not keep.is_contiguous()):
        raise ValueError(f"quad_attention_train: keep must be contiguous int16 [{N}, {heads}, {(H // 2) * (W // 2)}]")
    out = torch.empty(N, inner, H, W, dtype=torch.float32, device=q.device)
    _lib.check(_lib.lib().gencomm_quad_attn_train_fwd(ptr(q) + 4 * q_coff * hw, ptr(k) + 4 * k_coff * hw, ptr(v) + 4 * v_coff * hw, ptr(bias_table),
                                                      ptr(keep), float(keep_scale), ptr(out), N, Nkv, heads, dim_head, H, W, q_ct, kv_ct,
                                                      int(grid_mode), stream_ptr(q.device)), "gencomm_quad_attn_train_fwd")
    return out


def quad_attention_bwd(q, k, v, bias_table, dout, heads: int, dim_head: int, grid_mode: int, q_coff: int = 0, k_coff: int = 0, v_coff: int = 0,
                       keep=None, keep_scale: float = 1.0, self_form: bool = False):
    """``gencomm_quad_attn_bwd`` -> (dq, dk, dv, dbias or None). ``self_form``: q, k and v are one to_qkv output [N, 3 inner, H, W] and
    dq | dk | dv come back as ONE tensor dqkv of that shape (returned three times)."""
    N, q_ct, H, W = q.shape
    Nkv, kv_ct = k.shape[:2]
    inner, hw, dev = heads * dim_head, H * W, q.device
    if max(k_coff, v_coff) + inner > kv_ct or q_coff + inner > q_ct:
        raise ValueError("quad_attention_bwd: channel offset + heads dim_head exceeds the tensor's channels")
    if tuple(dout.shape) != (N, inner, H, W):
        raise ValueError(f"quad_attention_bwd: dout {tuple(dout.shape)} must be [{N}, {inner}, {H}, {W}]")
    l = _lib.lib()
    if self_form:
        dq = dk = dv = torch.empty_like(q) if q_ct == 3 * inner else torch.zeros_like(q)
    else:
        dq = torch.empty_like(q) if q_ct == inner else torch.zeros_like(q)
        dk, dv = (torch.empty_like(k) if kv_ct == inner else torch.zeros_like(k) for _ in range(2))
    dbias = torch.empty(9, heads, dtype=torch.float32, device=dev) if bias_table is not None else None
    need = _lib.check_size(l.gencomm_quad_attn_bwd_workspace_bytes(N, Nkv, heads, dim_head, H, W, int(bias_table is not None)),
                           "gencomm_quad_attn_bwd_workspace_bytes")
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
    _lib.check(l.gencomm_quad_attn_bwd(ptr(q) + 4 * q_coff * hw, ptr(k) + 4 * k_coff * hw, ptr(v) + 4 * v_coff * hw, ptr(bias_table), ptr(keep),
                                       float(keep_scale), ptr(dout), ptr(dq) + 4 * q_coff * hw, ptr(dk) + 4 * k_coff * hw, ptr(dv) + 4 * v_coff * hw,
                                       ptr(dbias), N, Nkv, heads, dim_head, H, W, q_ct, kv_ct, int(grid_mode), ptr(ws), need, stream_ptr(dev)),
               "gencomm_quad_attn_bwd")
    return dq, dk, dv, dbias


def resize_bilinear_bwd(dy, in_size):
    """The adjoint of ``resize_bilinear``: dy [n, C, Ho, Wo] -> dx [n, C, Hi, Wi] (``gencomm_resize_bilinear_bwd``, a gather)."""
    dy = f32c(dy)
    n, C, Ho, Wo = dy.shape
    Hi, Wi = int(in_size[0]), int(in_size[1])
    dx = torch.empty(n, C, Hi, Wi, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().gencomm_resize_bilinear_bwd(ptr(dy), ptr(dx), n, C, Hi, Wi, Ho, Wo, stream_ptr(dy.device)), "gencomm_resize_bilinear_bwd")
    return dx


def leaky_relu(x, slope: float = 0.01):
    x = f32c(x)
    y = torch.empty_like(x)
    _lib.check(_lib.lib().gencomm_leaky_relu_fwd(ptr(x), ptr(y), x.numel(), float(slope), stream_ptr(x.device)), "gencomm_leaky_relu_fwd")
    return y


def leaky_relu_bwd(y, dy, slope: float = 0.01):
    """dx = dy (y > 0 ? 1 : slope), from the OUTPUT y; slope 0 is the ReLU's adjoint."""
    y, dy = f32c(y), f32c(dy)
    dx = torch.empty_like(y)
    _lib.check(_lib.lib().gencomm_leaky_relu_bwd(ptr(y), ptr(dy), ptr(dx), y.numel(), float(slope), stream_ptr(y.device)), "gencomm_leaky_relu_bwd")
    return dx


def resize_bilinear(x, size):
    """``F.interpolate(x, size, mode='bilinear', align_corners=False)`` as one launch of ``gencomm_resize_bilinear_fwd``."""
    x = f32c(x)
    n, C, Hi, Wi = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = torch.empty(n, C, Ho, Wo, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().gencomm_resize_bilinear_fwd(ptr(x), ptr(y), n, C, Hi, Wi, Ho, Wo, stream_ptr(x.device)), "gencomm_resize_bilinear_fwd")
    return y


def _conv_bn_act(x, conv: nn.Conv2d, bn: nn.BatchNorm2d, act: int, residual=None):
    """act(BN_eval(conv3x3(x))) (+ residual after the activation) as one launch of gencomm_conv2d_act_res_fwd; act 4 = LeakyReLU(0.01).
    The prepared weight and the folded BatchNorm are cached on the module, keyed as conv2d_hip keys them."""
    from .bev_backbone import _versions
    from .runtime import conv2d_prepare
    dev = x.device
    l, st = _lib.lib(), stream_ptr(dev)
    bnp = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
    key = _versions(conv.weight, conv.bias, *bnp, bn.num_batches_tracked) + (str(dev),)
    cache = getattr(conv, "_gc_cache", None)
    cout, cin, kh, kw = conv.weight.shape
    if cache is None or cache[0] != key:
        prepared = conv2d_prepare(f32c(conv.weight.detach()), cin, cout, kh, kw, 0, dev)
        ss = torch.empty(2, cout, dtype=torch.float32, device=dev)
        d = [f32c(t.detach()) for t in bnp]
        b = f32c(conv.bias.detach()) if conv.bias is not None else None
        _lib.check(l.gencomm_conv2d_fold(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(b), float(bn.eps), cout, ptr(ss[0]), ptr(ss[1]), st),
                   "gencomm_conv2d_fold")
        cache = (key, prepared, ss)
        conv._gc_cache = cache
    _, prepared, ss = cache
    n, c, H, W = x.shape
    if c != cin:
        raise ValueError(f"expected {cin} input channels, got {c}")
    y = torch.empty(n, cout, H, W, dtype=torch.float32, device=dev)
    _lib.check(l.gencomm_conv2d_act_res_fwd(ptr(x), ptr(prepared), ptr(ss[0]), ptr(ss[1]), ptr(residual), ptr(y), n, cin, H, W, cout, kh, kw,
                                            1, conv.padding[0], int(act), st), "gencomm_conv2d_act_res_fwd")
    return y


def _ln(x, norm: nn.LayerNorm):
    return T.ln_fwd(x, norm.weight.detach(), norm.bias.detach(), norm.eps, False)


def _head(cache: _LinearCache, mlp_head: nn.Sequential, x):
    """mlp_head: Rearrange, LayerNorm, Linear, Rearrange (the parameters sit at 1 and 2)."""
    lin = mlp_head[2]
    return _linear(_ln(x, mlp_head[1]), cache.get("head", [lin.weight, lin.bias], lambda: (lin.weight, lin.bias), x.device))


# ----------------------------------------------------------------------------------------- the window + grid self-attention stack
class Attention(nn.Module):  # wg_fusion_modules.py:101-174
    def __init__(self, dim, dim_head=32, dropout=0.0, window_size=7):
        super().__init__()
        assert (dim % dim_head) == 0, "dimension should be divisible by dimension per head"
        self.heads, self.dim_head = dim // dim_head, dim_head
        self.scale = dim_head ** -0.5
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.attend = nn.Sequential(nn.Softmax(dim=-1), nn.Dropout(dropout))
        self.to_out = nn.Sequential(nn.Linear(dim, dim, bias=False), nn.Dropout(dropout))
        self.rel_pos_bias = nn.Embedding((2 * window_size - 1) ** 2, self.heads)
        pos = torch.arange(window_size)
        grid = torch.stack(torch.meshgrid(pos, pos, indexing="ij")).flatten(1).t()      # [(i j), 2]
        rel_pos = grid[:, None, :] - grid[None, :, :] + window_size - 1
        # [ws ws, ws ws]; the kernel computes the same value at window_size 2
        self.register_buffer("rel_pos_indices", (rel_pos * torch.tensor([2 * window_size - 1, 1])).sum(dim=-1), persistent=False)


class SwapFusionBlock(nn.Module):  # wg_fusion_modules.py:177-206
    """``block`` keeps the reference's Sequential indices: Rearrange, window attention, FeedForward, Rearrange, Rearrange, grid
    attention, FeedForward, Rearrange -- the parameters sit at 1, 2, 5 and 6."""

    def __init__(self, input_dim, mlp_dim, dim_head, window_size, drop_out):
        super().__init__()
        self.block = nn.Sequential(
            nn.Identity(),
            PreNormResidual(input_dim, Attention(input_dim, dim_head, drop_out, window_size)),
            PreNormResidual(input_dim, FeedForward(input_dim, mlp_dim, drop_out)),
            nn.Identity(), nn.Identity(),
            PreNormResidual(input_dim, Attention(input_dim, dim_head, drop_out, window_size)),
            PreNormResidual(input_dim, FeedForward(input_dim, mlp_dim, drop_out)),
            nn.Identity())


class SwapFusionEncoder(nn.Module):  # wg_fusion_modules.py:341-376 (unmasked)
    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.depth = args["depth"]
        input_dim, mlp_dim, dim_head = args["input_dim"], args["mlp_dim"], args["dim_head"]
        window_size, drop_out = args["window_size"], args["drop_out"]
        if window_size != 2:
            raise ValueError(f"SwapFusionEncoder: window_size {window_size} is not supported: the quad-attention kernel partitions into 2 x 2 "
                             "windows (every shipped MPDA yaml sets wg_att.window_size: 2)")
        _check_dim_head("SwapFusionEncoder", dim_head)
        if input_dim % dim_head:
            raise ValueError(f"SwapFusionEncoder: input_dim {input_dim} is not a multiple of dim_head {dim_head}")
        self.mask = False
        self.layers = nn.ModuleList([SwapFusionBlock(input_dim, mlp_dim, dim_head, window_size, drop_out) for _ in range(self.depth)])
        self.mlp_head = nn.Sequential(nn.Identity(), nn.LayerNorm(input_dim), nn.Linear(input_dim, input_dim), nn.Identity())
        self._linears = _LinearCache()

    def _attention(self, key, pre: PreNormResidual, h, grid_mode, tape=None, masks=None):
        """With a `tape` (training) the attention goes through gencomm_quad_attn_train_fwd and the tape receives what the backward
        reads; the packed keep mask of the probabilities is drawn FIRST in the half-block, then the mask after to_out."""
        att, cache = pre.fn, self._linears
        qkv = _linear(_ln(h, pre.norm), cache.get((key, "qkv"), [att.to_qkv.weight], lambda: (att.to_qkv.weight, None), h.device))
        inner = att.heads * att.dim_head
        table = f32c(att.rel_pos_bias.weight.detach())
        o = att.to_out[0]
        entry = cache.get((key, "out"), [o.weight], lambda: (o.weight, None), h.device)
        if tape is None:
            out = quad_attention(qkv, qkv, qkv, table, att.heads, att.dim_head, grid_mode, 0, inner, 2 * inner)
            return _linear(out, entry, 0, h)
        p_att, p_out = float(att.attend[1].p), float(att.to_out[1].p)
        keep, ks = None, 1.0
        if masks.active and p_att > 0:
            n, _, H, W = h.shape
            keep, ks = pack_keep(draw_keep(masks, n, att.heads, (H // 2) * (W // 2), p_att, h.device)), 1.0 / (1.0 - p_att)
        out = quad_attention_train(qkv, qkv, qkv, table, att.heads, att.dim_head, grid_mode, 0, inner, 2 * inner, keep, ks)
        if masks.active and p_out > 0:
            y, m = masks.apply(_linear(out, entry), p_out)
            y = y + h
        else:
            y, m = _linear(out, entry, 0, h), None
        tape.append(("att", pre, int(grid_mode), h, qkv, out, table, keep, ks, m))
        return y

    def _feed_forward(self, key, pre: PreNormResidual, h, tape=None, masks=None):
        cache, l0, l3 = self._linears, pre.fn.net[0], pre.fn.net[3]
        mid = _linear(_ln(h, pre.norm), cache.get((key, "ff0"), [l0.weight, l0.bias], lambda: (l0.weight, l0.bias), h.device), 2)   # Linear + GELU
        e3 = cache.get((key, "ff3"), [l3.weight, l3.bias], lambda: (l3.weight, l3.bias), h.device)
        if tape is None:
            return _linear(mid, e3, 0, h)                                                                                          # Linear + skip
        p = float(pre.fn.net[2].p)
        if masks.active and p > 0:
            mid, m_mid = masks.apply(mid, p)
            y, m_out = masks.apply(_linear(mid, e3), p)
            y = y + h
        else:
            y, m_mid, m_out = _linear(mid, e3, 0, h), None, None
        tape.append(("ff", pre, h, mid, m_mid, m_out))
        return y

    def dropout_p(self) -> float:
        return max([float(m.p) for m in self.modules() if isinstance(m, nn.Dropout)], default=0.0)

    def _forward_hip(self, x, tape=None, masks=None):
        """`tape` (a list) and `masks` (v2xvit_bwd._Masks): the training forward of mpda_bwd.SwapEncoderFunction. The kernel calls are
        the same; with dropout active the epilogue-fused residuals become separate additions."""
        h = f32c(x)
        for i, blk in enumerate(self.layers):
            b = blk.block
            h = self._attention((i, "window"), b[1], h, 0, tape, masks)
            h = self._feed_forward((i, "window"), b[2], h, tape, masks)
            h = self._attention((i, "grid"), b[5], h, 1, tape, masks)
            h = self._feed_forward((i, "grid"), b[6], h, tape, masks)
        if tape is not None:
            tape.append(("head", h))
        return _head(self._linears, self.mlp_head, h)

    def forward(self, x, mask=None):
        if mask is not None:
            raise NotImplementedError("SwapFusionEncoder: a mask is not built (the reference's module ignores it: self.mask = False)")
        train = _training_path(self, "SwapFusionEncoder", [x])
        n, C, H, W = x.shape
        if C != self.mlp_head[1].normalized_shape[0]:
            raise ValueError(f"SwapFusionEncoder: input has {C} channels, the module was built with input_dim {self.mlp_head[1].normalized_shape[0]}")
        _check_even("SwapFusionEncoder", H, W)
        require_gpu(x, "SwapFusionEncoder.forward")
        if train:
            from .mpda_bwd import SwapEncoderFunction
            return SwapEncoderFunction.apply(self, x, *self.parameters())
        with torch.no_grad():
            return self._forward_hip(x)


# ----------------------------------------------------------------------------------------- the resizer
class residual_block(nn.Module):  # resizer.py:11-24
    def __init__(self, input_dim, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.module = nn.Sequential(nn.Conv2d(input_dim, input_dim, 3, padding=1), nn.BatchNorm2d(input_dim), nn.LeakyReLU(),
                                    nn.Conv2d(input_dim, input_dim, 3, padding=1), nn.BatchNorm2d(input_dim))

    def forward(self, x):
        """Called by LearnableResizer (which has refused what a default module refuses): the folded inference layers, or, for a
        trainable block in train() mode or with gradients to produce, mpda_bwd.ResidualBlockFunction."""
        if self.trainable and (self.training or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))):
            from .mpda_bwd import ResidualBlockFunction
            return ResidualBlockFunction.apply(self, x, *self.parameters())
        m = self.module
        return _conv_bn_act(_conv_bn_act(x, m[0], m[1], 4), m[3], m[4], 0, residual=x)


class LearnableResizer(nn.Module):  # resizer.py:27-72
    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.channel_selector = nn.Conv2d(args["input_channel"], args["output_channel"], 1)
        self.wg_att_1 = SwapFusionEncoder(args["wg_att"], trainable)
        self.wg_att_2 = SwapFusionEncoder(args["wg_att"], trainable)
        self.res_blocks = nn.ModuleList([residual_block(args["residual"]["input_dim"], trainable) for _ in range(args["residual"]["depth"])])

    def _forward_train(self, ego_feature, cav_feature):
        """The same calls as the inference path, each an autograd node of its own (mpda_bwd.py; the 1x1 channel_selector through
        conv2d_hip's own HIP backward); the additions are plain torch, as in the inference path."""
        from .mpda_bwd import ResizeFunction
        size = tuple(ego_feature.shape[2:])
        cav = conv2d_hip(f32c(cav_feature), self.channel_selector, None, relu=False)
        one = ResizeFunction.apply(self.wg_att_1(cav), size)
        two = one
        for blk in self.res_blocks:
            two = blk(two)
        two = self.wg_att_2(two + one)
        return ResizeFunction.apply(cav, size) + two

    def forward(self, ego_feature, cav_feature):
        train = _training_path(self, "LearnableResizer", [ego_feature, cav_feature])
        h, w = ego_feature.shape[2:]
        _check_even("LearnableResizer (the ego's map)", h, w)
        _check_even("LearnableResizer (the collaborator's map)", *cav_feature.shape[2:])
        require_gpu(cav_feature, "LearnableResizer.forward")
        if train:
            return self._forward_train(ego_feature, cav_feature)
        with torch.no_grad():
            cav = conv2d_hip(f32c(cav_feature), self.channel_selector, None, relu=False)
            one = resize_bilinear(self.wg_att_1(cav), (h, w))
            two = one
            for blk in self.res_blocks:
                two = blk(two)
            two = self.wg_att_2(two + one)
            return resize_bilinear(cav, (h, w)) + two


# ----------------------------------------------------------------------------------------- the cross-domain encoder
class CrossAttention(nn.Module):  # wg_fusion_modules.py:12-97
    def __init__(self, dim, heads, dim_head, qkv_bias, rel_pos_emb=False, norm=nn.LayerNorm):
        super().__init__()
        self.scale = dim_head ** -0.5
        self.heads, self.dim_head, self.rel_pos_emb = heads, dim_head, rel_pos_emb
        self.to_q = nn.Sequential(norm(dim), nn.Linear(dim, heads * dim_head, bias=qkv_bias))
        self.to_k = nn.Sequential(norm(dim), nn.Linear(dim, heads * dim_head, bias=qkv_bias))
        self.to_v = nn.Sequential(norm(dim), nn.Linear(dim, heads * dim_head, bias=qkv_bias))
        self.proj = nn.Linear(heads * dim_head, dim)


class CrossDomainSwapFusionBlock(nn.Module):  # wg_fusion_modules.py:209-303
    def __init__(self, dim, dim_heads, heads, qkv_bias, win_size):
        super().__init__()
        self.win_size = 2   # hard-coded in the reference, whatever `win_size` says
        self.prenorm1 = nn.LayerNorm(dim)
        self.prenorm2 = nn.LayerNorm(dim)
        self.mlp_1 = nn.Sequential(nn.Linear(dim, 2 * dim), nn.GELU(), nn.Linear(2 * dim, dim))
        self.mlp_2 = nn.Sequential(nn.Linear(dim, 2 * dim), nn.GELU(), nn.Linear(2 * dim, dim))
        self.cross_win_1 = CrossAttention(dim, heads, dim_heads, qkv_bias)
        self.cross_win_2 = CrossAttention(dim, heads, dim_heads, qkv_bias)
        self.post_norm = nn.LayerNorm(dim)


class CrossDomainFusionEncoder(nn.Module):  # wg_fusion_modules.py:306-338
    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.depth = args["depth"]
        input_dim, heads, dim_head, window_size = args["input_dim"], args["heads"], args["dim_head"], args["window_size"]
        _check_dim_head("CrossDomainFusionEncoder", dim_head)
        self.layers = nn.ModuleList([CrossDomainSwapFusionBlock(input_dim, dim_head, heads, True, window_size) for _ in range(self.depth)])
        self.mlp_head = nn.Sequential(nn.Identity(), nn.LayerNorm(input_dim), nn.Linear(input_dim, input_dim), nn.Identity())
        self._linears = _LinearCache()

    def _project(self, key, seq: nn.Sequential, x):
        lin = seq[1]
        return _linear(_ln(x, seq[0]), self._linears.get(key, [lin.weight, lin.bias], lambda: (lin.weight, lin.bias), x.device))

    def _cross(self, key, att: CrossAttention, query, ego, grid_mode, tape=None):
        q = self._project((key, "q"), att.to_q, query)
        k = self._project((key, "k"), att.to_k, ego)       # the ego's n_ego maps (1: broadcast to every query map by the kernel)
        v = self._project((key, "v"), att.to_v, ego)
        if tape is None:
            a = quad_attention(q, k, v, None, att.heads, att.dim_head, grid_mode)
        else:
            a = quad_attention_train(q, k, v, None, att.heads, att.dim_head, grid_mode)     # no dropout in the reference's CrossAttention
            tape.append(("cross", att, int(grid_mode), query, q, k, v, a))
        p = att.proj
        return _linear(a, self._linears.get((key, "proj"), [p.weight, p.bias], lambda: (p.weight, p.bias), query.device), 0, query)   # + skip

    def _mlp(self, key, norm, mlp, x, tape=None):
        cache, l0, l2 = self._linears, mlp[0], mlp[2]
        mid = _linear(_ln(x, norm), cache.get((key, "0"), [l0.weight, l0.bias], lambda: (l0.weight, l0.bias), x.device), 2)
        if tape is not None:
            tape.append(("mlp", norm, mlp, x, mid))
        return _linear(mid, cache.get((key, "2"), [l2.weight, l2.bias], lambda: (l2.weight, l2.bias), x.device), 0, x)

    def _forward_hip(self, ego_feature, cav_feature, tape=None):
        ego, x = f32c(ego_feature), f32c(cav_feature)
        for i, blk in enumerate(self.layers):
            x = self._cross((i, "win"), blk.cross_win_1, x, ego, 0, tape)
            x = self._mlp((i, "mlp_1"), blk.prenorm1, blk.mlp_1, x, tape)
            x = self._cross((i, "grid"), blk.cross_win_2, x, ego, 1, tape)
            x = self._mlp((i, "mlp_2"), blk.prenorm2, blk.mlp_2, x, tape)
            if tape is not None:
                tape.append(("ln", blk.post_norm, x))
            x = _ln(x, blk.post_norm)
        if tape is not None:
            tape.append(("head", x))
        return _head(self._linears, self.mlp_head, x)

    def forward(self, ego_feature, cav_feature):
        """ego_feature [n, C, H, W] or [1, C, H, W] (one ego map for every collaborator: what the reference builds with
        ``ego.repeat(n, 1, 1, 1)``), cav_feature [n, C, H, W] -> [n, C, H, W]."""
        train = _training_path(self, "CrossDomainFusionEncoder", [ego_feature, cav_feature])
        n, C, H, W = cav_feature.shape
        if ego_feature.shape[0] not in (1, n) or tuple(ego_feature.shape[1:]) != (C, H, W):
            raise ValueError(f"CrossDomainFusionEncoder: ego_feature {tuple(ego_feature.shape)} must be [{n} or 1, {C}, {H}, {W}]")
        if C != self.mlp_head[1].normalized_shape[0]:
            raise ValueError(f"CrossDomainFusionEncoder: input has {C} channels, the module was built with input_dim "
                             f"{self.mlp_head[1].normalized_shape[0]}")
        _check_even("CrossDomainFusionEncoder", H, W)
        require_gpu(cav_feature, "CrossDomainFusionEncoder.forward")
        if train:
            from .mpda_bwd import CrossDomainFunction
            return CrossDomainFunction.apply(self, ego_feature, cav_feature, *self.parameters())
        with torch.no_grad():
            return self._forward_hip(ego_feature, cav_feature)


# ----------------------------------------------------------------------------------------- the classifier and the aligner
class GradientScalarLayer(nn.Module):  # gradient_layer.py: the identity in the forward (the reversal acts on the gradient only)
    def __init__(self, weight):
        super().__init__()
        self.weight = weight


class DAImgHead(nn.Module):  # classfier.py:36-65
    def __init__(self, in_channels, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.conv1_da = nn.Conv2d(in_channels, 512, kernel_size=1, stride=1)
        self.conv2_da = nn.Conv2d(512, 1, kernel_size=1, stride=1)
        self.rgl = GradientScalarLayer(-9.1)
        for l in [self.conv1_da, self.conv2_da]:
            torch.nn.init.normal_(l.weight, std=0.001)
            torch.nn.init.constant_(l.bias, 0)

    def forward(self, x):
        train = _training_path(self, "DAImgHead", [x])
        require_gpu(x, "DAImgHead.forward")
        if train:
            from .mpda_bwd import DAHeadFunction
            return DAHeadFunction.apply(self, x, *self.parameters())
        with torch.no_grad():
            return conv2d_hip(conv2d_hip(f32c(x), self.conv1_da, None, relu=True), self.conv2_da, None, relu=False)


class MPDAAlign(nn.Module):
    """``heter_model_baseline_w_mpda.py:232-262`` with the shell's attribute names: ``forward(heter_feature_2d, record_len) ->
    (aligned_features, class_logits)``. Per scene the ego map passes through unchanged and the collaborators go through ``resizer``
    then ``cdt`` (``rebuttal: true``: unchanged); the classifier sees the scene's aligned maps. For an ego-only scene the reference
    computes the resizer and ``cdt`` and discards the result: that work is skipped here, the outputs are the same."""

    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.resizer = LearnableResizer(args["resizer"], trainable)
        self.cdt = CrossDomainFusionEncoder(args["cdt"], trainable)
        self.classifier = DAImgHead(args["classifier"] if "classifier" in args else 128, trainable)
        self.rebuttal = args.get("rebuttal", False)

    def _forward_train(self, x, lens):
        """`aligned` assembled with autograd-visible ops (slices and one torch.cat). `rebuttal: true` passes the maps, and so the
        gradients, straight through. An ego-only scene skips the resizer and cdt as the inference path does: no gradient is lost (the
        reference discards that branch), but the resizer's BatchNorm running statistics do not see the ego-to-ego call the reference
        makes in train() mode (a stated difference)."""
        if self.rebuttal or max(lens) == 1:
            aligned = x.clone()
        else:
            parts, off = [], 0
            for k in lens:
                ego = x[off:off + 1]
                parts.append(ego)
                if k > 1:
                    parts.append(self.cdt(ego, self.resizer(ego, x[off + 1:off + k])))
                off += k
            aligned = torch.cat(parts, dim=0)
        return aligned, self.classifier(aligned)

    def forward(self, heter_feature_2d, record_len):
        train = _training_path(self, "MPDAAlign", [heter_feature_2d])
        lens = record_len_list(record_len)
        n = heter_feature_2d.shape[0]
        if sum(lens) != n or min(lens) < 1:
            raise ValueError(f"MPDAAlign: record_len {lens} inconsistent with {n} agents (every scene needs its ego)")
        if not self.rebuttal and max(lens) > 1:
            _check_even("MPDAAlign", *heter_feature_2d.shape[2:])
        require_gpu(heter_feature_2d, "MPDAAlign.forward")
        if train:
            return self._forward_train(f32c(heter_feature_2d), lens)
        with torch.no_grad():
            x = f32c(heter_feature_2d)
            if self.rebuttal or max(lens) == 1:
                aligned = x.clone()   # a tensor of its own, as the reference's torch.cat returns
            else:
                aligned = torch.empty_like(x)
                off = 0
                for k in lens:
                    ego = x[off:off + 1]
                    aligned[off] = x[off]
                    if k > 1:
                        aligned[off + 1:off + k] = self.cdt(ego, self.resizer(ego, x[off + 1:off + k]))
                    off += k
            return aligned, self.classifier(aligned)   # the classifier is per pixel and per map: one call equals the per-scene calls
