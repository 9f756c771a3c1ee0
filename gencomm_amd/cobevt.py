"""``CoBEVT`` -- host-side mirror of the reference's CoBEVT fusion (``opencood/models/fuse_modules/fusion_in_one.py:409-464``; blocks
in ``fuse_modules/swap_fusion_modules.py:131-192``, attention ``:13-128``), selected by ``fusion_method: cobevt`` in the ``*_cobevt.yaml``
configs. Same constructor keys (``input_dim, mlp_dim, agent_size, window_size, drop_out, dim_head, depth``), same ``forward(x, record_len,
affine_matrix)`` and the same ``state_dict`` keys, order and shapes (``tests/golden/cobevt_keys.json``; 76 entries at depth 3).

The ``torch.nn`` classes below are parameter containers; ``forward`` runs on the HIP kernels through the C ABI:
  pad + warp to ego     gencomm_warp_affine_fwd, one launch per scene straight into the padded [B L, C, H, W] buffer (rows of missing
                        agents stay zero, their matrix rows are not read)
  LayerNorm             gencomm_ln_nchw_fwd
  to_qkv, to_out (+ residual), Linear + GELU, Linear + residual, the head's Linear
                        1x1 convolutions on the implicit-GEMM kernel (gencomm_conv2d_act_res_fwd, the ``_linear`` route of v2xvit.py)
  swap attention        gencomm_swap_attn_fwd: window and grid partition by index arithmetic on the NCHW maps, the 3-D relative position
                        bias computed in the kernel (``relative_position_index`` exists here for the checkpoint keys only), keys of
                        padded agents masked from a per-scene count on the device
  mean over the agents  gencomm_agent_mean_fwd
Padded agents ARE materialised, unlike in V2XViTFusion: their rows are zero only before the first residual, they are queries of every
attention, and the head averages over all ``agent_size`` rows (swap_fusion_modules.py:275).

``CoBEVT(args)`` infers only: dropout is the identity in ``eval()``; a call with gradients enabled into a module that has a parameter
or an input requiring grad, and ``train()`` mode with ``drop_out > 0``, raise ``NotImplementedError``. ``CoBEVT(args, trainable=True)``
(what the model shells construct; the precedent is ``V2VNetFusion(args, trainable=True)``) sends those calls through
``cobevt_bwd.CoBEVTFunction``: the same kernel calls with the attention through ``gencomm_swap_attn_train_fwd`` (bit-identical output
while dropout is inactive), a tape of what the backward reads, the dropout masks of ``train()`` mode, and the HIP backward around
``gencomm_swap_attn_bwd``. ``trainable`` adds no parameter or buffer: the ``state_dict`` is the same.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib, train_ops as T
from .fusion import MAX_AGENTS_PER_SCENE, gather_ego_thetas
from .runtime import dev_ints, f32c, ptr, record_len_list, require_gpu, stream_ptr
from .v2xvit import FeedForward, _linear, _LinearCache

WINDOW_SIZES = (4, 8)       # what gencomm_swap_attn_fwd has kernels for
DIM_HEADS = (16, 32, 64)


# ----------------------------------------------------------------------------------------- parameter containers
class PreNormResidual(nn.Module):  # base_transformer.py:17-24
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class Attention(nn.Module):  # swap_fusion_modules.py:13-85
    def __init__(self, dim, dim_head=32, dropout=0.0, agent_size=6, window_size=7):
        super().__init__()
        assert dim % dim_head == 0, "dimension should be divisible by dimension per head"
        self.heads, self.dim_head = dim // dim_head, dim_head
        self.window_size = [agent_size, window_size, window_size]
        L, ws = agent_size, window_size
        coords = torch.stack(torch.meshgrid(torch.arange(L), torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
        rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += L - 1
        rel[:, :, 1] += ws - 1
        rel[:, :, 2] += ws - 1
        rel[:, :, 0] *= (2 * ws - 1) * (2 * ws - 1)
        rel[:, :, 1] *= 2 * ws - 1
        self.register_buffer("relative_position_index", rel.sum(-1))   # [L ws ws, L ws ws]; the kernel computes the same value
        self.to_qkv = nn.Linear(dim, dim * 3, bias=False)
        self.attend = nn.Sequential(nn.Softmax(dim=-1))
        self.to_out = nn.Sequential(nn.Linear(dim, dim, bias=False), nn.Dropout(dropout))
        self.relative_position_bias_table = nn.Embedding((2 * L - 1) * (2 * ws - 1) * (2 * ws - 1), self.heads)


class SwapFusionBlockMask(nn.Module):  # swap_fusion_modules.py:131-163
    def __init__(self, input_dim, mlp_dim, dim_head, window_size, agent_size, drop_out):
        super().__init__()
        self.window_size = window_size
        self.window_attention = PreNormResidual(input_dim, Attention(input_dim, dim_head, drop_out, agent_size, window_size))
        self.window_ffd = PreNormResidual(input_dim, FeedForward(input_dim, mlp_dim, drop_out))
        self.grid_attention = PreNormResidual(input_dim, Attention(input_dim, dim_head, drop_out, agent_size, window_size))
        self.grid_ffd = PreNormResidual(input_dim, FeedForward(input_dim, mlp_dim, drop_out))


# ----------------------------------------------------------------------------------------- the module
class CoBEVT(nn.Module):
    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.depth = args["depth"]
        input_dim, mlp_dim, dim_head = args["input_dim"], args["mlp_dim"], args["dim_head"]
        self.agent_size, self.window_size, self.drop_out = args["agent_size"], args["window_size"], float(args["drop_out"])
        if self.window_size not in WINDOW_SIZES:
            raise ValueError(f"CoBEVT: window_size {self.window_size} is not supported (the swap-attention kernel has window_size in {WINDOW_SIZES})")
        if dim_head not in DIM_HEADS:
            raise ValueError(f"CoBEVT: dim_head {dim_head} is not supported (the swap-attention kernel has dim_head in {DIM_HEADS})")
        if not 1 <= self.agent_size <= MAX_AGENTS_PER_SCENE:
            raise ValueError(f"CoBEVT: agent_size {self.agent_size} is not supported (1..{MAX_AGENTS_PER_SCENE} agents per scene)")
        if input_dim % dim_head:
            raise ValueError(f"CoBEVT: input_dim {input_dim} is not a multiple of dim_head {dim_head}")
        self.layers = nn.ModuleList([SwapFusionBlockMask(input_dim, mlp_dim, dim_head, self.window_size, self.agent_size, self.drop_out)
                                     for _ in range(self.depth)])
        # Reduce('b m d h w -> b d h w', 'mean'), Rearrange, LayerNorm, Linear, Rearrange: the parameters sit at 2 and 3
        self.mlp_head = nn.Sequential(nn.Identity(), nn.Identity(), nn.LayerNorm(input_dim), nn.Linear(input_dim, input_dim), nn.Identity())
        self._linears = _LinearCache()

    def forward(self, x, record_len, affine_matrix):
        """x [sumN, C, H, W], record_len [B], affine_matrix [B, L, L, 2, 3] -> [B, C, H, W]."""
        lens = record_len_list(record_len)
        n, C, H, W = x.shape
        B, L = affine_matrix.shape[:2]
        ws = self.window_size
        if len(lens) != B or sum(lens) != n or min(lens) < 1 or max(lens) > L:
            raise ValueError(f"record_len {lens} inconsistent with {n} agents / {B} scenes (1..{L} agents per scene)")
        if L != self.agent_size:
            raise ValueError(f"CoBEVT: affine_matrix holds {L} agents per scene, the module was built with agent_size {self.agent_size}")
        if C != self.mlp_head[2].normalized_shape[0]:
            raise ValueError(f"CoBEVT: input has {C} channels, the module was built with input_dim {self.mlp_head[2].normalized_shape[0]}")
        if H % ws or W % ws:
            raise ValueError(f"CoBEVT: H and W must be multiples of window_size ({ws}), got {H}x{W}")
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        dropout = self.training and self.drop_out > 0
        if self.trainable and (grad or dropout):
            require_gpu(x, "CoBEVT.forward")
            from .cobevt_bwd import CoBEVTFunction
            return CoBEVTFunction.apply(self, x, lens, affine_matrix, *self.parameters())
        if grad:
            raise NotImplementedError("cobevt training is not implemented (the swap-attention backward is missing): call under torch.no_grad() "
                                      "or freeze the module")
        if dropout:
            raise NotImplementedError(f"cobevt training is not implemented: train() mode with drop_out {self.drop_out} > 0 needs the dropout "
                                      "masks; call eval()")
        require_gpu(x, "CoBEVT.forward")
        with torch.no_grad():
            return self._forward_hip(f32c(x), lens, affine_matrix)

    def _attention(self, key, pre: PreNormResidual, h, nvalid, B, grid_mode, tape=None, masks=None):
        """h + to_out(swap attention(to_qkv(LN(h)))) over the padded batch h [B L, C, H, W]. With a `tape` (training) the attention goes
        through gencomm_swap_attn_train_fwd (the same `out`, plus lse) and the tape receives what the backward reads."""
        att, dev, cache = pre.fn, h.device, self._linears
        n, C, H, W = h.shape
        hn = T.ln_fwd(h, pre.norm.weight, pre.norm.bias, pre.norm.eps, False)
        qkv = _linear(hn, cache.get((key, "qkv"), [att.to_qkv.weight], lambda: (att.to_qkv.weight, None), dev))
        out = torch.empty_like(h)
        table = f32c(att.relative_position_bias_table.weight.detach())
        dims = (B, n // B, att.heads, att.dim_head, self.window_size, H, W, int(grid_mode), stream_ptr(dev))
        o = att.to_out[0]
        entry = cache.get((key, "out"), [o.weight], lambda: (o.weight, None), dev)
        if tape is None:
            _lib.check(_lib.lib().gencomm_swap_attn_fwd(ptr(qkv), ptr(table), ptr(nvalid), ptr(out), *dims), "gencomm_swap_attn_fwd")
            return _linear(out, entry, 0, h)
        lse = torch.empty(n, att.heads, H, W, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gencomm_swap_attn_train_fwd(ptr(qkv), ptr(table), ptr(nvalid), ptr(out), ptr(lse), *dims), "gencomm_swap_attn_train_fwd")
        p = float(att.to_out[1].p)
        if masks.active and p > 0:
            y, m = masks.apply(_linear(out, entry), p)
            y = y + h
        else:
            y, m = _linear(out, entry, 0, h), None
        tape.append(("att", pre, int(grid_mode), h, qkv, out, lse, table, m))
        return y

    def _feed_forward(self, key, pre: PreNormResidual, h, tape=None, masks=None):
        dev, cache = h.device, self._linears
        hn = T.ln_fwd(h, pre.norm.weight, pre.norm.bias, pre.norm.eps, False)
        l0, l3 = pre.fn.net[0], pre.fn.net[3]
        mid = _linear(hn, cache.get((key, "ff0"), [l0.weight, l0.bias], lambda: (l0.weight, l0.bias), dev), 2)        # Linear + GELU
        e3 = cache.get((key, "ff3"), [l3.weight, l3.bias], lambda: (l3.weight, l3.bias), dev)
        if tape is None:
            return _linear(mid, e3, 0, h)                                                                             # Linear + residual
        p = float(pre.fn.net[2].p)
        if masks.active and p > 0:
            mid, m_mid = masks.apply(mid, p)
            y, m_out = masks.apply(_linear(mid, e3), p)
            y = y + h
        else:
            y, m_mid, m_out = _linear(mid, e3, 0, h), None, None
        tape.append(("ff", pre, h, mid, m_mid, m_out))
        return y

    def _forward_hip(self, x, lens, affine_matrix, tape=None, masks=None):
        """`tape` (a list) and `masks` (v2xvit_bwd._Masks): the training forward of cobevt_bwd.CoBEVTFunction. The kernel calls are the
        same (the attention through the train entry); with dropout active the epilogue-fused residuals become separate additions."""
        n, C, H, W = x.shape
        B, L = affine_matrix.shape[:2]
        l, dev = _lib.lib(), x.device
        st = stream_ptr(dev)
        theta = gather_ego_thetas(affine_matrix, lens).to(dev)
        # regroup (fuse_utils.py:13-64) + warp (fusion_in_one.py:455-459) in one step: scene b's agents land in rows b L .. b L + N_b - 1
        h = (torch.empty if all(k == L for k in lens) else torch.zeros)(B * L, C, H, W, dtype=torch.float32, device=dev)
        off = 0
        for b, k in enumerate(lens):
            _lib.check(l.gencomm_warp_affine_fwd(ptr(x[off:]), ptr(theta[off:]), ptr(h[b * L:]), k, C, H, W, st), "gencomm_warp_affine_fwd")
            off += k
        nvalid = dev_ints(lens, dev)
        for i, blk in enumerate(self.layers):
            h = self._attention((i, "window"), blk.window_attention, h, nvalid, B, 0, tape, masks)
            h = self._feed_forward((i, "window"), blk.window_ffd, h, tape, masks)
            h = self._attention((i, "grid"), blk.grid_attention, h, nvalid, B, 1, tape, masks)
            h = self._feed_forward((i, "grid"), blk.grid_ffd, h, tape, masks)
        mean = torch.empty(B, C, H, W, dtype=torch.float32, device=dev)
        _lib.check(l.gencomm_agent_mean_fwd(ptr(h), ptr(mean), B, L, C * H * W, st), "gencomm_agent_mean_fwd")
        norm, lin = self.mlp_head[2], self.mlp_head[3]
        hn = T.ln_fwd(mean, norm.weight, norm.bias, norm.eps, False)
        if tape is not None:
            tape.append(("head", mean, hn, theta, nvalid))
        return _linear(hn, self._linears.get("head", [lin.weight, lin.bias], lambda: (lin.weight, lin.bias), dev))
