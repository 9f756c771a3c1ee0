"""``PyramidFusion`` / ``weighted_fuse`` -- host-side mirror of HEAL's collaboration backbone
(``opencood/models/fuse_modules/pyramid_fuse.py:17-168``): a ``ResNetBEVBackbone`` whose ResNet is, with ``resnext: true``, built from
``Bottleneck`` blocks with a grouped 3x3 (32 groups, 4 channels per group and 64 planes), one single-supervision 1x1 head per level
and a score-weighted fusion of every level's warped agent maps. Same constructor keys, attribute names and ``state_dict`` keys
(``resnet.layer0.0.conv2.weight``, ``single_head_1.bias``, ``deblocks.2.0.weight`` ...).

Per level ``forward_collab`` is two launches: ``gencomm_pyramid_score_fwd`` (head + sigmoid + 1e-4 + camera crop mask) and
``gencomm_warp_weightfuse_fwd`` (warp, 0 -> -inf, softmax over the agents, weighted sum, in one gather pass: the warped
``[N, C, H, W]`` maps of the reference are never written). The grouped 3x3 runs on ``gencomm_gconv3x3_fwd``
(``bev_backbone.gconv3x3_hip``), everything else of the backbone on ``conv2d_hip``.

By default inference only: the module refuses ``train()`` mode and grad-enabled calls with anything trainable, and always
``align_corners: true``, which no shipped yaml sets. Training is opt-in, as for every other component: ``PyramidFusion(cfg,
trainable=True)``, ``weighted_fuse(..., trainable=True)``, ``score_head(..., trainable=True)`` go through ``pyramid_bwd.py`` (HIP
backward kernels, BatchNorm batch statistics through the grouped layer); under ``no_grad`` in ``eval()`` such a module takes the
inference launches below and returns the same bits."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from .bev_backbone_resnet import Bottleneck, ResNetBEVBackbone, ResNetModified
from .fusion import MAX_AGENTS_PER_SCENE, gather_ego_thetas
from .runtime import dev_ints, f32c, ptr, record_len_list, require_gpu, stream_ptr

NO_RECT = (-1, 0, 0, 0)     # the per-agent "no mask" row of gencomm_pyramid_score_fwd's rect table


def crop_rect(H: int, W: int, ratio_H: float, ratio_W: float) -> Tuple[int, int, int, int]:
    """(h0, h1, w0, w1): the rows / columns where a camera agent's crop mask is 1 on an H x W level (pyramid_fuse.py:151-160), with the
    reference's float arithmetic and Python's own slice semantics for what ``[start_h:end_h, start_w:end_w]`` selects (a negative
    start counts from the end; an empty range selects nothing)."""
    crop_H = H / ratio_H - 4
    crop_W = W / ratio_W - 4
    start_h, end_h = int(H // 2 - crop_H // 2), int(H // 2 + crop_H // 2)
    start_w, end_w = int(W // 2 - crop_W // 2), int(W // 2 + crop_W // 2)
    h0, h1, _ = slice(start_h, end_h).indices(H)
    w0, w1, _ = slice(start_w, end_w).indices(W)
    return h0, max(h1, h0), w0, max(w1, w0)


def crop_rects(H: int, W: int, agent_modality_list: Sequence[str], cam_crop_info: dict) -> List[Tuple[int, int, int, int]]:
    """One rectangle per agent: ``crop_rect`` for an agent whose modality is a key of ``cam_crop_info``, ``NO_RECT`` otherwise."""
    rects = []
    for m in agent_modality_list:
        if m in cam_crop_info:
            rects.append(crop_rect(H, W, cam_crop_info[m][f"crop_ratio_H_{m}"], cam_crop_info[m][f"crop_ratio_W_{m}"]))
        else:
            rects.append(NO_RECT)
    return rects


def _scene_table(lens, n, B, what):
    if len(lens) != B or sum(lens) != n:
        raise ValueError(f"{what}: record_len {lens} inconsistent with {n} agents / {B} scenes")
    if min(lens) < 1 or max(lens) > MAX_AGENTS_PER_SCENE:
        raise ValueError(f"{what}: each scene needs 1..{MAX_AGENTS_PER_SCENE} agents, got {lens}")
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


def _refuse_training(what, tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise NotImplementedError(f"{what}: pyramid training is not built (no backward kernels): call it under torch.no_grad(), "
                                  "or with nothing that requires a gradient")


def weighted_fuse(x, score, record_len, affine_matrix, align_corners=False, trainable=False):
    """pyramid_fuse.py:17-63 as one launch of ``gencomm_warp_weightfuse_fwd``: x [sum(n_cav), C, H, W], score [sum(n_cav), 1, H, W],
    affine_matrix [B, L, L, 2, 3] -> [B, C, H, W]. ``trainable=True``: differentiable in x and score (``pyramid_bwd.WeightedFuseFn``)."""
    if align_corners:
        raise NotImplementedError("weighted_fuse: align_corners=True is not built (no shipped yaml sets it)")
    if not trainable:
        _refuse_training("weighted_fuse", (x, score))
    require_gpu(x, "weighted_fuse")
    lens = record_len_list(record_len)
    n, C, H, W = x.shape
    B = affine_matrix.shape[0]
    off = _scene_table(lens, n, B, "weighted_fuse")
    if tuple(score.shape) != (n, 1, H, W):
        raise ValueError(f"weighted_fuse: score must be [{n}, 1, {H}, {W}], got {tuple(score.shape)}")
    x, score = f32c(x), f32c(score)
    theta = gather_ego_thetas(affine_matrix, lens).to(x.device)
    if trainable and torch.is_grad_enabled() and (x.requires_grad or score.requires_grad):
        from .pyramid_bwd import WeightedFuseFn
        return WeightedFuseFn.apply(x, score, theta, dev_ints(off, x.device), B)
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().gencomm_warp_weightfuse_fwd(ptr(x), ptr(score), ptr(theta), ptr(dev_ints(off, x.device)), ptr(out), B, n, C, H, W,
                                                      stream_ptr(x.device)), "gencomm_warp_weightfuse_fwd")
    return out


def score_head(x: torch.Tensor, head: nn.Conv2d, rects: Optional[Sequence[Sequence[int]]] = None, trainable: bool = False):
    """(occ_map, score) of one level, both [n, 1, H, W], as one launch of ``gencomm_pyramid_score_fwd``: occ = head(x),
    score = (sigmoid(occ) + 1e-4) * crop mask. ``rects``: one (h0, h1, w0, w1) per agent (``crop_rects``), or None for no mask.
    ``trainable=True``: both outputs are differentiable in x and the head's parameters (``pyramid_bwd.ScoreHeadFn``)."""
    require_gpu(x, "score_head")
    x = f32c(x)
    n, C, H, W = x.shape
    if tuple(head.weight.shape) != (1, C, 1, 1) or head.bias is None:
        raise ValueError(f"score_head: the head must be Conv2d({C}, 1, 1) with a bias, got weight {tuple(head.weight.shape)}")
    rect = None
    if rects is not None:
        if len(rects) != n:
            raise ValueError(f"score_head: {len(rects)} rectangles for {n} agents")
        rect = dev_ints([v for r in rects for v in r], x.device)
    if trainable and torch.is_grad_enabled() and (x.requires_grad or head.weight.requires_grad or head.bias.requires_grad):
        from .pyramid_bwd import ScoreHeadFn
        return ScoreHeadFn.apply(x, rect, head.weight, head.bias)
    occ = torch.empty((n, 1, H, W), dtype=torch.float32, device=x.device)
    score = torch.empty_like(occ)
    _lib.check(_lib.lib().gencomm_pyramid_score_fwd(ptr(x), ptr(f32c(head.weight.detach())), ptr(f32c(head.bias.detach())), ptr(rect), ptr(occ),
                                                    ptr(score), n, C, H, W, stream_ptr(x.device)), "gencomm_pyramid_score_fwd")
    return occ, score


class PyramidFusion(ResNetBEVBackbone):  # pyramid_fuse.py:65-168
    def __init__(self, model_cfg, input_channels=64, trainable=False):
        super().__init__(model_cfg, input_channels)
        self.trainable = bool(trainable)   # a plain attribute, like the one set on the blocks below: the state_dict keys do not change
        if model_cfg["resnext"]:
            self.resnet = ResNetModified(Bottleneck, self.model_cfg['layer_nums'], self.model_cfg['layer_strides'], self.model_cfg['num_filters'],
                                         inplanes=model_cfg.get('inplanes', 64), groups=32, width_per_group=4)
        self.align_corners = model_cfg.get('align_corners', False)
        if self.align_corners:
            raise NotImplementedError("PyramidFusion: align_corners: true is not built (no shipped yaml sets it)")
        for i in range(self.num_levels):   # the single supervision heads
            setattr(self, f"single_head_{i}", nn.Conv2d(self.model_cfg["num_filters"][i], 1, kernel_size=1))
        for m in self.modules():
            if isinstance(m, Bottleneck):
                m.trainable = self.trainable

    def _refuse(self, spatial_features):
        if self.trainable:
            return
        if self.training:
            raise NotImplementedError("PyramidFusion: train() mode is not built (BatchNorm batch statistics through the grouped layer; pyramid "
                                      "training is a later change): call .eval()")
        _refuse_training("PyramidFusion", [spatial_features, *self.parameters()])

    def forward_single(self, spatial_features):
        """The single-agent pass: (final_feature, occ_map_list)."""
        self._refuse(spatial_features)
        feature_list = self.get_multiscale_feature(spatial_features)
        occ_map_list = [score_head(feature_list[i], getattr(self, f"single_head_{i}"), None, self.trainable)[0] for i in range(self.num_levels)]
        return self.decode_multiscale_feature(feature_list), occ_map_list

    def forward_collab(self, spatial_features, record_len, affine_matrix, agent_modality_list=None, cam_crop_info=None):
        """spatial_features [sum(record_len), C, H, W], affine_matrix [B, L, L, 2, 3], agent_modality_list: the modality of each cav,
        cam_crop_info: {'m2': {'crop_ratio_W_m2': 0.5, 'crop_ratio_H_m2': 0.5}} -> (fused_feature, occ_map_list)."""
        self._refuse(spatial_features)
        crop = cam_crop_info is not None and len(cam_crop_info) > 0 and not self.training   # the reference skips the mask when self.training
        if crop and (agent_modality_list is None or len(agent_modality_list) != spatial_features.shape[0]):
            raise ValueError("PyramidFusion.forward_collab: cam_crop_info needs agent_modality_list with one entry per agent")
        feature_list = self.get_multiscale_feature(spatial_features)
        fused_feature_list, occ_map_list = [], []
        for i in range(self.num_levels):
            H, W = feature_list[i].shape[2:]
            rects = crop_rects(H, W, agent_modality_list, cam_crop_info) if crop else None
            occ_map, score = score_head(feature_list[i], getattr(self, f"single_head_{i}"), rects, self.trainable)
            occ_map_list.append(occ_map)
            fused_feature_list.append(weighted_fuse(feature_list[i], score, record_len, affine_matrix, self.align_corners, self.trainable))
        return self.decode_multiscale_feature(fused_feature_list), occ_map_list
