"""``PointPillarPyramidLoss`` and ``PointPillarMPDALoss`` -- the training criteria of the HEAL and MPDA baselines
(``opencood/loss/point_pillar_pyramid_loss.py:12-103``, ``opencood/loss/point_pillar_mpda_loss.py:16-157``), as components: the model
shells that would resolve them from ``loss.core_method`` are not built, and until they are no module of the reference's names exists
here.

Both are the detection-head terms this package already computes in one launch (``gencomm_head_loss``) plus one new term each:

    PointPillarPyramidLoss   + sum over the pyramid levels of weight_i * focal(occ_i, labels max-pooled by relative_downsample_i) / B
                             (``gencomm_pyramid_occ_loss``: every level, value and gradient, two launches; the level labels are formed
                             from pos_equal_one / neg_equal_one inside the kernels and never stored)
    PointPillarMPDALoss      + 2 * mean(BCE-with-logits(da_feature, [agent is the first of its scene]))
                             (``gencomm_domain_bce_loss``, two launches; the reference adds the term twice, :146 and :150, and logs it once)

The new terms are differentiable in their logits: the launch that computes the value writes the gradient, the backward is one
multiply by the incoming scalar (the pattern of ``_HeadLossFn``); a second derivative raises. There is no composition of framework
operators behind them: CPU tensors are refused. As everywhere in this package ``loss_dict`` holds detached device scalars, converted
when ``logging`` prints.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .point_pillar_depth_loss import PointPillarDepthLoss
from .point_pillar_gencomm_loss import PointPillarGencommLoss
from .runtime import f32c, ptr, record_len_list, require_gpu, stream_ptr

MAX_LEVELS = 4


class _OccLossFn(torch.autograd.Function):
    """``calc_occ_loss`` over every level. Returns (total, per-level losses [levels]); the second is for logging (not differentiable)."""

    @staticmethod
    def forward(ctx, pos, neg, cfg, *occ):
        ks, weights, pcw, gamma, alpha = cfg
        L = len(occ)
        B, H, W, A = pos.shape
        dev = pos.device
        sizes = [o.numel() for o in occ]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        sums = torch.empty(5 + 8 * B, dtype=torch.float64, device=dev)
        offs = [sum(sizes[:i]) for i in range(L)]
        _lib.check(_lib.lib().gencomm_pyramid_occ_loss(
            ptr(pos), ptr(neg), (C.c_void_p * L)(*[ptr(o) for o in occ]), (C.c_void_p * L)(*[flat.data_ptr() + 4 * o for o in offs]),
            (C.c_int * L)(*ks), (C.c_float * L)(*weights), L, B, H, W, A, float(pcw), float(gamma), float(alpha), sums.data_ptr(),
            stream_ptr(dev)), "gencomm_pyramid_occ_loss")
        out = sums[:1 + L].float()
        ctx.save_for_backward(flat)
        ctx.shapes, ctx.offs = [o.shape for o in occ], offs
        levels = out[1:]
        ctx.mark_non_differentiable(levels)
        return out[0], levels

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _levels):
        (flat,) = ctx.saved_tensors
        flat = flat * g
        return (None, None, None) + tuple(flat[o:o + s.numel()].view(s) for o, s in zip(ctx.offs, ctx.shapes))


class _DomainBceFn(torch.autograd.Function):
    """mean(BCE-with-logits(x, target)) with target 1 on the agents in `sources`, 0 elsewhere."""

    @staticmethod
    def forward(ctx, x, sources):
        N, Cc, H, W = x.shape
        grad = torch.empty_like(x)
        sums = torch.empty(1 + 32 * N, dtype=torch.float64, device=x.device)
        _lib.check(_lib.lib().gencomm_domain_bce_loss(ptr(x), (C.c_int * max(1, len(sources)))(*sources), len(sources), ptr(grad), sums.data_ptr(),
                                                      N, Cc, H, W, stream_ptr(x.device)), "gencomm_domain_bce_loss")
        ctx.save_for_backward(grad)
        return sums[:1].float()[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def pyramid_occ_loss(occ_list: Sequence[torch.Tensor], pos_equal_one: torch.Tensor, neg_equal_one: torch.Tensor,
                     relative_downsample: Sequence[int], weight: Sequence[float], pos_cls_weight: float, gamma: float, alpha: float):
    """``calc_occ_loss`` (point_pillar_pyramid_loss.py:69-103): occ_list[i] [B, 1, H // k_i, W // k_i] logits, pos / neg_equal_one
    [B, H, W, A] (A >= 2; anchors 0 and 1 are read) -> (total, per-level losses [levels]); the total is differentiable in every occ map."""
    for t in (pos_equal_one, neg_equal_one, *occ_list):
        require_gpu(t, "pyramid_occ_loss")
    L = len(occ_list)
    if not 1 <= L <= MAX_LEVELS or L > len(relative_downsample) or L > len(weight):
        raise ValueError(f"pyramid_occ_loss: {L} occupancy maps for relative_downsample {list(relative_downsample)} and weight {list(weight)} "
                         f"(1..{MAX_LEVELS} levels)")
    if pos_equal_one.dim() != 4 or pos_equal_one.shape[-1] < 2 or neg_equal_one.shape != pos_equal_one.shape:
        raise ValueError(f"pyramid_occ_loss: pos_equal_one / neg_equal_one must be [B, H, W, A >= 2] and alike, got {tuple(pos_equal_one.shape)} "
                         f"and {tuple(neg_equal_one.shape)}")
    B, H, W, _ = pos_equal_one.shape
    ks = [int(k) for k in relative_downsample[:L]]
    for i, (o, k) in enumerate(zip(occ_list, ks)):
        if k < 1 or k > min(H, W):
            raise ValueError(f"pyramid_occ_loss: level {i}: relative_downsample {k} outside 1..{min(H, W)}")
        if o.dim() != 4 or o.shape[0] != B:
            raise ValueError(f"pyramid_occ_loss: level {i}: occupancy map {tuple(o.shape)} for a batch of {B} label maps")
        if tuple(o.shape) != (B, 1, H // k, W // k):
            raise ValueError(f"pyramid_occ_loss: level {i}: occupancy map must be {(B, 1, H // k, W // k)} (labels {H} x {W} pooled by {k}, "
                             f"floored), got {tuple(o.shape)}")
    cfg = (ks, [float(w) for w in weight[:L]], pos_cls_weight, gamma, alpha)
    return _OccLossFn.apply(f32c(pos_equal_one), f32c(neg_equal_one), cfg, *[f32c(o) for o in occ_list])


def source_index(record_len) -> List[int]:
    """The first agent of every scene: 0, cumsum(record_len)[:-1] (point_pillar_mpda_loss.py:248-256)."""
    idx, s = [], 0
    for n in record_len_list(record_len):
        idx.append(s)
        s += n
    return idx


def domain_bce_loss(da_feature: torch.Tensor, record_len):
    """mean(BCE-with-logits) of the domain classifier's logits [N, C, H, W] against 1 on the first agent of every scene and 0 on
    the others (point_pillar_mpda_loss.py:129-144); differentiable in da_feature."""
    require_gpu(da_feature, "domain_bce_loss")
    if da_feature.dim() != 4:
        raise ValueError(f"domain_bce_loss: da_feature must be [N, C, H, W], got {tuple(da_feature.shape)}")
    src = source_index(record_len)
    if sum(record_len_list(record_len)) != da_feature.shape[0]:
        raise ValueError(f"domain_bce_loss: record_len {record_len_list(record_len)} for {da_feature.shape[0]} agent maps")
    return _DomainBceFn.apply(f32c(da_feature), src)


class PointPillarPyramidLoss(PointPillarDepthLoss):  # point_pillar_pyramid_loss.py:12-103
    def __init__(self, args):
        super().__init__(args)
        self.pyramid = args["pyramid"]
        self.relative_downsample = self.pyramid["relative_downsample"]
        self.pyramid_weight = self.pyramid["weight"]
        self.num_levels = len(self.relative_downsample)

    def calc_occ_loss(self, occ_single_list, positives, negatives, batch_size=None):
        if batch_size is not None and batch_size != positives.shape[0]:
            raise ValueError(f"PointPillarPyramidLoss: batch_size {batch_size} for {positives.shape[0]} label maps")
        total, self.level_losses = pyramid_occ_loss(occ_single_list, positives, negatives, self.relative_downsample, self.pyramid_weight,
                                                    self.pos_cls_weight, self.cls["gamma"], self.cls["alpha"])
        return total

    def forward(self, output_dict, target_dict, suffix=""):
        kind = output_dict["pyramid"]
        if kind == "collab":                                    # intermediate fusion (:46-66)
            if suffix == "":
                return super().forward(output_dict, target_dict)
            if suffix != "_single":
                raise ValueError(f"PointPillarPyramidLoss: suffix {suffix!r} with pyramid 'collab' (\"\" or \"_single\")")
            total = self.calc_occ_loss(output_dict["occ_single_list"], target_dict["pos_equal_one"], target_dict["neg_equal_one"])
            self.loss_dict = {"pyramid_loss": total.detach(), "total_loss": total.detach()}
            return total
        if kind == "single":                                    # late fusion (:30-44)
            for t in (target_dict["pos_equal_one"], *output_dict["occ_single_list"]):
                require_gpu(t, "PointPillarPyramidLoss")
            total = super().forward(output_dict, target_dict, suffix)
            occ = self.calc_occ_loss(output_dict["occ_single_list"], target_dict["pos_equal_one"], target_dict["neg_equal_one"])
            total = total + occ
            self.loss_dict.update({"pyramid_loss": occ.detach(), "total_loss": total.detach()})
            return total
        raise ValueError(f"PointPillarPyramidLoss: output_dict['pyramid'] is {kind!r} ('collab' or 'single')")

    def logging(self, epoch, batch_id, batch_len, writer=None, suffix="", iter=None):  # point_pillar_pyramid_loss.py:108-158 (no wandb)
        d = {k: float(v) for k, v in self.loss_dict.items()}
        print("[epoch %d][%d/%d]%s || Loss: %.4f || Conf Loss: %.4f || Loc Loss: %.4f || Dir Loss: %.4f || IoU Loss: %.4f || Depth Loss: %.4f"
              " || Pyramid Loss: %.4f" % (epoch, batch_id + 1, batch_len, suffix, d.get("total_loss", 0), d.get("cls_loss", 0), d.get("reg_loss", 0),
                                          d.get("dir_loss", 0), d.get("iou_loss", 0), d.get("depth_loss", 0), d.get("pyramid_loss", 0)))
        if writer is not None:
            for tag, key in (("Regression_loss", "reg_loss"), ("Confidence_loss", "cls_loss"), ("Dir_loss", "dir_loss"), ("Iou_loss", "iou_loss"),
                             ("Depth_loss", "depth_loss"), ("Pyramid_loss", "pyramid_loss")):
                writer.add_scalar(tag + suffix, d.get(key, 0), epoch * batch_len + batch_id)
        return d


class PointPillarMPDALoss(nn.Module):  # point_pillar_mpda_loss.py:16-157
    def __init__(self, args):
        super().__init__()
        if "iou" in args:
            raise NotImplementedError("loss.args.iou (IoU head supervision) is outside this build (no shipped yaml sets it)")
        head_args = {k: args[k] for k in ("pos_cls_weight", "cls", "reg")}
        if "dir" in args:
            head_args["dir"] = args["dir"]
        self.heads = _HeadTerms(head_args)                      # `depth` is accepted and ignored, as in the reference
        self.pos_cls_weight, self.cls, self.reg, self.dir = self.heads.pos_cls_weight, self.heads.cls, self.heads.reg, self.heads.dir
        self.da = args.get("da", False)
        self.loss_dict = {}

    def forward(self, output_dict, target_dict, suffix="", validate=False):
        for t in (target_dict["pos_equal_one"], output_dict.get(f"psm{suffix}"), output_dict.get(f"cls_preds{suffix}")):
            if t is not None:
                require_gpu(t, "PointPillarMPDALoss")
        for short, full in (("psm", "cls_preds"), ("rm", "reg_preds"), ("dm", "dir_preds")):   # :64-70 "rename variable"
            if f"{short}{suffix}" in output_dict:
                output_dict[f"{full}{suffix}"] = output_dict[f"{short}{suffix}"]
        # the batch size is the label maps' (:54): record_len, which this dict carries for the domain term, does not enter the head terms
        heads = {k: v for k, v in output_dict.items() if k not in ("record_len", "batch_size")}
        total = self.heads._head_terms(heads, target_dict, suffix)
        parts = self.heads.loss_dict
        if self.da and not validate:
            da = domain_bce_loss(output_dict["da_feature"], output_dict["record_len"])
            total = total + da + da                             # :146 and :150
        else:
            da = torch.zeros((), dtype=total.dtype, device=total.device)
        if "dir_loss" in parts:
            self.loss_dict["dir_loss"] = parts["dir_loss"]
        self.loss_dict.update({"total_loss": total.detach(), "reg_loss": parts["reg_loss"], "cls_loss": parts["cls_loss"], "da_loss": da.detach()})
        return total

    def logging(self, epoch, batch_id, batch_len, writer=None, suffix="", iter=None):  # point_pillar_mpda_loss.py:204-246 (no wandb)
        d = {k: float(v) for k, v in self.loss_dict.items()}
        print("[epoch %d][%d/%d]%s || Loss: %.4f || Conf Loss: %.4f || Loc Loss: %.4f || Dir Loss: %.4f || IoU Loss: %.4f || Da Loss: %.4f" % (
            epoch, batch_id + 1, batch_len, suffix, d.get("total_loss", 0), d.get("cls_loss", 0), d.get("reg_loss", 0), d.get("dir_loss", 0),
            d.get("iou_loss", 0), d.get("da_loss", 0)))
        if writer is not None:
            for tag, key in (("Regression_loss", "reg_loss"), ("Confidence_loss", "cls_loss"), ("Dir_loss", "dir_loss"), ("Iou_loss", "iou_loss")):
                writer.add_scalar(tag + suffix, d.get(key, 0), epoch * batch_len + batch_id)
        return d


class _HeadTerms(PointPillarGencommLoss):
    """cls + reg + dir of ``PointPillarGencommLoss`` alone (``_head_terms``: the one-launch form on float32 GPU maps)."""
    with_generation = False

    def __init__(self, args):
        super().__init__(dict(args, generate_weight=None))
