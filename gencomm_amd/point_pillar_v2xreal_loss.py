"""``PointPillarV2XRealLoss`` -- the training criterion of the V2X-Real stage-2 recipes (``opencood/loss/point_pillar_v2xreal_loss.py``),
resolved by the reference's ``create_loss`` from ``loss.core_method: point_pillar_v2xreal_loss`` (``train_utils.py:304-323``: module name,
lower-cased class name).  ``point_pillar_v2xreal_gencomm_loss.py`` adds the generate term for the stage-1 recipes.

    conf = cls_weight * sigmoid focal loss (alpha 0.25, gamma 2) over the one-hot of the slot's label value, / #positives / B
    reg  = reg * smooth-L1 (beta 1/9) on the sin-difference encoding, positives only, NaN targets ignored, / #positives / B
    total = reg + conf

Layouts: cls_preds [B, S*K, H, W], reg_preds [B, 7S, H, W], labels ``pos_equal_one`` [B, H, W, S] (-1 ignore, 0 background, 1..K class)
and ``targets`` [B, H, W, S, 7] as ``generate_label_v2xreal`` / ``collate_batch_v2xreal`` produce them (float64: the collate keeps numpy's
dtype), S = anchor rotations x K class blocks.  On the GPU the two head terms and their gradients are two launches of the library
(``gencomm_head_loss_mc``, ``csrc/loss_kernels.h``: a per-sample count of the positives, then the loss); the framework-operator
composition below (the reference's arithmetic, :88-160 with :12-70, :168-233) is kept for CPU tensors and other layouts.  Nothing here
synchronises the host: ``loss_dict`` holds detached device scalars that ``logging`` converts when it prints.  The reference's regression
term runs in the targets' dtype (float32 predictions promote), so the returned total is float64 for float64 targets, as there.
"""
from __future__ import annotations

import torch
import torch.nn as nn

ALPHA, GAMMA, BETA = 0.25, 2.0, 1.0 / 9.0   # point_pillar_v2xreal_loss.py:78-79 (hard-coded), :21 (WeightedSmoothL1Loss default)
MAX_CLASSES = 8                             # the kernel's bound on K (csrc/loss_kernels.h, kLossMcMaxClasses)


def sigmoid_focal_loss(preds, targets, weights):  # cls_loss_func + sigmoid_cross_entropy_with_logits (:168-219)
    p = torch.sigmoid(preds)
    alpha_weight = targets * ALPHA + (1 - targets) * (1 - ALPHA)
    pt = targets * (1.0 - p) + (1.0 - targets) * p
    bce = torch.clamp(preds, min=0) - preds * targets + torch.log1p(torch.exp(-torch.abs(preds)))
    return alpha_weight * torch.pow(pt, GAMMA) * bce * weights.unsqueeze(-1)


def weighted_smooth_l1_loss(preds, targets, weights):  # WeightedSmoothL1Loss.forward (:36-70)
    targets = torch.where(torch.isnan(targets), preds, targets)   # ignore NaN targets
    n = torch.abs(preds - targets)
    return torch.where(n < BETA, 0.5 * n ** 2 / BETA, n - 0.5 * BETA) * weights.unsqueeze(-1)


def add_sin_difference(b1, b2, dim=6):  # :221-233 (float32 predictions and float64 targets promote to float64 here)
    s = torch.sin(b1[..., dim:dim + 1]) * torch.cos(b2[..., dim:dim + 1])
    t = torch.cos(b1[..., dim:dim + 1]) * torch.sin(b2[..., dim:dim + 1])
    return torch.cat([b1[..., :dim], s, b1[..., dim + 1:]], -1), torch.cat([b2[..., :dim], t, b2[..., dim + 1:]], -1)


class _HeadLossMcFn(torch.autograd.Function):
    """conf + reg loss of the multi-class head maps in two launches of the library (``gencomm_head_loss_mc``: forward values and the
    gradients of their sum) and -- in the backward -- one multiply by the incoming scalar.  Returns (sum, [conf, reg]) in the targets'
    dtype; the parts are for logging (not differentiable)."""

    @staticmethod
    def forward(ctx, cls, reg, lab, tgt, K, cls_weight, reg_weight):
        from . import _lib
        from .runtime import ptr, stream_ptr, zeros as pool_zeros
        B, SK, H, W = cls.shape
        dev = cls.device
        n1, n2 = cls.numel(), reg.numel()
        flat = torch.empty(n1 + n2, dtype=torch.float32, device=dev)
        count = pool_zeros(B, torch.int32, dev)
        sums = pool_zeros(3, torch.float64, dev)
        _lib.check(_lib.lib().gencomm_head_loss_mc(ptr(cls), ptr(reg), ptr(lab), ptr(tgt), int(tgt.dtype == torch.float64), ptr(count),
                                                   flat.data_ptr(), flat.data_ptr() + 4 * n1, sums.data_ptr(), B, SK // K, K, H, W,
                                                   float(cls_weight), float(reg_weight), stream_ptr(dev)), "gencomm_head_loss_mc")
        out = sums if tgt.dtype == torch.float64 else sums.float()   # float32 targets: the reference's arithmetic is float32 throughout
        ctx.save_for_backward(flat)
        ctx.shapes = (cls.shape, reg.shape)
        parts = out[:2]
        ctx.mark_non_differentiable(parts)
        return out[2], parts

    @staticmethod
    def backward(ctx, g, _parts):
        (flat,) = ctx.saved_tensors
        s1, s2 = ctx.shapes
        flat = flat * g      # a 0-dim float64 g does not promote the float32 gradient
        return flat[:s1.numel()].view(s1), flat[s1.numel():].view(s2), None, None, None, None, None


class PointPillarV2XRealLoss(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.num_class = args["num_class"]
        self.cls_weight = args["cls_weight"]
        self.reg_coe = args["reg"]
        self.fuse_heads = True      # False: always the composition of framework operators (tests compare the two)
        self.loss_dict = {}

    def _check_shapes(self, psm, rm, labels, targets):
        K = self.num_class
        if psm.dim() != 4 or psm.shape[1] % K:
            raise ValueError(f"cls_preds {tuple(psm.shape)}: expected [B, S*K, H, W] with K = num_class = {K}")
        B, SK, H, W = psm.shape
        S = SK // K
        if tuple(rm.shape) != (B, 7 * S, H, W):
            raise ValueError(f"reg_preds {tuple(rm.shape)} does not match cls_preds {tuple(psm.shape)}: expected {(B, 7 * S, H, W)}")
        if labels.numel() != B * H * W * S:
            raise ValueError(f"pos_equal_one {tuple(labels.shape)} does not hold B*H*W*S = {B * H * W * S} labels "
                             f"for cls_preds {tuple(psm.shape)}")
        if targets.numel() != 7 * labels.numel():
            raise ValueError(f"targets {tuple(targets.shape)} does not hold 7 codes per label of pos_equal_one {tuple(labels.shape)}")

    def _fused_heads(self, psm, rm, labels, targets):
        """(conf + reg, [conf, reg]) from the library when the maps are float32 GPU tensors and labels / targets share a float dtype on
        the GPU; None otherwise and the composition runs."""
        if not self.fuse_heads or self.num_class > MAX_CLASSES:
            return None
        if not all(t.is_cuda for t in (psm, rm, labels, targets)) or psm.dtype != torch.float32 or rm.dtype != torch.float32:
            return None
        if labels.dtype not in (torch.float32, torch.float64) or targets.dtype != labels.dtype:
            return None
        c = lambda t: t if t.is_contiguous() else t.contiguous()
        return _HeadLossMcFn.apply(c(psm), c(rm), c(labels), c(targets), self.num_class, self.cls_weight, self.reg_coe)

    def _composed_heads(self, psm, rm, labels, targets):
        """The reference's arithmetic (point_pillar_v2xreal_loss.py:88-143) as framework operators."""
        B = psm.shape[0]
        cls_preds = psm.permute(0, 2, 3, 1).contiguous()
        box_cls_labels = labels.reshape(B, -1)
        cared = box_cls_labels >= 0
        positives = box_cls_labels > 0
        negatives = box_cls_labels == 0
        cls_weights = (negatives * 1.0 + 1.0 * positives).float()
        reg_weights = positives.float()
        pos_normalizer = positives.sum(1, keepdim=True).float()
        reg_weights = reg_weights / torch.clamp(pos_normalizer, min=1.0)
        cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)
        cls_targets = box_cls_labels * cared.type_as(box_cls_labels)
        one_hot = torch.zeros(*cls_targets.shape, self.num_class + 1, dtype=cls_preds.dtype, device=cls_targets.device)
        one_hot.scatter_(-1, cls_targets.unsqueeze(-1).long(), 1.0)
        cls_preds = cls_preds.view(B, -1, self.num_class)
        conf_loss = sigmoid_focal_loss(cls_preds, one_hot[..., 1:], cls_weights).sum() / B * self.cls_weight

        rm = rm.permute(0, 2, 3, 1).contiguous().view(B, -1, 7)
        bp, bt = add_sin_difference(rm, targets.reshape(B, -1, 7))
        reg_loss = weighted_smooth_l1_loss(bp, bt, reg_weights).sum() / B * self.reg_coe
        return reg_loss + conf_loss, (conf_loss, reg_loss)

    def head_losses(self, output_dict, target_dict):
        psm, rm = output_dict["cls_preds"], output_dict["reg_preds"]
        labels, targets = target_dict["pos_equal_one"], target_dict["targets"]
        self._check_shapes(psm, rm, labels, targets)
        fused = self._fused_heads(psm, rm, labels, targets)
        return fused if fused is not None else self._composed_heads(psm, rm, labels, targets)

    def forward(self, output_dict, target_dict):
        total, (conf_loss, reg_loss) = self.head_losses(output_dict, target_dict)
        self.loss_dict = {"total_loss": total.detach(), "reg_loss": reg_loss.detach(), "conf_loss": conf_loss.detach()}
        return total

    def _line(self, epoch, batch_id, batch_len, d):
        return ("[epoch %d][%d/%d], || Loss: %.4f || Conf Loss: %.4f || Loc Loss: %.4f" % (
            epoch, batch_id + 1, batch_len, d["total_loss"], d["conf_loss"], d["reg_loss"]))

    def logging(self, epoch, batch_id, batch_len, writer=None, pbar=None, iter=None):  # :235-258 (no swanlab)
        d = {k: float(v) for k, v in self.loss_dict.items()}   # the only host synchronisation of the criterion
        line = self._line(epoch, batch_id, batch_len, d)
        if pbar is None:
            print(line)
        else:
            pbar.set_description(line)
        if writer is not None:
            writer.add_scalar("Regression_loss", d["reg_loss"], epoch * batch_len + batch_id)
            writer.add_scalar("Confidence_loss", d["conf_loss"], epoch * batch_len + batch_id)
        return d
