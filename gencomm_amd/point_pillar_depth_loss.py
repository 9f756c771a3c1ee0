"""``PointPillarDepthLoss`` -- the criterion of the camera baselines (``opencood/loss/point_pillar_depth_loss.py:11-59`` on top of
``point_pillar_loss.py:15-126``), resolved by the reference's ``create_loss`` from ``loss.core_method: point_pillar_depth_loss``
(``train_utils.py:304-323``: module name, lower-cased class name); 157 reference yamls name it, every stage-1 camera baseline among them.

    total = cls + reg + dir                                            (the head terms of ``PointPillarGencommLoss``: one launch)
          + depth.weight * mean(FocalLoss(depth_logit, depth_gt_indices))   for every ``depth_items{suffix}*`` key (one launch each)

``loss_dict`` reports ``depth_loss``; as in the reference (``:56-57``) the logged ``total_loss`` is the sum of the head terms.
"""
from __future__ import annotations

from .point_pillar_gencomm_loss import PointPillarGencommLoss


class PointPillarDepthLoss(PointPillarGencommLoss):
    with_generation = False

    def __init__(self, args):
        super().__init__(dict(args, generate_weight=None))
        if self.depth is None:
            raise KeyError("loss.args.depth")           # the reference reads args['depth'] unconditionally (:14)

    def logging(self, epoch, batch_id, batch_len, writer=None, suffix="", iter=None):  # point_pillar_depth_loss.py:62-100 (no wandb)
        d = {k: float(v) for k, v in self.loss_dict.items()}
        print("[epoch %d][%d/%d]%s || Loss: %.4f || Conf Loss: %.4f || Loc Loss: %.4f || Dir Loss: %.4f || IoU Loss: %.4f || Depth Loss: %.4f" % (
            epoch, batch_id + 1, batch_len, suffix, d.get("total_loss", 0), d.get("cls_loss", 0), d.get("reg_loss", 0), d.get("dir_loss", 0),
            d.get("iou_loss", 0), d.get("depth_loss", 0)))
        if writer is not None:
            for tag, key in (("Regression_loss", "reg_loss"), ("Confidence_loss", "cls_loss"), ("Dir_loss", "dir_loss"), ("Iou_loss", "iou_loss"),
                             ("Depth_loss", "depth_loss")):
                writer.add_scalar(tag + suffix, d.get(key, 0), epoch * batch_len + batch_id)
        return d
