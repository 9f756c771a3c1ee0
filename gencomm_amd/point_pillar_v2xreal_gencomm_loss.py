"""``PointPillarV2XRealGenCommLoss`` -- the training criterion of the V2X-Real GenComm stage-1 recipes
(``opencood/loss/point_pillar_v2xreal_gencomm_loss.py``), resolved by the reference's ``create_loss`` from
``loss.core_method: point_pillar_v2xreal_gencomm_loss``.  The head terms are ``PointPillarV2XRealLoss``'s (two launches of the library on
the GPU); this adds ``generate_weight * MSE(gt_feature, pred_feature)`` (:147-159) through ``F.mse_loss``, as the OPV2V criterion does.
"""
from __future__ import annotations

import torch.nn.functional as F

from .point_pillar_v2xreal_loss import PointPillarV2XRealLoss


class PointPillarV2XRealGenCommLoss(PointPillarV2XRealLoss):
    def __init__(self, args):
        super().__init__(args)
        self.generate_weight = args["generate_weight"]

    def forward(self, output_dict, target_dict):
        total, (conf_loss, reg_loss) = self.head_losses(output_dict, target_dict)
        gen_loss = F.mse_loss(output_dict["gt_feature"], output_dict["pred_feature"])
        total = total + self.generate_weight * gen_loss
        g = gen_loss.detach()
        self.loss_dict = {"generate_loss": g, "total_loss": total.detach(), "reg_loss": reg_loss.detach(), "conf_loss": conf_loss.detach(),
                          "gen_loss": g}
        return total

    def _line(self, epoch, batch_id, batch_len, d):   # :250-263
        return ("[epoch %d][%d/%d], || Loss: %.4f || Conf Loss: %.4f || Loc Loss: %.4f || Gen Loss: %.4f" % (
            epoch, batch_id + 1, batch_len, d["total_loss"], d["conf_loss"], d["reg_loss"], d["gen_loss"]))
