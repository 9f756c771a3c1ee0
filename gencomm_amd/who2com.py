"""``Who2comFusion`` -- host-side mirror of ``opencood/models/fuse_modules/fusion_in_one.py:521-574``: the ego row of the parameter-free
per-pixel attention over the warped agents (exactly ``AttFusion``), concatenated behind the ego's own (unwarped) map, then one 3x3
convolution 2C -> C (``decode_layer``). Same constructor argument, attribute names and ``state_dict`` keys (``decode_layer.weight``,
``decode_layer.bias``; ``att`` has no parameters).

Everything runs on kernels the library already has, forward and backward:
  attention            gencomm_warp_attfuse_fwd / _bwd (``AttFusion`` / ``autograd.AttFusionFunction``)
  decode_layer         the general convolution (``HipConv2d``: gencomm_conv2d_fwd; backward ``bev_backbone._conv_backward``)
The ego-row gather and the concatenation are framework operators, so autograd adds the ego branch's gradient to the first agent of
each scene."""
from __future__ import annotations

from collections.abc import Mapping

import torch

from .bev_backbone import HipConv2d
from .fusion import AttFusion
from .runtime import f32c, record_len_list, require_gpu


class Who2comFusion(AttFusion):
    def __init__(self, feature_dims):
        """``feature_dims``: the channel count. The reference's shells pass ``args['who2com']`` itself
        (heter_model_baseline_w_gencomm_stage1.py:127-128), so a yaml writes ``who2com: 128``; a mapping ``{feat_dim: 128}`` (the
        spelling of the ``att`` block) is accepted as well."""
        if isinstance(feature_dims, Mapping):
            if "feat_dim" not in feature_dims:
                raise KeyError(f"who2com: a mapping needs 'feat_dim', got {dict(feature_dims)!r}")
            feature_dims = feature_dims["feat_dim"]
        if isinstance(feature_dims, bool) or not isinstance(feature_dims, int) or feature_dims < 1:
            raise TypeError(f"who2com: feature_dims must be a positive int (or a mapping with 'feat_dim'), got {feature_dims!r}")
        super().__init__(feature_dims)   # self.att: the non-learning attention (fusion_in_one.py:524-525)
        self.decode_layer = HipConv2d(feature_dims * 2, feature_dims, kernel_size=3, stride=1, padding=1)

    def forward(self, x, record_len, affine_matrix):
        """x [sumN, C, H, W], record_len [B], affine_matrix [B, L, L, 2, 3] -> [B, C, H, W]."""
        require_gpu(x, "Who2comFusion.forward")
        lens = record_len_list(record_len)
        if x.shape[1] * 2 != self.decode_layer.in_channels:
            raise ValueError(f"Who2comFusion was built for {self.decode_layer.in_channels // 2} channels, got {x.shape[1]}")
        x = f32c(x)
        attended = AttFusion.forward(self, x, lens, affine_matrix)   # validates record_len; [B, C, H, W]
        ego, o = [], 0
        for k in lens:                                               # batch_node_features[b][0], not warped (fusion_in_one.py:561); slices:
            ego.append(x[o:o + 1])                                   # an index list would be copied to the device on every call
            o += k
        return self.decode_layer(torch.cat((torch.cat(ego), attended), dim=1))
