"""gencomm_amd -- MI355X (gfx950) implementation of GenComm's generative-communication hot path.

Public surface mirrors the reference's plugin API:

    GenComm(model_cfg)                 opencood/models/gencomm_modules/cond_diff.py:185
    DiffusionUNet(config)              opencood/models/gencomm_modules/unet.py:198
    Enhancer(C, win_size, num_heads)   opencood/models/gencomm_modules/enhancer.py:359
    AttFusion(feature_dims)            opencood/models/fuse_modules/fusion_in_one.py:126
    MaxFusion()                        opencood/models/fuse_modules/fusion_in_one.py:87 (fusion_method: max)
    Who2comFusion(feature_dims)        opencood/models/fuse_modules/fusion_in_one.py:521 (fusion_method: who2com)
    CoBEVT(args)                       opencood/models/fuse_modules/fusion_in_one.py:409 (fusion_method: cobevt; trainable=True trains)
    V2VNetFusion(args)                 opencood/models/fuse_modules/fusion_in_one.py:238 (the v2vnet block; a component; trainable=True trains)
    regroup, normalize_pairwise_tfm    fusion_in_one.py:48, opencood/utils/transformation_utils.py:68
    MessageExtractorv2(in_ch, out_ch)  opencood/models/gencomm_modules/message_extractor_v2.py:109
    LiftSplatShoot(args)               opencood/models/heter_encoders.py:83 (camera_encoder: Resnet101; trainable=True trains it)
    PointPillarDepthLoss(args)         opencood/loss/point_pillar_depth_loss.py:11 (loss.core_method: point_pillar_depth_loss)
    UMGMQuantizer(channel, m, k, ...)  opencood/models/sub_modules/codebook.py:280 (the CodeFilling codebook codec; a component, inference)
    Adapter(args), Reverter(args)      opencood/models/stamp_modules/adapter.py:759, :783 (STAMP's adapter / reverter; components, inference)
    PyramidFusion(model_cfg)           opencood/models/fuse_modules/pyramid_fuse.py:65 (HEAL's pyramid backbone + fusion; a component, inference)
    weighted_fuse(x, score, ...)       opencood/models/fuse_modules/pyramid_fuse.py:17
    MPDAAlign(args)                    opencood/models/heter_model_baseline_w_mpda.py:232-262 (MPDA's feature aligner; a component; trainable=True: training on mpda_bwd.py), with
    LearnableResizer, SwapFusionEncoder, CrossDomainFusionEncoder, DAImgHead   opencood/models/mpda_modules/
    PointPillarPyramidLoss(args)       opencood/loss/point_pillar_pyramid_loss.py:12 (HEAL's criterion; a component, in baseline_criteria.py)
    PointPillarMPDALoss(args)          opencood/loss/point_pillar_mpda_loss.py:16 (MPDA's criterion; a component, in baseline_criteria.py)

All compute runs in hand-written HIP kernels behind the C ABI of ``include/gencomm_hip.h``.
"""
from .baseline_criteria import PointPillarMPDALoss, PointPillarPyramidLoss
from .cobevt import CoBEVT
from .codebook import UMGMQuantizer
from .cond_diff import GenComm
from .enhancer import Enhancer
from .fusion import AttFusion, MaxFusion, normalize_pairwise_tfm, regroup
from .lift_splat_shoot import LiftSplatShoot
from .message_extractor import MessageExtractorv2
from .point_pillar_depth_loss import PointPillarDepthLoss
from .mpda import CrossDomainFusionEncoder, DAImgHead, LearnableResizer, MPDAAlign, SwapFusionEncoder
from .pyramid_fuse import PyramidFusion, weighted_fuse
from .stamp_adapter import Adapter, Reverter
from .unet import DiffusionUNet
from .v2vnet import V2VNetFusion
from .who2com import Who2comFusion



def set_denoise_dtype(dtype) -> None:
    """Arithmetic of the denoise loop, process-wide (``gencomm_set_mode(GENCOMM_MODE_ARITH, ...)``):
    ``torch.float32`` (default: fp32 tensors, fp32-grade products on the f16 matrix pipe), ``"exact_fp32"`` (exact-fp32 MFMA
    kernels) or ``torch.bfloat16`` (bf16 storage of the UNet's 8-channel maps and single bf16 products -- the analogue of the
    reference's ``--half`` / autocast runs, ``train_ddp.py:139-141``; inference only)."""
    import torch
    from . import _lib
    value = {torch.float32: 0, "float32": 0, "exact_fp32": 1, torch.bfloat16: 2, "bfloat16": 2, "bf16": 2}[dtype]
    _lib.check(_lib.lib().gencomm_set_mode(_lib.MODE_ARITH, value), "gencomm_set_mode")


__all__ = ["GenComm", "DiffusionUNet", "Enhancer", "AttFusion", "MaxFusion", "Who2comFusion", "CoBEVT", "V2VNetFusion", "UMGMQuantizer", "Adapter", "Reverter", "PyramidFusion", "weighted_fuse", "MPDAAlign", "LearnableResizer", "SwapFusionEncoder", "CrossDomainFusionEncoder", "DAImgHead", "MessageExtractorv2", "LiftSplatShoot", "PointPillarDepthLoss", "PointPillarPyramidLoss", "PointPillarMPDALoss", "regroup", "normalize_pairwise_tfm",
           "set_denoise_dtype"]
