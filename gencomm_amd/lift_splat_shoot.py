"""``LiftSplatShoot`` -- the camera encoder of the OPV2V-H camera modalities, ResNet-101 trunk (``camera_encoder: Resnet101``, the
``m4`` agents): host-side mirror of ``opencood/models/heter_encoders.py:83-241`` with ``CamEncode_Resnet101``
(``sub_modules/lss_submodule.py:140-233``). Same constructor arguments, ``forward(data_dict, modality_name)`` signature, output
``[B, C nz, ny, nx]`` and ``state_dict`` keys (``camencode.conv1.weight``, ``camencode.layer2.0.downsample.1.running_mean``,
``camencode.image_head.bias`` ...), so a reference checkpoint loads with ``strict=True``.

Every operation of ``forward`` is a HIP kernel behind the C ABI: the trunk (7x7 stride-2 stem, max-pool, the bottlenecks of
``layer1`` / ``layer2`` with folded eval BatchNorm and the fused identity + ReLU) and the heads on ``conv2d_hip``; the depth softmax,
geometry, sort and splat in ``gencomm_lss_splat_fwd`` (the ``depth (x) feature`` tensor is never formed); the depth targets of
``depth_supervision`` in ``gencomm_lss_depth_target_fwd``.

``LiftSplatShoot(args)`` is inference only (the GenComm stage-2 model freezes the encoders) and refuses a grad-enabled forward.
``LiftSplatShoot(args, trainable=True)`` trains (stage 1 of the reference trains every encoder from scratch): the trunk and heads run
through ``conv2d_hip``'s autograd paths (batch-statistics BatchNorm in ``.train()``; the 7x7 stem's weight gradient on
``gencomm_stem7x7_wgrad``, the max-pool's on ``gencomm_maxpool3x3s2_bwd``), the lift-splat through ``_LiftSplatFn``
(``gencomm_lss_splat_bwd``), and ``depth_items[0]`` stays attached to the graph for the depth term of the criteria. The images and the
camera matrices get no gradient.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .bev_backbone import conv2d_hip
from .runtime import f32c, ptr, require_gpu, stream_ptr, workspaces


def gen_dx_bx(xbound, ybound, zbound):   # camera_utils.py:129-134
    dx = torch.Tensor([row[2] for row in [xbound, ybound, zbound]])
    bx = torch.Tensor([row[0] + row[2] / 2.0 for row in [xbound, ybound, zbound]])
    nx = torch.LongTensor([(row[1] - row[0]) / row[2] for row in [xbound, ybound, zbound]])
    return dx, bx, nx


def depth_discretization(depth_min, depth_max, num_bins, mode):   # camera_utils.py:183-192
    if mode == "UD":
        bin_size = (depth_max - depth_min) / num_bins
        return depth_min + bin_size * np.arange(num_bins)
    if mode == "LID":
        bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
        return depth_min + bin_size * (np.arange(num_bins) * np.arange(1, 1 + num_bins)) / 2
    raise NotImplementedError(f"grid_conf.mode {mode!r}: UD and LID are supported")


class _MaxPoolFn(torch.autograd.Function):
    """maxpool3x3s2 with its HIP backward (``gencomm_maxpool3x3s2_bwd``: every window's gradient goes to its arg-max, torch's tie rule)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        with torch.no_grad():
            return maxpool3x3s2(x)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().gencomm_maxpool3x3s2_bwd(ptr(x), ptr(f32c(gy)), ptr(dx), n, c, h, w, stream_ptr(x.device)), "gencomm_maxpool3x3s2_bwd")
        return dx


def maxpool3x3s2(x: torch.Tensor) -> torch.Tensor:
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on the HIP kernel (differentiable: HIP backward)."""
    require_gpu(x, "maxpool3x3s2")
    x = f32c(x)
    if torch.is_grad_enabled() and x.requires_grad:
        return _MaxPoolFn.apply(x)
    n, c, h, w = x.shape
    y = torch.empty(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().gencomm_maxpool3x3s2_fwd(ptr(x), ptr(y), n, c, h, w, stream_ptr(x.device)), "gencomm_maxpool3x3s2_fwd")
    return y


class Bottleneck(nn.Module):   # torchvision.models.resnet.Bottleneck (stride on the 3x3 layer), the names of its state_dict
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x if self.downsample is None else conv2d_hip(x, self.downsample[0], self.downsample[1], relu=False)
        out = conv2d_hip(x, self.conv1, self.bn1, relu=True)
        out = conv2d_hip(out, self.conv2, self.bn2, relu=True)
        return conv2d_hip(out, self.conv3, self.bn3, relu=True, residual=identity)   # relu(bn3(conv3(out)) + identity)


def _make_layer(inplanes, planes, blocks, stride):
    downsample = None
    if stride != 1 or inplanes != planes * Bottleneck.expansion:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                                   nn.BatchNorm2d(planes * Bottleneck.expansion))
    layers = [Bottleneck(inplanes, planes, stride, downsample)]
    layers += [Bottleneck(planes * Bottleneck.expansion, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


class CamEncodeResnet101(nn.Module):
    """CamEncode_Resnet101 (lss_submodule.py:140-233): resnet101's conv1 / bn1 / maxpool / layer1 (3 blocks) / layer2 (4 blocks), then
    the 1x1 depth and image heads. ``forward`` returns (depth_logit [BN, D, fH, fW], image features [BN, C, fH, fW])."""

    def __init__(self, D, C, downsample, ddiscr, mode, use_gt_depth=False, depth_supervision=True):
        super().__init__()
        self.D, self.C, self.downsample = D, C, downsample
        self.d_min, self.d_max, self.num_bins = ddiscr[0], ddiscr[1], ddiscr[2]
        self.mode = mode
        self.use_gt_depth = use_gt_depth
        self.depth_supervision = depth_supervision
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = _make_layer(64, 64, 3, 1)
        self.layer2 = _make_layer(256, 128, 4, 2)
        self.layer3 = nn.Identity()
        self.depth_head = nn.Conv2d(512, self.D, kernel_size=1, padding=0)
        self.image_head = nn.Conv2d(512, self.C, kernel_size=1, padding=0)

    def trunk(self, x):
        x = conv2d_hip(x, self.conv1, self.bn1, relu=True)   # 7x7 stride 2 pad 3
        x = maxpool3x3s2(x)
        for blk in list(self.layer1) + list(self.layer2):
            x = blk(x)
        return x

    def forward(self, x):
        features = self.trunk(x)
        return conv2d_hip(features, self.depth_head), conv2d_hip(features, self.image_head)

    def depth_gt_indices(self, x):
        """get_gt_depth_dist's depth_gt_indices (eval mode) from channel 3 of x [BN, >= 4, H, W] -> int64 [BN, fH, fW]."""
        bn, cimg, h, w = x.shape
        ds = self.downsample
        out = torch.empty(bn, len(range(ds // 2, h, ds)), len(range(ds // 2, w, ds)), dtype=torch.int64, device=x.device)
        mode = {"UD": 0, "LID": 1}.get(self.mode)
        if mode is None:
            raise NotImplementedError(f"grid_conf.mode {self.mode!r}: depth targets support UD and LID")
        _lib.check(_lib.lib().gencomm_lss_depth_target_fwd(ptr(x), bn, cimg, h, w, ds, mode, float(self.d_min), float(self.d_max),
                                                           int(self.num_bins), ptr(out), None, stream_ptr(x.device)),
                   "gencomm_lss_depth_target_fwd")
        return out


class _LiftSplatFn(torch.autograd.Function):
    """``LiftSplatShoot.splat`` with gradients for depth_logit and feat. The forward is the same three launches plus the sort, on a
    workspace of its OWN (the per-device shared one would be overwritten by the next forward) that stays in the context together with
    the cells; the backward is ``gencomm_lss_splat_bwd``. The camera matrices get None (the reference's ``.long()`` cuts that path)."""

    @staticmethod
    def forward(ctx, depth_logit, feat, module, rots, trans, intrins, post_rots, post_trans):
        B, N = trans.shape[:2]
        D, fH, fW = module.frustum.shape[:3]
        Cc, dev = feat.shape[1], feat.device
        nbytes = _lib.check_size(_lib.lib().gencomm_lss_workspace_bytes(B, N, D, fH, fW, Cc, module._grid()[2]), "gencomm_lss_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out, cell = module.splat(depth_logit, feat, rots, trans, intrins, post_rots, post_trans, return_cells=True, workspace=ws)
        ctx.save_for_backward(ws, cell)
        ctx.module, ctx.dims = module, (B, N, D, fH, fW, Cc)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ws, cell = ctx.saved_tensors
        B, N, D, fH, fW, Cc = ctx.dims
        dev = grad_out.device
        l = _lib.lib()
        nx = ctx.module._grid()[2]
        nbytes = _lib.check_size(l.gencomm_lss_splat_bwd_workspace_bytes(B, Cc, nx), "gencomm_lss_splat_bwd_workspace_bytes")
        scratch = workspaces.get(dev, nbytes, "lss_bwd")
        g = f32c(grad_out)
        d_logit = torch.empty(B * N, D, fH, fW, dtype=torch.float32, device=dev)
        d_feat = torch.empty(B * N, Cc, fH, fW, dtype=torch.float32, device=dev)
        _lib.check(l.gencomm_lss_splat_bwd(ptr(g), ptr(ws), ws.numel(), ptr(cell), nx, B, N, D, fH, fW, Cc, ptr(d_logit), ptr(d_feat),
                                           ptr(scratch), scratch.numel(), stream_ptr(dev)), "gencomm_lss_splat_bwd")
        return d_logit, d_feat, None, None, None, None, None, None


class LiftSplatShoot(nn.Module):
    """heter_encoders.py:83-241 with ``camera_encoder: Resnet101``. ``forward(data_dict, modality_name)`` reads
    ``data_dict['inputs_<modality_name>']`` = {imgs [B, N, 4, H, W] (RGB + depth), rots, intrins, post_rots [B, N, 3, 3], trans,
    post_trans [B, N, 3]} and returns the BEV map [B, img_features * nz, ny, nx]; with ``depth_supervision`` it keeps
    ``self.depth_items = (depth_logit [B N, D, fH, fW], depth_gt_indices [B N, fH, fW] int64)`` as the reference does.
    ``trainable=True`` opts into the grad-enabled forward (HIP backward of every stage; ``depth_logit`` stays attached to the graph)."""

    def __init__(self, args, trainable=False):
        super().__init__()
        self.trainable = bool(trainable)
        self.grid_conf = args["grid_conf"]
        self.data_aug_conf = args["data_aug_conf"]
        self.camera_encoder_type = args["camera_encoder"]
        if self.camera_encoder_type == "EfficientNet":
            raise NotImplementedError("camera_encoder: EfficientNet (the m2 trunk: depthwise 3x3 / 5x5 stride-2 convolutions, squeeze-"
                                      "excitation, swish, bilinear Up blocks) is outside this build; camera_encoder: Resnet101 is supported")
        if self.camera_encoder_type != "Resnet101":
            raise NotImplementedError(f"camera_encoder: {self.camera_encoder_type!r} is not a reference camera encoder")
        if args.get("use_depth_gt", False):
            raise NotImplementedError("use_depth_gt: true (splatting the one-hot ground-truth depth) is outside this build; no shipped "
                                      "yaml sets it")
        dx, bx, nx = gen_dx_bx(self.grid_conf["xbound"], self.grid_conf["ybound"], self.grid_conf["zbound"])
        self.dx, self.bx, self.nx = dx, bx, nx                  # host constants (the reference pins them to cuda; this module does not)
        self.depth_supervision = args["depth_supervision"]
        self.downsample = args["img_downsample"]
        self.camC = args["img_features"]
        self.frustum = self.create_frustum()                    # [D, fH, fW, 3] float32, built on the host as the reference does
        self.use_quickcumsum = True
        self.D = self.frustum.shape[0]
        self.camencode = CamEncodeResnet101(self.D, self.camC, self.downsample, self.grid_conf["ddiscr"], self.grid_conf["mode"],
                                            args.get("use_depth_gt", False), args["depth_supervision"])
        self.depth_items = None
        self._dev_frustum = {}

    def create_frustum(self):   # heter_encoders.py:107-121
        ogfH, ogfW = self.data_aug_conf["final_dim"]
        fH, fW = ogfH // self.downsample, ogfW // self.downsample
        ds = torch.tensor(depth_discretization(*self.grid_conf["ddiscr"], self.grid_conf["mode"]), dtype=torch.float).view(-1, 1, 1).expand(-1, fH, fW)
        D, _, _ = ds.shape
        xs = torch.linspace(0, ogfW - 1, fW, dtype=torch.float).view(1, 1, fW).expand(D, fH, fW)
        ys = torch.linspace(0, ogfH - 1, fH, dtype=torch.float).view(1, fH, 1).expand(D, fH, fW)
        return torch.stack((xs, ys, ds), -1)

    def _grid(self):
        lo = (self.bx - self.dx / 2.0).numpy().astype(np.float32)   # float32 arithmetic, as voxel_pooling's (bx - dx / 2.)
        return ((C.c_float * 3)(*lo.tolist()), (C.c_float * 3)(*self.dx.numpy().astype(np.float32).tolist()),
                (C.c_int * 3)(*[int(v) for v in self.nx.tolist()]))

    def splat(self, depth_logit, feat, rots, trans, intrins, post_rots, post_trans, return_cells=False, workspace=None):
        """get_geometry + voxel_pooling (+ QuickCumsum, griddify) on ``gencomm_lss_splat_fwd``: depth_logit [B N, D, fH, fW], feat
        [B N, C, fH, fW] -> [B, C nz, ny, nx]; with ``return_cells`` also the reference's rank of every frustum point (-1 outside).
        ``workspace``: a uint8 tensor of ``gencomm_lss_workspace_bytes`` the caller owns (``_LiftSplatFn``), else the shared one.
        Not differentiable by itself: ``splat_grad`` is."""
        B, N = trans.shape[:2]
        D, fH, fW = self.frustum.shape[:3]
        Cc = feat.shape[1]
        dev = feat.device
        if tuple(depth_logit.shape) != (B * N, D, fH, fW) or tuple(feat.shape) != (B * N, Cc, fH, fW):
            raise ValueError(f"expected depth_logit [{B * N}, {D}, {fH}, {fW}] and feat [{B * N}, C, {fH}, {fW}], got "
                             f"{tuple(depth_logit.shape)} / {tuple(feat.shape)} (imgs must be data_aug_conf.final_dim)")
        fr = self._dev_frustum.get(dev)
        if fr is None:
            fr = self._dev_frustum[dev] = self.frustum.contiguous().to(dev)
        cams = [f32c(t) for t in (rots, trans, intrins, post_rots, post_trans)]
        lo, dx, nx = self._grid()
        nxs = [int(v) for v in self.nx.tolist()]
        l = _lib.lib()
        nbytes = _lib.check_size(l.gencomm_lss_workspace_bytes(B, N, D, fH, fW, Cc, nx), "gencomm_lss_workspace_bytes")
        ws = workspaces.get(dev, nbytes, "lss") if workspace is None else workspace
        out = torch.empty(B, Cc * nxs[2], nxs[1], nxs[0], dtype=torch.float32, device=dev)
        cell = torch.empty(B * N * D * fH * fW, dtype=torch.int32, device=dev) if return_cells else None
        dl, ft = f32c(depth_logit), f32c(feat)
        _lib.check(l.gencomm_lss_splat_fwd(ptr(dl), ptr(ft), ptr(fr), *[ptr(t) for t in cams], lo, dx, nx, B, N, D, fH, fW, Cc,
                                           ptr(out), ptr(cell), ptr(ws), ws.numel(), stream_ptr(dev)), "gencomm_lss_splat_fwd")
        return (out, cell) if return_cells else out

    def splat_grad(self, depth_logit, feat, rots, trans, intrins, post_rots, post_trans):
        """``splat`` with gradients for depth_logit and feat (``_LiftSplatFn``)."""
        require_gpu(feat, "LiftSplatShoot.splat_grad")
        return _LiftSplatFn.apply(depth_logit, feat, self, rots, trans, intrins, post_rots, post_trans)

    def _forward_train(self, x, rots, trans, intrins, post_rots, post_trans):
        require_gpu(x, "LiftSplatShoot")
        if x.requires_grad:
            raise NotImplementedError("LiftSplatShoot(trainable=True): gradients with respect to imgs are not implemented -- the 7x7 stride-2 "
                                      "stem (camencode.conv1) has a weight gradient only; pass imgs without requires_grad")
        B, N, Cimg, imH, imW = x.shape
        xf = f32c(x).view(B * N, Cimg, imH, imW)
        depth_logit, feat = self.camencode(xf[:, :3].contiguous())
        out = self.splat_grad(depth_logit, feat, rots, trans, intrins, post_rots, post_trans)
        if self.depth_supervision:
            self.depth_items = (depth_logit, self.camencode.depth_gt_indices(xf))   # depth_logit attached to the graph, as in the reference
        return out

    def forward(self, data_dict, modality_name):
        inp = data_dict[f"inputs_{modality_name}"]
        x, rots, trans, intrins, post_rots, post_trans = (inp["imgs"], inp["rots"], inp["trans"], inp["intrins"], inp["post_rots"],
                                                          inp["post_trans"])
        if self.trainable and torch.is_grad_enabled():
            return self._forward_train(x, rots, trans, intrins, post_rots, post_trans)
        if torch.is_grad_enabled() and any(t.requires_grad for t in (x, rots, trans, intrins, post_rots, post_trans, *self.parameters())):
            raise NotImplementedError(
                "LiftSplatShoot is inference only: gradients through the camera encoder are not implemented. The GenComm stage-2 model "
                "freezes every encoder_* parameter (heter_model_baseline_w_gencomm_stage2.py:99), so the reference's stage-2 training never "
                "needs them; run the encoder under torch.no_grad() or with requires_grad_(False) parameters")
        require_gpu(x, "LiftSplatShoot")
        B, N, Cimg, imH, imW = x.shape
        xf = f32c(x).view(B * N, Cimg, imH, imW)
        depth_logit, feat = self.camencode(xf[:, :3].contiguous())
        out = self.splat(depth_logit, feat, rots, trans, intrins, post_rots, post_trans)
        if self.depth_supervision:
            self.depth_items = (depth_logit, self.camencode.depth_gt_indices(xf))
        return out
