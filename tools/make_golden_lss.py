#!/usr/bin/env python3
"""Golden fixture of the Lift-Splat-Shoot camera encoder, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_lss.py      # writes tests/golden/lss.npz and tests/golden/lss_state_dict_keys.json

The reference's ``LiftSplatShoot`` (opencood/models/heter_encoders.py:83-241) runs with its hard-coded ``cuda`` device mapped to the
CPU, ``efficientnet_pytorch`` stubbed (oracle/make_golden.py's import stubs) and ``torchvision.models.resnet.resnet101`` bound to the
from-scratch standard ResNet-101 below (torchvision's key names). The trunk arithmetic is therefore NOT pinned to torchvision's
code (as DCNv1 and polygon IoU are not); the frustum, depth discretisation, geometry, truncation, rank / argsort, QuickCumsum,
softmax, lift and griddify are the reference's own.

Weights: ``gencomm_amd.synth.fill_params_(module, SEED)`` and ``synth.fill_running_stats_(module, SEED)`` -- the tests rebuild them
from the seed. Inputs and camera parameters are stored; the image values lie on a 1/16 grid, so float16 holds them exactly (and the
file stays small). Stored outputs are the fp32 reference's only: the tests form the float64 result themselves (a float64 run of the
trunk on the same weights, summed on the reference's cells) for the relative criterion.
"""
from __future__ import annotations

import json
import math
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))

import numpy as np
import torch
import torch.nn as nn

from gencomm_amd import synth

REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
SEED = 31

GRID_CONF = {"xbound": [-51.2, 51.2, 0.4], "ybound": [-51.2, 51.2, 0.4], "zbound": [-10, 10, 20.0], "ddiscr": [2, 50, 48], "mode": "LID"}


def m4_args():   # hypes_yaml/opv2v/GenComm_yamls/baselines/stage1/m4_att.yaml encoder_args
    return {"grid_conf": dict(GRID_CONF),
            "data_aug_conf": {"resize_lim": [0.56, 0.61], "final_dim": [336, 448], "rot_lim": [-3.6, 3.6], "H": 600, "W": 800,
                              "rand_flip": False, "bot_pct_lim": [0.0, 0.05], "cams": ["camera0", "camera1", "camera2", "camera3"], "Ncams": 4},
            "img_downsample": 8, "img_features": 128, "use_depth_gt": False, "depth_supervision": True, "camera_encoder": "Resnet101"}


def small_args():   # the fixture: shipped grid, 64 x 128 images, 8 image channels
    a = m4_args()
    a["data_aug_conf"] = dict(a["data_aug_conf"], final_dim=[64, 128])
    a["img_features"] = 8
    return a


# ---- from-scratch standard ResNet-101 (torchvision's attribute names, so state_dict keys match) -----------------------------
class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        return self.relu(self.bn3(self.conv3(out)) + idt)


class _ResNet(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)

    def _make_layer(self, planes, blocks, stride=1):
        ds = None
        if stride != 1 or self.inplanes != planes * 4:
            ds = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
        layers = [_Bottleneck(self.inplanes, planes, stride, ds)]
        self.inplanes = planes * 4
        layers += [_Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


def resnet101(pretrained=False, zero_init_residual=False, **kw):
    return _ResNet([3, 4, 23, 3])


class _TorchCpu(types.ModuleType):
    """The reference module's `torch`, with torch.device("cuda") mapped to the CPU (heter_encoders.py:93-99)."""

    def __init__(self):
        super().__init__("torch")

    def __getattr__(self, k):
        if k == "device":
            return lambda *a, **kw: torch.device("cpu")
        return getattr(torch, k)


def load_reference():
    from make_golden import _install_stubs
    _install_stubs()
    sys.path.insert(0, REF)
    import torchvision.models.resnet as tvr   # the import stub
    tvr.resnet101 = resnet101
    import opencood.models.heter_encoders as he
    he.torch = _TorchCpu()
    return he


def camera(yaw_deg, t, pitch_deg=0.0):
    """rots (camera -> ego; camera x right, y down, z forward; ego x forward, y left, z up), trans."""
    base = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], np.float64)
    p = math.radians(pitch_deg)
    pitch = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    y = math.radians(yaw_deg)
    yaw = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    return yaw @ pitch @ base, np.array(t, np.float64)


def make_inputs(rng, B=2, N=2, H=64, W=128):
    """Two agents x two cameras. Agent 0: front camera at the origin, rear camera 10 m behind it (its far points cross x = -51.2:
    the truncation edge); agent 1: a camera 40 m forward (half its frustum beyond the grid) and a side camera, pitched."""
    poses = [[(0.0, (0.0, 0.0, 1.7)), (180.0, (-10.0, 0.5, 1.7))],
             [(3.0, (40.0, -2.0, 1.8)), (90.0, (1.0, 1.0, 1.6), 4.0)]]
    rots = np.zeros((B, N, 3, 3)); trans = np.zeros((B, N, 3)); intrins = np.zeros((B, N, 3, 3))
    post_rots = np.zeros((B, N, 3, 3)); post_trans = np.zeros((B, N, 3))
    for b in range(B):
        for n in range(N):
            pose = poses[b][n]
            R, t = camera(pose[0], pose[1], pose[2] if len(pose) > 2 else 0.0)
            rots[b, n], trans[b, n] = R, t
            f = 400.0 + 20.0 * rng.standard_normal()
            intrins[b, n] = [[f, 0.0, 400.0 + 5 * rng.standard_normal()], [0.0, f, 300.0 + 5 * rng.standard_normal()], [0.0, 0.0, 1.0]]
            s = 0.16 + 0.005 * rng.standard_normal()                      # resize 800 x 600 -> ~128 x 96, crop to 64 rows
            a = math.radians(rng.uniform(-3.6, 3.6))                      # rot_lim
            post_rots[b, n] = [[s * math.cos(a), -s * math.sin(a), 0.0], [s * math.sin(a), s * math.cos(a), 0.0], [0.0, 0.0, 1.0]]
            post_trans[b, n] = [rng.uniform(-3, 3), -16.0 + rng.uniform(-2, 2), 0.0]
    imgs = np.clip(np.round(16 * rng.standard_normal((B, N, 4, H, W))) / 16, -4, 4).astype(np.float32)
    imgs[:, :, 3] = (np.round(16 * rng.uniform(0.0, 70.0, (B, N, H, W))) / 16).astype(np.float32)   # depth: below d_min, inside, beyond d_max
    f32 = lambda a: a.astype(np.float32)
    return {"imgs": imgs, "rots": f32(rots), "trans": f32(trans), "intrins": f32(intrins), "post_rots": f32(post_rots),
            "post_trans": f32(post_trans)}


def cells_of(model, geom):
    """voxel_pooling's cell arithmetic (heter_encoders.py:167-190) on the reference's geometry: rank per frustum point, -1 outside."""
    B = geom.shape[0]
    g = ((geom - (model.bx - model.dx / 2.)) / model.dx).long().view(-1, 3)
    Np = g.shape[0]
    b = torch.cat([torch.full([Np // B], ix, dtype=torch.long) for ix in range(B)])
    nx = model.nx
    kept = (g[:, 0] >= 0) & (g[:, 0] < nx[0]) & (g[:, 1] >= 0) & (g[:, 1] < nx[1]) & (g[:, 2] >= 0) & (g[:, 2] < nx[2])
    rank = g[:, 0] * (nx[1] * nx[2] * B) + g[:, 1] * (nx[2] * B) + g[:, 2] * B + b
    return torch.where(kept, rank, torch.full_like(rank, -1))


def main():
    he = load_reference()
    torch.manual_seed(0)

    keys_model = he.LiftSplatShoot(m4_args())
    keys = [[k, list(v.shape)] for k, v in keys_model.state_dict().items()]
    with open(os.path.join(OUT, "lss_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    del keys_model

    args = small_args()
    model = he.LiftSplatShoot(args).eval()
    synth.fill_params_(model, SEED)
    synth.fill_running_stats_(model, SEED)
    rng = np.random.RandomState(SEED)
    inp = make_inputs(rng)
    t = {k: torch.from_numpy(v.copy()) for k, v in inp.items()}
    with torch.no_grad():
        bev = model({"inputs_m4": dict(t)}, "m4")
        depth_logit, depth_gt_indices = model.depth_items
        geom = model.get_geometry(t["rots"], t["trans"], t["intrins"], t["post_rots"], t["post_trans"])
        cell = cells_of(model, geom)
    B, N = 2, 2
    Cc = args["img_features"]
    nx = [int(v) for v in model.nx]
    cn = cell.numpy()
    live = cn >= 0
    ranks = np.unique(cn[live])
    # rank -> flat index of (b, z, y, x) in [B, nz, ny, nx]
    bb = ranks % B; zz = (ranks // B) % nx[2]; yy = (ranks // (B * nx[2])) % nx[1]; xx = ranks // (B * nx[2] * nx[1])
    flat = ((bb * nx[2] + zz) * nx[1] + yy) * nx[0] + xx
    bevn = bev.numpy().reshape(B, nx[2], Cc, nx[1], nx[0])
    vals32 = bevn[bb, zz, :, yy, xx]
    assert np.count_nonzero(bev.numpy()) <= vals32.size
    np.savez_compressed(
        os.path.join(OUT, "lss.npz"), seed=np.int64(SEED), imgs=inp["imgs"].astype(np.float16),
        **{k: v for k, v in inp.items() if k != "imgs"},
        frustum=model.frustum.numpy(), depth_bins=model.frustum[:, 0, 0, 2].numpy(),
        cell=cn.astype(np.int32), bev_shape=np.array(bev.shape, np.int64), bev_idx=flat.astype(np.int32),
        bev_val=vals32.astype(np.float32),
        depth_logit=depth_logit.numpy(), depth_gt_indices=depth_gt_indices.numpy())
    print("lss.npz:", os.path.getsize(os.path.join(OUT, "lss.npz")), "bytes;", int(live.sum()), "of", cn.size, "points inside;",
          len(ranks), "non-empty cells")


if __name__ == "__main__":
    main()
