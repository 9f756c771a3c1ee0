"""Torch restatement of HEAL's PyramidFusion (opencood/models/fuse_modules/pyramid_fuse.py) in any dtype, the seeded parameters both
sides of the fixture use, the cases of the fixture and the margin rule of the 0 -> -inf step. Shared by tests/test_pyramid.py,
tests/test_gpu_pyramid.py, tools/make_golden_pyramid.py and tools/bench_pyramid.py. Framework operators only: nothing here touches
the HIP library."""
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from fusion_train_restatement import affine_of, rel_rms, rot, theta, warp_to_ego  # noqa: F401

MARGIN = 1e-4          # an agent whose scoring taps weigh less than this (and more than 0) at a pixel marks the pixel
MARGIN_CAP = 1e-3      # the share of marked pixels any case may have (the strict cases: none at all)
SEED = 6100


def cfg(resnext=True, layer_nums=(1, 2, 1)):
    """The shipped pyramid configuration (e.g. hypes_yaml/opv2v/MoreModality/HEAL/stage1/m1_pyramid.yaml) with a short layer_nums."""
    return {"layer_nums": list(layer_nums), "num_filters": [64, 128, 256], "layer_strides": [1, 2, 2], "upsample_strides": [1, 2, 4],
            "num_upsample_filter": [128, 128, 128], "resnext": resnext}


# ------------------------------------------------------------------------------------------- parameters from a seed
def fill_params_(model, seed=SEED):
    """Every parameter and BatchNorm statistic of `model` from numpy's legacy RandomState, keyed by (seed, crc32 of the state_dict key):
    the same values on any module with the same keys, whatever their order. Values are float32-representable."""
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if key.endswith("num_batches_tracked"):
                continue
            rng = np.random.RandomState([seed, zlib.crc32(key.encode()) & 0x7fffffff])
            shape = tuple(t.shape)
            if t.dim() == 4:
                fan_in = shape[1] * shape[2] * shape[3]
                v = rng.standard_normal(shape) * np.sqrt(1.5 / fan_in)
            elif key.endswith("running_var") or key.endswith(".weight"):
                v = rng.uniform(0.5, 1.5, shape)
            else:                                        # running_mean, BatchNorm bias, head bias
                v = 0.2 * rng.standard_normal(shape)
            t.copy_(torch.from_numpy(v.astype(np.float32)).to(t.dtype))
    return model


# ------------------------------------------------------------------------------------------- the model
def _bn(c, **kw):
    return nn.BatchNorm2d(c, **kw)


class _Basic(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample, groups, width):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = _bn(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = _bn(planes)
        self.downsample = downsample

    def forward(self, x):
        idn = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn1(self.conv1(x)))
        return F.relu(self.bn2(self.conv2(out)) + idn)


class _Bottle(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample, groups, width):
        super().__init__()
        w = int(planes * (width / 64.)) * groups
        self.conv1 = nn.Conv2d(inplanes, w, 1, bias=False)
        self.bn1 = _bn(w)
        self.conv2 = nn.Conv2d(w, w, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = _bn(w)
        self.conv3 = nn.Conv2d(w, planes, 1, bias=False)
        self.bn3 = _bn(planes)
        self.downsample = downsample

    def forward(self, x):
        idn = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        return F.relu(self.bn3(self.conv3(out)) + idn)


class _ResNet(nn.Module):
    def __init__(self, block, layers, strides, filters, inplanes, groups, width):
        super().__init__()
        for i, (n, s, c) in enumerate(zip(layers, strides, filters)):
            down = None
            if s != 1 or inplanes != c:
                down = nn.Sequential(nn.Conv2d(inplanes, c, 1, s, bias=False), _bn(c))
            blocks = [block(inplanes, c, s, down, groups, width)] + [block(c, c, 1, None, groups, width) for _ in range(1, n)]
            inplanes = c
            setattr(self, f"layer{i}", nn.Sequential(*blocks))


class PyramidRestatement(nn.Module):
    """PyramidFusion in framework operators; the state_dict keys are the reference's."""

    def __init__(self, model_cfg):
        super().__init__()
        nf, ups, nu = model_cfg["num_filters"], model_cfg["upsample_strides"], model_cfg["num_upsample_filter"]
        block, g, w = (_Bottle, 32, 4) if model_cfg["resnext"] else (_Basic, 1, 64)
        self.resnet = _ResNet(block, model_cfg["layer_nums"], model_cfg["layer_strides"], nf, model_cfg.get("inplanes", 64), g, w)
        self.num_levels = len(nf)
        self.deblocks = nn.ModuleList(nn.Sequential(nn.ConvTranspose2d(nf[i], nu[i], ups[i], stride=ups[i], bias=False),
                                                    _bn(nu[i], eps=1e-3, momentum=0.01), nn.ReLU()) for i in range(self.num_levels))
        for i in range(self.num_levels):
            setattr(self, f"single_head_{i}", nn.Conv2d(nf[i], 1, 1))

    def features(self, x):
        out = []
        for i in range(self.num_levels):
            x = getattr(self.resnet, f"layer{i}")(x)
            out.append(x)
        return out

    def decode(self, feats):
        return torch.cat([self.deblocks[i](f) for i, f in enumerate(feats)], dim=1)

    def forward_single(self, x):
        feats = self.features(x)
        return self.decode(feats), [getattr(self, f"single_head_{i}")(f) for i, f in enumerate(feats)]

    def forward_collab(self, x, record_len, affine, modalities=None, crop=None, levels=None):
        """(fused, occ_map_list); `levels`, if a list, receives per level (feature, score, fused level)."""
        feats = self.features(x)
        fused, occs = [], []
        for i, f in enumerate(feats):
            occ = getattr(self, f"single_head_{i}")(f)
            occs.append(occ)
            score = torch.sigmoid(occ) + 1e-4
            if crop:
                score = score * crop_mask(f.shape[2], f.shape[3], modalities, crop).to(score)
            fused.append(weighted_fuse(f, score, record_len, affine))
            if levels is not None:
                levels.append((f, score, fused[-1]))
        return self.decode(fused), occs


def crop_mask(H, W, modalities, crop):
    """[n, 1, H, W] bool: where the score survives (pyramid_fuse.py:147-160, by numpy slicing: Python's slice semantics)."""
    m = np.ones((len(modalities), 1, H, W), bool)
    for j, mod in enumerate(modalities):
        if mod not in crop:
            continue
        ch = H / crop[mod][f"crop_ratio_H_{mod}"] - 4
        cw = W / crop[mod][f"crop_ratio_W_{mod}"] - 4
        sh, eh, sw, ew = int(H // 2 - ch // 2), int(H // 2 + ch // 2), int(W // 2 - cw // 2), int(W // 2 + cw // 2)
        m[j] = False
        m[j, :, sh:eh, sw:ew] = True
    return torch.from_numpy(m)


def weighted_fuse(x, score, record_len, affine):
    """pyramid_fuse.py:17-63."""
    out = []
    for fx, fs in zip(warp_to_ego(x, record_len, affine), warp_to_ego(score, record_len, affine)):
        fs = fs.masked_fill(fs == 0, -float("inf"))
        p = torch.softmax(fs, dim=0)
        p = torch.where(torch.isnan(p), torch.zeros_like(p), p)
        out.append((fx * p).sum(0))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------- the margin rule
def margin_mask(score, record_len, affine):
    """bool [B, H, W]: output pixels where, in float64, some agent's bilinear taps that lie inside the map AND carry a nonzero score
    have a total weight in (0, MARGIN): there float32 rounding of the sampling position may decide whether the agent takes a softmax
    share at all. These are the only elements a comparison may leave out."""
    nz = (torch.as_tensor(score).double() != 0).double()
    out = []
    for w in warp_to_ego(nz, record_len, torch.as_tensor(affine)):
        out.append(((w > 0) & (w < MARGIN)).any(0)[0])
    return torch.stack(out)


def within(got, ref, leave_out=None):
    """(worst err / (1e-5 + 1e-4 |ref|), number compared): the project's elementwise tolerance."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    r = np.abs(got - ref) / (1e-5 + 1e-4 * np.abs(ref))
    if leave_out is not None:
        r = r[~np.broadcast_to(np.asarray(leave_out, bool), r.shape)]
    return (float(r.max()) if r.size else 0.0), int(r.size)


# ------------------------------------------------------------------------------------------- cases of the fixture
def quantised(seed, shape, step=8):
    """Normal values on a 1/step grid (the fixture's inputs compress well and are exact in float32)."""
    return (np.round(step * np.random.RandomState(seed).standard_normal(shape)) / step).astype(np.float32)


def collab_scenes(H, W):
    """Scene 0: ONE agent whose own matrix affine[b, 0, 0] is not the identity (part of the output sees nobody and must be exactly 0).
    Scene 1: identity ego, two agents with generic rotations and fractional shifts, one agent entirely outside the map."""
    I = theta(H, W)
    return [[rot(H, W, 0.35, 1.37, -0.61)],
            [I, rot(H, W, 0.4, 1.37, -0.61), rot(H, W, -0.9, -1.21, 1.43), theta(H, W, tx=3.0 * W + 0.37)]]


COLLAB = dict(C=64, H=8, W=12, record_len=[1, 4])
# the crop case: one scene on a 12 x 12 map (ratio 2 keeps rows / columns 5..6 of level 0 and nothing below; ratio 1 keeps 2..9 of level 0,
# 1..4 of level 1 and nothing of level 2). The camera agents are NOT the ego: an identity warp samples within rounding of the lattice,
# where the 0 -> -inf step of a cropped score is decided by rounding residue in float64 as well.
CROP = dict(C=64, H=12, W=12, record_len=[4], modalities=["m1", "m2", "m4", "m1"],
            info={"m2": {"crop_ratio_W_m2": 2, "crop_ratio_H_m2": 2}, "m4": {"crop_ratio_W_m4": 1, "crop_ratio_H_m4": 1}})


def crop_scenes(H, W):
    return [[theta(H, W), rot(H, W, 0.3, 0.37, -0.41), rot(H, W, -0.5, -0.63, 0.29), rot(H, W, 1.1, 1.21, 0.77)]]


FUSE = dict(C=5, H=8, W=12, record_len=[1, 4])     # the direct weighted_fuse case: random maps, COLLAB's poses


def fuse_inputs():
    """x, score of the direct case. Scores are positive with blocks of exact zeros INSIDE the map on the non-ego agents."""
    n, C, H, W = sum(FUSE["record_len"]), FUSE["C"], FUSE["H"], FUSE["W"]
    x = quantised(SEED + 30, (n, C, H, W))
    s = np.random.RandomState(SEED + 31).uniform(0.05, 1.0, (n, 1, H, W)).astype(np.float32)
    s[2, :, 2:6, 3:9] = 0.0
    s[3, :, :, :5] = 0.0
    s[0, :, 0:3, :] = 0.0          # the lone agent of scene 0 (a generic pose, not an identity)
    return x, s
