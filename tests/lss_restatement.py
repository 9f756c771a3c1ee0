"""Float64 restatements of the Lift-Splat-Shoot encoder's geometry and splat (opencood/models/heter_encoders.py:123-205) and of its
ResNet trunk (conv1 / bn1 / ReLU / max-pool, torchvision Bottlenecks, 1x1 heads), written from the formulas for the tests of
gencomm_amd.lift_splat_shoot; the shared fixture arguments of tests/golden/lss.npz."""
import numpy as np

SEED = 31
GRID_CONF = {"xbound": [-51.2, 51.2, 0.4], "ybound": [-51.2, 51.2, 0.4], "zbound": [-10, 10, 20.0], "ddiscr": [2, 50, 48], "mode": "LID"}


def m4_args():   # the shipped m4 encoder_args (GenComm_yamls/baselines/stage1/m4_att.yaml)
    return {"grid_conf": dict(GRID_CONF),
            "data_aug_conf": {"resize_lim": [0.56, 0.61], "final_dim": [336, 448], "rot_lim": [-3.6, 3.6], "H": 600, "W": 800,
                              "rand_flip": False, "bot_pct_lim": [0.0, 0.05], "cams": ["camera0", "camera1", "camera2", "camera3"], "Ncams": 4},
            "img_downsample": 8, "img_features": 128, "use_depth_gt": False, "depth_supervision": True, "camera_encoder": "Resnet101"}


def small_args():   # lss.npz: shipped grid, 64 x 128 images, 8 image channels
    a = m4_args()
    a["data_aug_conf"] = dict(a["data_aug_conf"], final_dim=[64, 128])
    a["img_features"] = 8
    return a


def grid(grid_conf):
    rows = [grid_conf["xbound"], grid_conf["ybound"], grid_conf["zbound"]]
    dx = np.array([r[2] for r in rows], np.float64)
    lo = np.array([r[0] for r in rows], np.float64)   # bx - dx / 2 in exact arithmetic
    nx = [int((r[1] - r[0]) / r[2]) for r in rows]
    return lo, dx, nx


def geometry64(frustum, rots, trans, intrins, post_rots, post_trans):
    """get_geometry in float64: [B, N, D, fH, fW, 3] ego coordinates."""
    f = np.asarray(frustum, np.float64)
    pr, pt = np.asarray(post_rots, np.float64), np.asarray(post_trans, np.float64)
    R, I, T = np.asarray(rots, np.float64), np.asarray(intrins, np.float64), np.asarray(trans, np.float64)
    p = f[None, None] - pt[:, :, None, None, None, :]
    p = np.einsum("bnij,bndhwj->bndhwi", np.linalg.inv(pr), p)
    p = np.concatenate([p[..., :2] * p[..., 2:3], p[..., 2:3]], -1)
    p = np.einsum("bnij,bndhwj->bndhwi", R @ np.linalg.inv(I), p)
    return p + T[:, :, None, None, None, :]


def cells64(geom, grid_conf):
    """(rank per frustum point or -1, float64 cell coordinates) -- truncation toward zero as .long()."""
    lo, dx, nx = grid(grid_conf)
    B = geom.shape[0]
    v = ((geom - lo) / dx).reshape(-1, 3)
    g = np.trunc(v).astype(np.int64)
    b = np.repeat(np.arange(B), v.shape[0] // B)
    kept = np.all((g >= 0) & (g < np.array(nx)) & (v > -1), axis=1)
    rank = g[:, 0] * (nx[1] * nx[2] * B) + g[:, 1] * (nx[2] * B) + g[:, 2] * B + b
    return np.where(kept, rank, -1), v


def softmax64(logit):
    x = np.asarray(logit, np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def splat64(prob, feat, cell, B, nx):
    """voxel_pooling's sum per cell in float64 from given cells: prob [BN, D, fH, fW], feat [BN, C, fH, fW] -> (out [B, nz C, ny, nx],
    abs-sum [B, nz C, ny, nx] = sum of |prob * feat| per element, the scale of its rounding error)."""
    prob = np.asarray(prob, np.float64)
    feat = np.asarray(feat, np.float64)
    BN, D, fH, fW = prob.shape
    C = feat.shape[1]
    lift = (prob[:, :, None] * feat[:, None]).transpose(0, 1, 3, 4, 2).reshape(-1, C)   # [BN D fH fW, C]
    live = cell >= 0
    r = cell[live]
    b = r % B; z = (r // B) % nx[2]; y = (r // (B * nx[2])) % nx[1]; x = r // (B * nx[2] * nx[1])
    flat = ((b * nx[2] + z) * nx[1] + y) * nx[0] + x
    out = np.zeros((B * nx[2] * nx[1] * nx[0], C))
    mag = np.zeros_like(out)
    np.add.at(out, flat, lift[live])
    np.add.at(mag, flat, np.abs(lift[live]))
    shape = (B, nx[2], nx[1], nx[0], C)
    to_map = lambda a: a.reshape(shape).transpose(0, 1, 4, 2, 3).reshape(B, nx[2] * C, nx[1], nx[0])
    return to_map(out), to_map(mag)


def trunk64(enc, x):
    """CamEncode_Resnet101's trunk and heads in float64 on the CPU (torch.nn.functional, eval-mode BatchNorm): enc = the module
    (parameters anywhere), x [BN, 3, H, W] -> (depth_logit, image features), float64."""
    import torch
    import torch.nn.functional as F

    d = lambda t: None if t is None else t.detach().cpu().double()

    def layer(x, conv, bn, relu=True, res=None):
        y = F.conv2d(x, d(conv.weight), d(conv.bias), conv.stride, conv.padding)
        if bn is not None:
            y = F.batch_norm(y, d(bn.running_mean), d(bn.running_var), d(bn.weight), d(bn.bias), False, 0.0, bn.eps)
        if res is not None:
            y = y + res
        return y.relu() if relu else y

    with torch.no_grad():
        x = F.max_pool2d(layer(torch.as_tensor(x).double(), enc.conv1, enc.bn1), 3, 2, 1)
        for blk in list(enc.layer1) + list(enc.layer2):
            idt = x if blk.downsample is None else layer(x, blk.downsample[0], blk.downsample[1], relu=False)
            out = layer(layer(x, blk.conv1, blk.bn1), blk.conv2, blk.bn2)
            x = layer(out, blk.conv3, blk.bn3, res=idt)
        return layer(x, enc.depth_head, None, relu=False), layer(x, enc.image_head, None, relu=False)


def depth_targets32(depth, d_min, d_max, num_bins, mode, ds):
    """bin_depths(target=False) + the pick of get_gt_depth_dist in float32 numpy arithmetic, in the reference's operation order."""
    d = np.minimum(np.asarray(depth, np.float32), np.float32(d_max))
    f32 = np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "UD":
            idx = (d - f32(d_min)) / f32((d_max - d_min) / num_bins)
        else:
            bin_size = f32(2 * (d_max - d_min) / (num_bins * (1 + num_bins)))
            idx = f32(-0.5) + f32(0.5) * np.sqrt(f32(1) + f32(8) * (d - f32(d_min)) / bin_size)
    idx = idx.astype(np.float32)
    idx[idx < 0] = 0
    idx[idx >= num_bins] = num_bins - 1
    idx[~np.isfinite(idx)] = num_bins - 1
    return idx.astype(np.int64)[:, ds // 2::ds, ds // 2::ds]
