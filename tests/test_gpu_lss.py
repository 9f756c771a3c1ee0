"""Lift-Splat-Shoot camera encoder on the GPU: geometry and splat kernels against float64 restatements, the whole encoder against
tests/golden/lss.npz (the reference's own code, fp32 on the CPU) and against a float64 run on the same cells, determinism, degenerate and
ragged cases, the 7x7 stride-2 stem + max-pool."""
import os

import numpy as np
import pytest
import torch

from helpers import assert_close
from lss_restatement import SEED, cells64, geometry64, small_args, softmax64, splat64, trunk64

from gencomm_amd import synth
from gencomm_amd.lift_splat_shoot import LiftSplatShoot, maxpool3x3s2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAMS = ("rots", "trans", "intrins", "post_rots", "post_trans")
RTOL, ATOL = 1e-4, 2e-5   # the backbone tests' conv tolerance


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lss.npz"))


def _cams(g, dev=DEV):
    return [torch.from_numpy(g[k]).to(dev) for k in CAMS]


def _random_maps(B, N, D, C, fH, fW, seed):
    rng = np.random.RandomState(seed)
    logit = (2.0 * rng.standard_normal((B * N, D, fH, fW))).astype(np.float32)
    feat = rng.standard_normal((B * N, C, fH, fW)).astype(np.float32)
    return logit, feat


def _check_splat(name, out, cell, logit, feat, B, nx):
    ref, mag = splat64(softmax64(logit), feat, cell.astype(np.int64), B, nx)
    got = out.cpu().numpy().astype(np.float64)
    live = mag > 0
    err = np.abs(got - ref)
    worst = float((err[live] / (mag[live] + 1e-30)).max())
    print(f"{name}: {int(live.sum())} non-empty elements, max |err| / sum |terms| = {worst:.2e}")
    assert worst <= 1e-5, (name, worst)
    assert (got[~live] == 0).all(), name   # empty cells: exact zeros


def test_geometry_cells_match_fixture(g):
    m = LiftSplatShoot(small_args())
    B, N = g["trans"].shape[:2]
    logit, feat = _random_maps(B, N, 48, 16, 8, 16, 1)
    _, cell = m.splat(torch.from_numpy(logit).to(DEV), torch.from_numpy(feat).to(DEV), *_cams(g), return_cells=True)
    cell = cell.cpu().numpy()
    want = g["cell"]
    diff = cell != want
    print(f"geometry: {int(diff.sum())} of {cell.size} frustum points differ from the reference's cells")
    assert diff.sum() <= 1e-4 * cell.size
    if diff.any():
        geom = geometry64(g["frustum"], *[g[k] for k in CAMS])
        _, v = cells64(geom, small_args()["grid_conf"])
        frac = np.abs(v[diff] - np.round(v[diff]))
        assert (frac.min(axis=1) < 1e-3).all(), frac   # within rounding distance of a cell boundary


def test_splat_kernel_vs_float64_on_hip_cells(g):
    m = LiftSplatShoot(small_args())
    B, N = g["trans"].shape[:2]
    logit, feat = _random_maps(B, N, 48, 16, 8, 16, 2)
    out, cell = m.splat(torch.from_numpy(logit).to(DEV), torch.from_numpy(feat).to(DEV), *_cams(g), return_cells=True)
    _check_splat("splat C=16", out, cell.cpu().numpy(), logit, feat, B, [256, 256, 1])


def test_splat_kernel_wide_channels_vs_float64(g):
    """C = 200: two channel passes, the second one partial."""
    a = small_args()
    a["img_features"] = 200
    m = LiftSplatShoot(a)
    B, N = g["trans"].shape[:2]
    logit, feat = _random_maps(B, N, 48, 200, 8, 16, 3)
    out, cell = m.splat(torch.from_numpy(logit).to(DEV), torch.from_numpy(feat).to(DEV), *_cams(g), return_cells=True)
    _check_splat("splat C=200", out, cell.cpu().numpy(), logit, feat, B, [256, 256, 1])


def _encoder(args=None):
    m = LiftSplatShoot(args or small_args()).eval()
    synth.fill_params_(m, SEED)
    synth.fill_running_stats_(m, SEED)
    return m.to(DEV)


def _run(m, g):
    inp = {k: torch.from_numpy(g[k].astype(np.float32)).to(DEV) for k in ("imgs",) + CAMS}   # imgs are stored as (exact) float16
    with torch.no_grad():
        out = m({"inputs_m4": inp}, "m4")
    torch.cuda.synchronize()
    return out, m.depth_items


def test_encoder_vs_reference_fixture(g):
    m = _encoder()
    out, (depth_logit, depth_gt) = _run(m, g)
    assert tuple(out.shape) == tuple(g["bev_shape"])
    assert np.array_equal(depth_gt.cpu().numpy(), g["depth_gt_indices"])
    assert_close(depth_logit.cpu().numpy(), g["depth_logit"], RTOL, ATOL, "depth_logit")
    # BEV: compare on the cells whose point sets agree between the HIP geometry and the reference's (all but rounding-edge points)
    B, C = out.shape[0], small_args()["img_features"]
    _, cell = m.splat(depth_logit, torch.zeros(B * 2, C, 8, 16, device=DEV), *_cams(g), return_cells=True)
    cell, want = cell.cpu().numpy().astype(np.int64), g["cell"].astype(np.int64)
    nx = [256, 256, 1]

    def flat(r):
        r = r[r >= 0]
        return ((r % B) * nx[1] + (r // B) % nx[1]) * nx[0] + r // (B * nx[1])   # nz = 1: (b, y, x)

    bad = set(flat(cell[cell != want]).tolist()) | set(flat(want[cell != want]).tolist())
    keep = np.array([i not in bad for i in g["bev_idx"].tolist()])
    hip = out.cpu().numpy().reshape(B, C, nx[1] * nx[0]).transpose(0, 2, 1).reshape(-1, C)
    idx = g["bev_idx"]
    got, r32 = hip[idx][keep].astype(np.float64), g["bev_val"][keep].astype(np.float64)
    # float64 truth: the trunk in float64 on the same weights and inputs, softmax + lift + sum in float64 on the reference's cells
    imgs = g["imgs"].astype(np.float64)
    dl64, ft64 = trunk64(m.camencode, imgs.reshape(-1, *imgs.shape[2:])[:, :3])
    m64, _ = splat64(softmax64(dl64.numpy()), ft64.numpy(), want, B, nx)
    r64 = m64.reshape(B, C, nx[1] * nx[0]).transpose(0, 2, 1).reshape(-1, C)[idx][keep]
    h_gap, r_gap = np.abs(got - r64), np.abs(r32 - r64)
    rms = lambda a: float(np.sqrt((a ** 2).mean()))
    print(f"encoder vs float64: HIP rms {rms(h_gap):.3e} max {h_gap.max():.3e} | reference fp32 rms {rms(r_gap):.3e} max {r_gap.max():.3e} "
          f"({int(keep.sum())} of {keep.size} cells compared)")
    assert keep.sum() >= 0.999 * keep.size
    assert rms(h_gap) <= 2.0 * rms(r_gap) and h_gap.max() <= 2.0 * r_gap.max()
    empty = np.ones(hip.shape[0], bool)
    empty[idx] = False
    empty[list(bad)] = False
    assert (hip[empty] == 0).all()


def test_encoder_is_deterministic(g):
    m = _encoder()
    a, (la, ia) = _run(m, g)
    a, la, ia = a.clone(), la.clone(), ia.clone()
    b, (lb, ib) = _run(m, g)
    assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(ia, ib)


def test_camera_that_sees_nothing_gives_zero_bev(g):
    m = LiftSplatShoot(small_args())
    B, N = g["trans"].shape[:2]
    trans = g["trans"].copy()
    trans[:, :, 0] += 1000.0   # every camera 1 km away
    cams = _cams(g)
    cams[1] = torch.from_numpy(trans).to(DEV)
    logit, feat = _random_maps(B, N, 48, 16, 8, 16, 4)
    out, cell = m.splat(torch.from_numpy(logit).to(DEV), torch.from_numpy(feat).to(DEV), *cams, return_cells=True)
    assert (cell == -1).all()
    assert torch.count_nonzero(out) == 0


def test_agents_with_different_cameras_in_one_batch(g):
    """Each agent's BEV equals the same agent run alone: per-camera parameters are read per camera, ranks carry the batch index."""
    m = LiftSplatShoot(small_args())
    B, N = g["trans"].shape[:2]
    logit, feat = _random_maps(B, N, 48, 16, 8, 16, 5)
    both = m.splat(torch.from_numpy(logit).to(DEV), torch.from_numpy(feat).to(DEV), *_cams(g))
    for b in range(B):
        cams = [torch.from_numpy(g[k][b:b + 1]).to(DEV) for k in CAMS]
        one = m.splat(torch.from_numpy(logit[b * N:(b + 1) * N]).to(DEV), torch.from_numpy(feat[b * N:(b + 1) * N]).to(DEV), *cams)
        assert torch.equal(both[b:b + 1], one), b
        assert torch.count_nonzero(one) > 0


def test_two_height_layers(g):
    a = small_args()
    a["grid_conf"] = dict(a["grid_conf"], zbound=[-10, 10, 10.0])   # nz = 2: channel z C + c
    m = LiftSplatShoot(a)
    B, N = g["trans"].shape[:2]
    logit, feat = _random_maps(B, N, 48, 16, 8, 16, 6)
    out, cell = m.splat(torch.from_numpy(logit).to(DEV), torch.from_numpy(feat).to(DEV), *_cams(g), return_cells=True)
    assert tuple(out.shape) == (B, 32, 256, 256)
    cell = cell.cpu().numpy().astype(np.int64)
    c64, _ = cells64(geometry64(g["frustum"], *[g[k] for k in CAMS]), a["grid_conf"])
    assert (cell != c64).sum() <= 1e-4 * cell.size
    z = (cell[cell >= 0] // B) % 2
    assert (z == 0).any() and (z == 1).any()
    _check_splat("splat nz=2", out, cell, logit, feat, B, [256, 256, 2])


def test_stem_and_maxpool_vs_float64():
    from gencomm_amd.bev_backbone import conv2d_hip
    import torch.nn.functional as F
    m = _encoder().camencode
    rng = np.random.RandomState(7)
    for shape in ((2, 3, 64, 128), (1, 3, 37, 53)):
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
        with torch.no_grad():
            y = conv2d_hip(x.to(DEV), m.conv1, m.bn1, relu=True)
            p = maxpool3x3s2(y)
            w = m.conv1.weight.detach().cpu().double()
            bn = m.bn1
            r = F.conv2d(x.double(), w, stride=2, padding=3)
            r = F.batch_norm(r, bn.running_mean.cpu().double(), bn.running_var.cpu().double(), bn.weight.detach().cpu().double(),
                             bn.bias.detach().cpu().double(), False, 0.0, bn.eps).relu()
            rp = F.max_pool2d(r, 3, 2, 1)
        assert_close(y.cpu().numpy(), r.numpy(), RTOL, ATOL, f"stem {shape}")
        assert_close(p.cpu().numpy(), rp.numpy(), RTOL, ATOL, f"stem + max-pool {shape}")
        # the max-pool alone is exact
        assert torch.equal(p.cpu(), F.max_pool2d(y.cpu(), 3, 2, 1))
