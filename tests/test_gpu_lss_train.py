"""Training the Lift-Splat-Shoot camera encoder on the GPU: the lift-splat backward, the max-pool backward, the stem's weight gradient
and the depth-loss kernel against float64, determinism and workspace ownership, and one whole training step against
tests/golden/lss_train.npz (the reference's own modules in .train() mode, tools/make_golden_lss_train.py).

Criterion of the float64 comparisons (unless a test says otherwise): relative rms error <= 2 x the error of the fp32 ATen autograd of
the same formula against the same float64 result, floored at 1e-6; the factor 2 allows for the different summation order."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lss_restatement import SEED, small_args

from gencomm_amd import synth
from gencomm_amd.bev_backbone import conv2d_hip
from gencomm_amd.lift_splat_shoot import LiftSplatShoot, maxpool3x3s2
from gencomm_amd.point_pillar_gencomm_loss import depth_focal_loss, depth_term

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAMS = ("rots", "trans", "intrins", "post_rots", "post_trans")
PARAMS = ("conv1.weight", "bn1.weight", "layer1.0.conv2.weight", "layer2.0.downsample.0.weight", "layer2.3.bn3.bias", "depth_head.weight",
          "depth_head.bias", "image_head.weight")
STATS = ("bn1.running_mean", "bn1.running_var", "layer2.3.bn3.running_mean", "layer2.3.bn3.running_var")


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lss.npz"))


@pytest.fixture(scope="module")
def gt(golden_dir):
    return np.load(os.path.join(golden_dir, "lss_train.npz"))


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


def cotangent(seed, shape):   # tools/make_golden_lss_train.py: the seeded cotangent of the BEV map, on a 1/16 grid
    rng = np.random.RandomState(seed + 1000)
    return (np.clip(np.round(16 * rng.standard_normal(shape)), -32, 32) / 16).astype(np.float32)


def dense_splat(logit, feat, cell, B, nx):
    """The dense restatement sum prob . feat on given cells with framework operators (any dtype / device of `logit`): logit
    [BN, D, fH, fW], feat [BN, C, fH, fW], cell int64 [BN D fH fW] (rank or -1) -> [B, nz C, ny, nx]. No point is excluded."""
    BN, D, fH, fW = logit.shape
    C, HW = feat.shape[1], fH * fW
    prob = logit.softmax(1).reshape(-1)
    rows = feat.permute(0, 2, 3, 1).reshape(BN * HW, C)
    pt = torch.nonzero(cell >= 0)[:, 0]
    r = cell[pt]
    b, z, y, x = r % B, (r // B) % nx[2], (r // (B * nx[2])) % nx[1], r // (B * nx[2] * nx[1])
    flat = ((b * nx[2] + z) * nx[1] + y) * nx[0] + x
    pix = (pt // (D * HW)) * HW + pt % HW
    out = torch.zeros(B * nx[2] * nx[1] * nx[0], C, dtype=logit.dtype).index_add(0, flat, prob[pt][:, None] * rows[pix])
    return out.view(B, nx[2], nx[1], nx[0], C).permute(0, 1, 4, 2, 3).reshape(B, nx[2] * C, nx[1], nx[0])


def _splat_args(C, D, nz, final_dim):
    a = small_args()
    a["img_features"] = C
    a["data_aug_conf"] = dict(a["data_aug_conf"], final_dim=list(final_dim))
    a["grid_conf"] = dict(a["grid_conf"], xbound=[-51.2, 51.2, 6.4], ybound=[-51.2, 51.2, 6.4], zbound=[-10, 10, 20.0 / nz], ddiscr=[2, 50, D])
    return a


def _cams(g, special):
    c = {k: g[k].copy() for k in CAMS}
    if special:
        c["trans"][0, 1, 0] += 1000.0    # camera (0, 1) sees nothing: every cell -1
        c["rots"][1, 0] = 0.0            # camera (1, 0): every frustum point lands on its translation, one cell
    return c


# C: below a wave, the shipped small value, the m4 value (two channels per lane), past the 128-channel chunk; D: not a multiple of the four
# rows in flight, the shipped value, above 64 lanes; fH fW = 35 (two pixel tiles per camera, the second ragged) and 99; nz = 2
SPLAT_CASES = {"C1_D3": (1, 3, 1, (40, 56), False), "C8_D48_special_cameras": (8, 48, 1, (40, 56), True), "C128_D48": (128, 48, 1, (40, 56), False),
               "C160_D70_nz2": (160, 70, 2, (40, 56), False), "C8_D70_99px": (8, 70, 1, (72, 88), False)}


@pytest.mark.parametrize("case", list(SPLAT_CASES))
def test_splat_backward_vs_float64(g, case):
    """Measured on MI355X, relative rms error against float64, HIP (fp32 ATen autograd of the same restatement):
        C1_D3                   d_logit 1.99e-07 (1.06e-07)   d_feat 4.76e-08 (6.26e-08)
        C8_D48_special_cameras  d_logit 1.40e-07 (2.49e-07)   d_feat 1.65e-07 (1.50e-07)
        C128_D48                d_logit 1.64e-07 (2.02e-07)   d_feat 1.62e-07 (1.60e-07)
        C160_D70_nz2            d_logit 1.95e-07 (2.02e-07)   d_feat 2.09e-07 (1.97e-07)
        C8_D70_99px             d_logit 1.80e-07 (2.14e-07)   d_feat 2.01e-07 (1.96e-07)
    (every figure is under the 1e-6 floor of the criterion)."""
    C, D, nz, final_dim, special = SPLAT_CASES[case]
    m = LiftSplatShoot(_splat_args(C, D, nz, final_dim), trainable=True)
    B, N = 2, 2
    fH, fW = final_dim[0] // 8, final_dim[1] // 8
    nx = [16, 16, nz]
    rng = np.random.RandomState(11)
    logit = (2.0 * rng.standard_normal((B * N, D, fH, fW))).astype(np.float32)
    feat = rng.standard_normal((B * N, C, fH, fW)).astype(np.float32)
    G = cotangent(3, (B, nz * C, 16, 16))
    cams = [torch.from_numpy(v).to(DEV) for v in _cams(g, special).values()]
    lg, ft = torch.from_numpy(logit).to(DEV).requires_grad_(True), torch.from_numpy(feat).to(DEV).requires_grad_(True)
    out = m.splat_grad(lg, ft, *cams)
    with torch.no_grad():
        plain, cell = m.splat(lg.detach(), ft.detach(), *cams, return_cells=True)
    assert torch.equal(out.detach(), plain)
    out.backward(torch.from_numpy(G).to(DEV))
    torch.cuda.synchronize()
    cell = cell.cpu().long()
    assert (cell >= 0).sum() > 100
    if nz == 2:
        zs = (cell[cell >= 0] // B) % 2
        assert (zs == 0).any() and (zs == 1).any()
    res = {}
    for dtype in (torch.float64, torch.float32):
        l, f = torch.from_numpy(logit).to(dtype).requires_grad_(True), torch.from_numpy(feat).to(dtype).requires_grad_(True)
        o = dense_splat(l, f, cell, B, nx)
        (o * torch.from_numpy(G).to(dtype)).sum().backward()
        res[dtype] = (l.grad.numpy(), f.grad.numpy(), o.detach().numpy())
    r64, r32 = res[torch.float64], res[torch.float32]
    assert rel_rms(out.detach().cpu().numpy(), r64[2]) <= 1e-5
    for name, got, k in (("d_logit", lg.grad, 0), ("d_feat", ft.grad, 1)):
        got = got.cpu().numpy()
        e_hip, e_aten = rel_rms(got, r64[k]), rel_rms(r32[k], r64[k])
        print(f"splat backward {case} {name}: HIP {e_hip:.3e}, fp32 ATen {e_aten:.3e}")
        assert np.isfinite(got).all()
        assert e_hip <= max(2.0 * e_aten, 1e-6), (case, name, e_hip, e_aten)
    if special:
        HW = fH * fW
        cc = cell.view(B * N, D, HW)
        assert (cc[1] == -1).all() and len(torch.unique(cc[2])) == 1 and int(cc[2][0, 0]) >= 0
        assert torch.count_nonzero(lg.grad[1]) == 0 and torch.count_nonzero(ft.grad[1]) == 0   # sees nothing: exact zeros
        # one cell: every bin reads the same gradient row, so dprob is constant over d and the softmax backward cancels it
        assert float(lg.grad[2].abs().max()) <= 1e-5 * float(lg.grad.abs().max())
        assert torch.count_nonzero(ft.grad[2]) > 0


def test_splat_backward_is_deterministic_and_owns_its_workspace(g):
    """Two backward calls are bit-identical, and a second forward (other inputs, the shared and a fresh private workspace) between the
    forward and its backward does not change the gradients: what the backward reads lives in the autograd context."""
    C, D = 128, 48
    m = LiftSplatShoot(_splat_args(C, D, 1, (40, 56)), trainable=True)
    rng = np.random.RandomState(12)
    logit = torch.from_numpy((2.0 * rng.standard_normal((4, D, 5, 7))).astype(np.float32)).to(DEV)
    feat = torch.from_numpy(rng.standard_normal((4, C, 5, 7)).astype(np.float32)).to(DEV)
    G = torch.from_numpy(cotangent(4, (2, C, 16, 16))).to(DEV)
    cams = [torch.from_numpy(g[k]).to(DEV) for k in CAMS]

    def grads(disturb):
        lg, ft = logit.clone().requires_grad_(True), feat.clone().requires_grad_(True)
        out = m.splat_grad(lg, ft, *cams)
        if disturb:
            other = m.splat_grad((logit * -1.5).requires_grad_(True), feat.flip(0).requires_grad_(True), *[c.flip(0) for c in cams])
            with torch.no_grad():
                m.splat(logit * 0.5, feat + 1.0, *[c.flip(0) for c in cams])
            del other
        out.backward(G)
        return lg.grad, ft.grad

    a, b, c = grads(False), grads(False), grads(True)
    assert torch.count_nonzero(a[0]) > 0 and torch.count_nonzero(a[1]) > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("shape", [(2, 3, 7, 9), (1, 5, 8, 8)])
def test_maxpool_backward_vs_float64_autograd(shape):
    """Exact: the backward is a selection, and both x and dy lie on coarse grids here, so the at most four-term sums are exact in any
    order (no statement about torch's order is needed). Post-ReLU maps (exact-zero ties in most windows, ties among the positive
    values too) and a constant map (every window all-equal: the first element wins) pin the tie rule."""
    rng = np.random.RandomState(13)
    maps = [np.maximum(np.round(2 * rng.standard_normal(shape)) / 2, 0.0), np.full(shape, 0.75), np.zeros(shape),
            np.round(4 * rng.standard_normal(shape)) / 4]
    for i, xm in enumerate(maps):
        x64 = torch.from_numpy(xm).double().requires_grad_(True)
        y64 = F.max_pool2d(x64, 3, 2, 1)
        dy = np.round(16 * rng.standard_normal(tuple(y64.shape))) / 16
        y64.backward(torch.from_numpy(dy))
        if i == 0:
            assert (F.max_pool2d(-(x64.detach() == 0).double(), 3, 2, 1) == -1).any()   # windows of nothing but zeros exist
        x = torch.from_numpy(xm.astype(np.float32)).to(DEV).requires_grad_(True)
        y = maxpool3x3s2(x)
        assert y.requires_grad and torch.equal(y.detach().cpu().double(), y64.detach())
        y.backward(torch.from_numpy(dy.astype(np.float32)).to(DEV))
        assert torch.equal(x.grad.cpu().double(), x64.grad), (shape, i)


@pytest.mark.parametrize("shape", [(2, 3, 16, 20), (2, 3, 15, 19)])
def test_stem_weight_gradient_vs_float64_autograd(shape):
    """conv2d_hip(x, conv1, bn1, relu=True) under batch statistics: gradients of the 7x7 stride-2 pad-3 weight (gencomm_stem7x7_wgrad)
    and of the BatchNorm affine against float64 conv2d + batch_norm autograd; the same 2 x fp32-ATen criterion."""
    rng = np.random.RandomState(14)
    x = rng.standard_normal(shape).astype(np.float32)
    w = (0.1 * rng.standard_normal((64, 3, 7, 7))).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(64)).astype(np.float32), (0.2 * rng.standard_normal(64)).astype(np.float32)
    Ho, Wo = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    G = rng.standard_normal((shape[0], 64, Ho, Wo)).astype(np.float32)

    def torch_run(dtype):
        t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (w, gamma, beta)]
        y = F.batch_norm(F.conv2d(torch.from_numpy(x).to(dtype), t[0], None, 2, 3), None, None, t[1], t[2], True, 0.1, 1e-5).relu()
        (y * torch.from_numpy(G).to(dtype)).sum().backward()
        return [a.grad.numpy() for a in t], y.detach().numpy()

    (r64, y64), (r32, _) = torch_run(torch.float64), torch_run(torch.float32)
    conv, bn = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False), torch.nn.BatchNorm2d(64)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w)); bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
    conv, bn = conv.to(DEV), bn.to(DEV).train()
    y = conv2d_hip(torch.from_numpy(x).to(DEV), conv, bn, relu=True)
    assert tuple(y.shape) == (shape[0], 64, Ho, Wo) and rel_rms(y.detach().cpu().numpy(), y64) <= 1e-5
    (y * torch.from_numpy(G).to(DEV)).sum().backward()
    for name, got, k in (("conv1.weight", conv.weight.grad, 0), ("bn1.weight", bn.weight.grad, 1), ("bn1.bias", bn.bias.grad, 2)):
        e_hip, e_aten = rel_rms(got.cpu().numpy(), r64[k]), rel_rms(r32[k], r64[k])
        print(f"stem {shape} {name}: HIP {e_hip:.3e}, fp32 ATen {e_aten:.3e}")
        assert e_hip <= max(2.0 * e_aten, 1e-6), (shape, name, e_hip, e_aten)
    with pytest.raises(NotImplementedError, match="7x7 stride-2 pad-3 stem"):   # an input gradient of this layer is not built
        conv2d_hip(torch.from_numpy(x).to(DEV).requires_grad_(True), conv, bn, relu=True).sum().backward()


@pytest.mark.parametrize("D", [3, 48])
def test_depth_loss_kernel_vs_float64_composition(D):
    """gencomm_depth_focal_loss through depth_term (two depth_items keys in one dict) against the float64 composition: logits spread over
    +-30 (the softmax range: p_t from e^-60 to 1 - e^-30), targets at bin 0 and bin D - 1 among them. Value: relative error <= 1e-6 (per-pixel
    fp32 terms of a few ulp each, accumulated in float64); gradient: the 2 x fp32-ATen criterion, floored at 1e-6."""
    rng = np.random.RandomState(15 + D)
    items = []
    for shape in ((4, D, 5, 7), (3, D, 9, 11)):
        logit = rng.uniform(-30, 30, shape).astype(np.float32)
        tgt = rng.randint(0, D, (shape[0],) + shape[2:]).astype(np.int64)
        tgt[0, 0, :3], tgt[0, 1, :3] = 0, D - 1
        logit[0, :, 0, 0] = np.linspace(30, -30, D)     # target = the largest logit ...
        logit[0, :, 1, 0] = np.linspace(30, -30, D)     # ... and the smallest one
        items.append((logit, tgt))

    def run(dtype, dev, fuse):
        ls = [torch.from_numpy(l).to(dtype).to(dev).requires_grad_(True) for l, _ in items]
        out = {"depth_items": (ls[0], torch.from_numpy(items[0][1]).to(dev)), "depth_items_m2": (ls[1], torch.from_numpy(items[1][1]).to(dev))}
        total = depth_term(out, "", {"weight": 1.5}, fuse)
        total.backward()
        return float(total.detach()), [l.grad.cpu().numpy() for l in ls]

    v64, g64 = run(torch.float64, "cpu", False)
    v32, g32 = run(torch.float32, "cpu", False)
    v, gh = run(torch.float32, DEV, True)
    print(f"depth loss D={D}: value {v:.9g} vs float64 {v64:.9g} (rel {abs(v - v64) / abs(v64):.2e}; fp32 ATen {abs(v32 - v64) / abs(v64):.2e})")
    assert abs(v - v64) <= 1e-6 * abs(v64)
    for i in range(2):
        e_hip, e_aten = rel_rms(gh[i], g64[i]), rel_rms(g32[i], g64[i])
        print(f"depth loss D={D} key {i}: gradient HIP {e_hip:.3e}, fp32 ATen {e_aten:.3e}")
        assert np.isfinite(gh[i]).all() and e_hip <= max(2.0 * e_aten, 1e-6), (D, i, e_hip, e_aten)
    # the gradient scales with the incoming scalar
    l = torch.from_numpy(items[0][0]).to(DEV).requires_grad_(True)
    (3.0 * depth_term({"depth_items": (l, torch.from_numpy(items[0][1]).to(DEV))}, "", {"weight": 1.5})).backward()
    assert rel_rms(l.grad.cpu().numpy(), 3.0 * g64[0]) <= max(2.0 * rel_rms(g32[0], g64[0]), 1e-6)


def _torch_encoder(enc, x):
    """CamEncode_Resnet101's trunk and heads with torch's own operators on the module's layers (CPU, the module's dtype, the module's
    training flag: batch statistics and running-statistics updates in .train())."""
    x = F.max_pool2d(torch.relu(enc.bn1(enc.conv1(x))), 3, 2, 1)
    for blk in list(enc.layer1) + list(enc.layer2):
        idt = x if blk.downsample is None else blk.downsample[1](blk.downsample[0](x))
        out = torch.relu(blk.bn1(blk.conv1(x)))
        out = torch.relu(blk.bn2(blk.conv2(out)))
        x = torch.relu(blk.bn3(blk.conv3(out)) + idt)
    return enc.depth_head(x), enc.image_head(x)


def _fresh(trainable):
    m = LiftSplatShoot(small_args(), trainable=trainable).train()
    synth.fill_params_(m, SEED)
    synth.fill_running_stats_(m, SEED)
    return m


def test_training_step_vs_reference_fixture(g, gt):
    """One training step of LiftSplatShoot(small_args(), trainable=True).train(): L = <G, bev> + depth_loss, one backward.
    Every stored parameter gradient and running statistic against a float64 run (torch operators on the CPU, the dense restatement on
    the HIP cells): error <= max(2 e_ref, 1e-6), e_ref = the fp32 reference's own error against float64 (lss_train.npz).
    d depth_logit and d features per pixel against the reference's, leaving out pixels with any of their D points in another cell than
    the fixture's (at most 1 % may be left out: a condition, not a tolerance): against float64 the same criterion; against the
    reference's fp32 values 3 e_ref (its own e_ref plus the 2 e_ref of this side).
    Measured on MI355X (HIP error / e_ref): conv1.weight 1.89e-3 / 1.84e-3, bn1.weight 1.68e-3 / 1.70e-3, layer1.0.conv2.weight 1.89e-3 /
    1.85e-3, layer2.0.downsample.0.weight 3.37e-4 / 3.37e-4, layer2.3.bn3.bias 1.80e-4 / 1.80e-4, depth_head.weight 7.98e-6 / 7.71e-6,
    depth_head.bias 5.35e-6 / 5.80e-6, image_head.weight 6.09e-6 / 5.22e-6, running statistics 4.2e-8 - 7.0e-8 / 4.2e-8 - 6.4e-8,
    d_depth_logit 7.92e-6 / 7.35e-6 (6.41e-6 against the reference's fp32), d_feat 4.71e-6 / 4.34e-6 (3.90e-6); no pixel left out."""
    m = _fresh(True).to(DEV)
    inp = {k: torch.from_numpy(g[k].astype(np.float32)).to(DEV) for k in ("imgs",) + CAMS}
    kept = {}
    splat_grad = m.splat_grad

    def capture(dl, ft, *cams):
        ft.retain_grad()
        kept["feat"] = ft
        return splat_grad(dl, ft, *cams)

    m.splat_grad = capture
    bev = m({"inputs_m4": inp}, "m4")
    depth_logit, depth_gt = m.depth_items
    assert depth_logit.requires_grad and np.array_equal(depth_gt.cpu().numpy(), g["depth_gt_indices"])
    depth_logit.retain_grad()
    G = cotangent(SEED, tuple(bev.shape))
    l_bev = (torch.from_numpy(G).to(DEV) * bev).sum()
    l_depth = depth_term({"depth_items": m.depth_items}, "", {"weight": 1.0})
    (l_bev + l_depth).backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        _, cell = m.splat(depth_logit.detach(), kept["feat"].detach(), *[inp[k] for k in CAMS], return_cells=True)
    cell = cell.cpu().long()

    # float64 run on the HIP cells
    m64 = _fresh(False).double()
    imgs = torch.from_numpy(g["imgs"].astype(np.float64))
    B, N = imgs.shape[:2]
    dl64, ft64 = _torch_encoder(m64.camencode, imgs.view(B * N, *imgs.shape[2:])[:, :3])
    dl64.retain_grad(); ft64.retain_grad()
    bev64 = dense_splat(dl64, ft64, cell, B, [256, 256, 1])
    lb64 = (torch.from_numpy(G).double() * bev64).sum()
    ld64 = depth_focal_loss(dl64, torch.from_numpy(g["depth_gt_indices"])).mean()
    (lb64 + ld64).backward()

    for name, got, want, ref in (("loss_bev", l_bev, lb64, gt["loss_bev"]), ("loss_depth", l_depth, ld64, gt["loss_depth"])):
        print(f"{name}: HIP {float(got):.8g}, float64 {float(want):.8g}, reference fp32 {float(ref):.8g}")
        assert float(got) == pytest.approx(float(want), rel=1e-4) and float(ref) == pytest.approx(float(want), rel=1e-4)
    p32, p64 = dict(m.camencode.named_parameters()), dict(m64.camencode.named_parameters())
    b32, b64 = dict(m.camencode.named_buffers()), dict(m64.camencode.named_buffers())
    worst = []
    for key, got, want in [("grad__" + k, p32[k].grad, p64[k].grad) for k in PARAMS] + [("stat__" + k, b32[k], b64[k]) for k in STATS]:
        e_hip, e_ref = rel_rms(got.detach().cpu().numpy(), want.detach().numpy()), float(gt["e_ref__" + key])
        print(f"{key:45s} HIP {e_hip:.3e}   reference fp32 {e_ref:.3e}   (fixture vs this float64: {rel_rms(gt[key], want.detach().numpy()):.3e})")
        if e_hip > max(2.0 * e_ref, 1e-6):
            worst.append((key, e_hip, e_ref))
    # per-pixel gradients of the heads' outputs against the reference's
    want_cell = torch.from_numpy(g["cell"].astype(np.int64))
    D, HW = depth_logit.shape[1], depth_logit.shape[2] * depth_logit.shape[3]
    flipped = (cell.view(B * N, D, HW) != want_cell.view(B * N, D, HW)).any(1)            # [BN, HW]
    print(f"pixels left out (a frustum point in another cell than the fixture's): {int(flipped.sum())} of {flipped.numel()}")
    assert flipped.float().mean() <= 0.01
    keep = (~flipped).numpy()
    for key, got, want in (("d_depth_logit", depth_logit.grad, dl64.grad), ("d_feat", kept["feat"].grad, ft64.grad)):
        sel = lambda a: np.asarray(a).reshape(B * N, -1, HW).transpose(0, 2, 1)[keep]
        e_hip, e_ref = rel_rms(sel(got.cpu().numpy()), sel(want.numpy())), float(gt["e_ref__" + key])
        e_fix = rel_rms(sel(got.cpu().numpy()), sel(gt[key]))
        print(f"{key:45s} HIP vs float64 {e_hip:.3e}   reference fp32 {e_ref:.3e}   HIP vs reference fp32 {e_fix:.3e}")
        if e_hip > max(2.0 * e_ref, 1e-6) or e_fix > 3.0 * max(e_ref, 1e-6):
            worst.append((key, e_hip, e_ref, e_fix))
    assert not worst, worst


def test_refusals_that_stay(g):
    inp = {k: torch.from_numpy(g[k].astype(np.float32)).to(DEV) for k in ("imgs",) + CAMS}
    with pytest.raises(NotImplementedError, match="inference only"):
        _fresh(False).to(DEV)({"inputs_m4": inp}, "m4")
    with pytest.raises(NotImplementedError, match="stem"):
        _fresh(True).to(DEV)({"inputs_m4": dict(inp, imgs=inp["imgs"].clone().requires_grad_(True))}, "m4")
    m = _fresh(True).to(DEV)   # without gradients the trainable module is the inference path
    with torch.no_grad():
        out = m({"inputs_m4": inp}, "m4")
    assert not out.requires_grad and not m.depth_items[0].requires_grad
