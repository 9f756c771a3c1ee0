"""Shared pieces of the message-extractor kernel tests (test_gpu_msgext_kernels.py, test_msgext_oracle.py): the edge-offset
construction, an independent scalar restatement of one bilinear sample, and the float64 / float32 references. CPU only, no GPU import.

Edge offsets. Every value of the two sets below, added to an integer tap position of a map of at most a few hundred pixels, is exactly
representable in float32 (quarters of small integers; 1e6 + small integers < 2^24), except 3 W + 0.37, which is outside the map wherever
it lands. So the float32 kernels and the float64 truth see THE SAME sampling positions: the same cell, the same open-bound decision and,
in the backward, the same one-sided derivative at integral positions."""
import functools

import numpy as np
import torch

from oracle import torch_port as O

P = "bev_extractor."
NEAR = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.25, 1.75, -1.25)


def far_values(H, W):
    return (float(H), float(-H), float(W), float(-W), 3.0 * W + 0.37, 1e6, -1e6, 100.0)


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


def edge_offsets(n, H, W, seed, plant=0.0):
    """[n, 18, H, W] float32: per element with probability 0.9 from NEAR, else from far_values(H, W).
    plant > 0: additionally, that fraction of the pixels (chosen per pixel, so every 256-pixel workgroup of a large map gets some) has one
    coordinate of EVERY tap put exactly on -1, size, size - 1, 0, -0.5 or size - 0.5 -- on a large map the two sets alone reach the bounds
    only in the outermost rows and columns."""
    rng = np.random.RandomState(seed)
    near, far = np.asarray(NEAR, np.float32), np.asarray(far_values(H, W), np.float32)
    shape = (n, 18, H, W)
    off = np.where(rng.random_sample(shape) < 0.9, near[rng.randint(0, len(near), shape)], far[rng.randint(0, len(far), shape)]).astype(np.float32)
    if plant > 0.0:
        ys, xs = np.arange(H, dtype=np.float32).reshape(1, 1, H, 1), np.arange(W, dtype=np.float32).reshape(1, 1, 1, W)
        k = np.arange(9).reshape(1, 9, 1, 1)
        base = np.stack([np.broadcast_to(ys - 1 + k // 3, (n, 9, H, W)), np.broadcast_to(xs - 1 + k % 3, (n, 9, H, W))], 2)   # [n, 9, 2, H, W]
        size = np.asarray([H, W], np.float32).reshape(1, 1, 2, 1, 1)
        kind = rng.randint(0, 6, (n, 9, 1, H, W))
        target = np.choose(kind, [-1.0 + 0 * size, size, size - 1, 0 * size, -0.5 + 0 * size, size - 0.5])                     # [n, 9, 2, H, W]
        which = rng.randint(0, 2, (n, 9, 1, H, W)) == np.arange(2).reshape(1, 1, 2, 1, 1)                                      # the coordinate that is planted
        pixel = rng.random_sample((n, 1, 1, H, W)) < plant
        planted = (target - base).astype(np.float32)
        off = np.where((which & pixel).reshape(n, 18, H, W), planted.reshape(n, 18, H, W), off)
    return torch.from_numpy(off)


def tap_positions(off):
    """(py, px) [n, 9, H, W] float64 of every (pixel, tap): output position - 1 + tap + offset."""
    n, _, H, W = off.shape
    o = off.double()
    k = torch.arange(9).view(1, 9, 1, 1)
    py = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1) - 1 + k // 3 + o[:, 0::2]
    px = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W) - 1 + k % 3 + o[:, 1::2]
    return py, px


def edge_stats(off):
    """(fraction of (pixel, tap) positions inside the open interval (-1, H) x (-1, W), fraction with a coordinate exactly on -1, H or W,
    on-bound mask [n, 9, H, W])."""
    _, _, H, W = off.shape
    py, px = tap_positions(off)
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    bound = (py == -1) | (py == H) | (px == -1) | (px == W)
    return float(inside.double().mean()), float(bound.double().mean()), bound


def far_corner_count(off, tile=16, halo=4):
    """Number of (pixel, tap) positions inside the map whose upper-left corner lies outside the pixel's 16 x 16 tile grown by the 4-pixel
    halo of dcn_scatter_dx_tile_kernel: these corners take the kernel's direct global-atomic branch."""
    _, _, H, W = off.shape
    py, px = tap_positions(off)
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    ty0 = (torch.arange(H).view(1, 1, H, 1) // tile) * tile
    tx0 = (torch.arange(W).view(1, 1, 1, W) // tile) * tile
    iy, ix = torch.floor(py), torch.floor(px)
    far = (iy < ty0 - halo) | (iy >= ty0 + tile + halo) | (ix < tx0 - halo) | (ix >= tx0 + tile + halo)
    return int((inside & far & (iy >= 0) & (ix >= 0)).sum())


def bilinear_sample_scalar(plane, py, px):
    """One bilinear sample of plane [H][W] (nested lists of Python floats = float64) at (py, px), from the rule alone: zero outside the
    open interval (-1, size) in either coordinate; the four surrounding cells weighted by the products of (1 - distance) along each axis;
    a cell outside the map contributes zero."""
    H, W = len(plane), len(plane[0])
    if not (-1.0 < py < H and -1.0 < px < W):
        return 0.0
    y0, x0 = int(np.floor(py)), int(np.floor(px))
    total = 0.0
    for cy in (y0, y0 + 1):
        for cx in (x0, x0 + 1):
            if 0 <= cy < H and 0 <= cx < W:
                total += (1.0 - abs(py - cy)) * (1.0 - abs(px - cx)) * plane[cy][cx]
    return total


def identity_weight(C, dtype):
    """[9 C, C, 3, 3]: output channel c * 9 + k of the deformable convolution = sampled column (c, k) -- the layout of T.dcn_sample."""
    w = torch.zeros(C * 9, C, 3, 3, dtype=dtype)
    for c in range(C):
        for k in range(9):
            w[c * 9 + k, c, k // 3, k % 3] = 1.0
    return w


def sample_ref(x, off):
    """col [n, 9 C, H, W] in the dtype of x."""
    C = x.shape[1]
    return O.deform_conv2d_ref(x, off, identity_weight(C, x.dtype), None, 1)


def random_state_dict(C, seed):
    """A MessageExtractorv2 state dict (float32, CPU) with random parameters and the offset layer scaled as in
    test_gpu_parity.py::test_message_extractor_vs_oracle, so that taps really cross pixels."""
    from gencomm_amd import MessageExtractorv2, synth
    m = MessageExtractorv2(C, 2).eval()
    synth.fill_params_(m, seed)
    with torch.no_grad():
        m.bev_extractor.offset1.weight.mul_(6.0)
        m.bev_extractor.offset1.bias.mul_(10.0)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def exact_offset_state_dict(C, seed):
    """Parameters under which input channel k < 18 IS offset map k, bit for bit (offset1 = the centre tap of channel k, no bias), and the
    deformable convolution reads only channels 18 .. C - 1."""
    assert C > 18
    sd = random_state_dict(C, seed)
    w = torch.zeros_like(sd[P + "offset1.weight"])
    for k in range(18):
        w[k, k, 1, 1] = 1.0
    sd[P + "offset1.weight"] = w
    sd[P + "offset1.bias"] = torch.zeros(18)
    sd[P + "dcn1.weight"][:, :18] = 0.0
    return sd


def exact_offset_input(n, C, H, W, seed, plant=0.0):
    x = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal((n, C, H, W)).astype(np.float32))
    x[:, :18] = edge_offsets(n, H, W, seed, plant)
    return x


def module_from_col(sd, col):
    """The module output from sampled columns col [n, 9 C, H, W] (the layout of T.dcn_sample), in float64: the GEMM half of the deformable
    convolution, then the gate and the two 1x1 layers exactly as oracle.torch_port.message_extractor_forward applies them to b1."""
    import torch.nn.functional as F
    sd = {k: v.double() for k, v in sd.items()}
    wd = sd[P + "dcn1.weight"]
    b1 = torch.einsum("oc,bchw->bohw", wd.reshape(wd.shape[0], -1), col.double()) + sd[P + "dcn1.bias"].view(1, -1, 1, 1)
    g = b1.mean((2, 3), keepdim=True)
    g = F.relu(F.conv2d(g, sd[P + "attn.1.weight"], sd[P + "attn.1.bias"]))
    g = torch.sigmoid(F.conv2d(g, sd[P + "attn.3.weight"], sd[P + "attn.3.bias"]))
    h = F.relu(F.conv2d(b1 * g, sd[P + "fuse.0.weight"], sd[P + "fuse.0.bias"]))
    return F.conv2d(h, sd[P + "fuse.2.weight"], sd[P + "fuse.2.bias"])


@functools.lru_cache(maxsize=None)
def sampling_case(n, C, H, W, seed):
    """Random x and dcol, edge offsets; columns and gradients of sum(col * dcol) by autograd through deform_conv2d_ref in float64 (truth)
    and in float32 (yardstick). Shared like random_case."""
    rng = np.random.RandomState(seed)
    x = torch.from_numpy(rng.standard_normal((n, C, H, W)).astype(np.float32))
    dcol = torch.from_numpy(rng.standard_normal((n, C * 9, H, W)).astype(np.float32))
    off = edge_offsets(n, H, W, seed)
    case = {"x": x, "off": off, "dcol": dcol}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xd, od = x.to(dt).clone().requires_grad_(True), off.to(dt).clone().requires_grad_(True)
        col = sample_ref(xd, od)
        (col * dcol.to(dt)).sum().backward()
        case["col" + tag], case["dx" + tag], case["doff" + tag] = col.detach(), xd.grad.detach(), od.grad.detach()
    return case


def references(sd, x):
    """(truth float64, yardstick float32) of the module output, both on the CPU with the same oracle code."""
    with torch.no_grad():
        truth = O.message_extractor_forward({k: v.double() for k, v in sd.items()}, x.double())
        yard = O.message_extractor_forward(sd, x)
    return truth.numpy(), yard.numpy()


@functools.lru_cache(maxsize=None)
def random_case(n, C, H, W, seed):
    """(state dict, x, truth, yardstick) of a random-parameter case; computed once per process and shared (do not modify)."""
    from gencomm_amd import synth
    sd = random_state_dict(C, seed)
    x = torch.from_numpy(synth.make_inputs([n], C, H, W, seed + 1)["feat"])
    with torch.no_grad():
        off = torch.nn.functional.conv2d(x, sd[P + "offset1.weight"], sd[P + "offset1.bias"], padding=1)
    assert off.abs().max() > 1.5 and (off.abs() > 1.0).float().mean() > 0.05      # taps really move across pixels
    return (sd, x) + references(sd, x)


@functools.lru_cache(maxsize=None)
def exact_case(n, C, H, W, seed, plant=0.0):
    """(state dict, x, truth, yardstick) of an exact-edge-offset case; shared like random_case."""
    sd = exact_offset_state_dict(C, seed)
    x = exact_offset_input(n, C, H, W, seed, plant)
    return (sd, x) + references(sd, x)
