"""Torch restatements of MaxFusion (fusion_in_one.py:87-124) and Who2comFusion (:521-574) in any dtype, the case table of the max
backward tests and the near-tie mask. Shared by tests/test_fusion_train.py, tests/test_gpu_fusion_train.py and
tools/make_golden_fusion_train.py. Framework operators only: nothing here touches the HIP library."""
import math

import numpy as np
import torch
import torch.nn.functional as F

NEAR_TIE_REL = 1e-5      # top two warped values closer than this x max|x| without being equal: a near tie
NEAR_TIE_CAP = 1e-3      # the share of near ties a case may have


def warp_to_ego(xx, lens, affine_matrix):
    """Per scene the agents warped into the ego frame (warp_affine_simple: float64 affine grid cast to the input's dtype,
    bilinear, zeros, align_corners=False): list of [n_b, C, H, W]."""
    _, C, H, W = xx.shape
    out, o = [], 0
    for b, n in enumerate(lens):
        M = affine_matrix[b][0, :n].to(xx.device)
        grid = F.affine_grid(M, [n, C, H, W], align_corners=False).to(xx)
        out.append(F.grid_sample(xx[o:o + n], grid, align_corners=False))
        o += n
    return out


def max_fusion_forward(xx, lens, affine_matrix):
    return torch.stack([torch.max(w, dim=0)[0] for w in warp_to_ego(xx, lens, affine_matrix)])


def who2com_forward(weight, bias, xx, lens, affine_matrix):
    C = xx.shape[1]
    out, o = [], 0
    for w, n in zip(warp_to_ego(xx, lens, affine_matrix), lens):
        H, W = w.shape[2:]
        t = w.view(n, C, -1).permute(2, 0, 1)
        score = torch.bmm(t[:, :1], t.transpose(1, 2)) / math.sqrt(C)   # ego row only
        att = torch.bmm(F.softmax(score, -1), t)[:, 0].permute(1, 0).view(C, H, W)
        out.append(F.conv2d(torch.cat((xx[o], att), dim=0).unsqueeze(0), weight, bias, padding=1))
        o += n
    return torch.cat(out, dim=0)


def near_tie_mask(x, lens, affine_matrix):
    """bool [B, C, H, W]: the float64 top two warped values differ by less than NEAR_TIE_REL max|x| WITHOUT being equal. Exact ties
    are not near ties: they are what the winner rule is for."""
    x64 = torch.as_tensor(x).double()
    thr = NEAR_TIE_REL * float(x64.abs().max())
    out = []
    for w in warp_to_ego(x64, lens, torch.as_tensor(affine_matrix)):
        if w.shape[0] == 1:
            out.append(torch.zeros(w.shape[1:], dtype=torch.bool))
            continue
        top = torch.topk(w, 2, dim=0)[0]
        d = top[0] - top[1]
        out.append((d > 0) & (d < thr))
    return torch.stack(out)


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


# ------------------------------------------------------------------------------------------- transforms (normalised 2 x 3, float64)
def theta(H, W, cos=1.0, sin=0.0, tx=0.0, ty=0.0, scale=1.0):
    """Output pixel -> source pixel: rotate about the map centre by (cos, sin), scale, then shift by (tx, ty) PIXELS; as the
    normalised matrix affine_grid takes."""
    return np.array([[scale * cos, -scale * sin * H / W, 2.0 * tx / W], [scale * sin * W / H, scale * cos, 2.0 * ty / H]], np.float64)


def rot(H, W, angle, tx, ty, scale=1.0):
    return theta(H, W, math.cos(angle), math.sin(angle), tx, ty, scale)


def affine_of(scenes, L=8):
    """[B, L, L, 2, 3] with row [b, 0, j] = the j-th transform of scene b (the only rows the fusion nets read); identity elsewhere."""
    a = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (len(scenes), L, L, 1, 1))
    for b, ts in enumerate(scenes):
        for j, t in enumerate(ts):
            a[b, 0, j] = t
    return a


def probe(seed, shape):
    """Cotangent on a 1/4 grid, nowhere zero (so that the support of a gradient is the support of the winners' taps)."""
    rng = np.random.RandomState(seed)
    g = np.clip(np.round(4 * rng.standard_normal(shape)), -12, 12) / 4
    return np.where(g == 0, 0.25, g).astype(np.float32)


# Translations are fractional pixels on purpose: a bilinear cell whose corner falls within rounding of a lattice point is a different
# cell in float32 and in float64, and such residue is not what these cases are about. The exact cases (identity; half a pixel along
# H = 16, where every quantity is dyadic) are exact in both.
def _scenes(name, H, W):
    I = theta(H, W)
    outside = theta(H, W, tx=3.0 * W + 0.37)
    r90, r180 = theta(H, W, 0.0, 1.0, 1.37, 0.61), theta(H, W, -1.0, 0.0, -2.63, 1.37)
    if name == "identity_ties":
        return [[I], [I, I, I], [I, I]]
    if name == "rigid_relu":
        return [[I], [I, r90, r180], [I, outside]]
    if name == "halfpix_quant":
        half = theta(H, W, ty=0.5)
        return [[I, half, half]]
    if name == "max_agents":
        return [[I, rot(H, W, 0.3, 2.37, -1.61), r90, r180, rot(H, W, -1.2, -4.21, 3.43), theta(H, W, tx=0.5), outside, rot(H, W, 2.5, 6.11, -2.27)]]
    if name == "nontame":
        return [[I], [I, rot(H, W, 0.2, 1.37, -0.61, scale=0.4), rot(H, W, 0.5, -1.29, 2.43)], [I, r180]]
    raise KeyError(name)


#            name              C   H   W   record_len  inputs        rigid (every agent on a deterministic path)
CASES = {"identity_ties": (1, 7, 9, [1, 3, 2], "equal", True),
         "rigid_relu": (5, 33, 65, [1, 3, 2], "relu", True),
         "halfpix_quant": (5, 16, 24, [3], "quant", True),
         "max_agents": (64, 33, 65, [8], "normal", True),
         "nontame": (5, 16, 24, [1, 3, 2], "normal", False)}


def build_case(name):
    """x [n, C, H, W] float32, record_len, affine [B, 8, 8, 2, 3] float64, probe G [B, C, H, W] float32."""
    C, H, W, rl, kind, _ = CASES[name]
    seed = 7000 + sorted(CASES).index(name)
    rng = np.random.RandomState(seed)
    n = sum(rl)
    x = rng.standard_normal((n, C, H, W))
    if kind == "relu":
        # half exact zeros on every agent but the egos: where the ego is negative and the others are zero (or out of range), agents tie
        # at an exact 0. The egos stay continuous: an identity warp on a map whose size is no power of two leaves rounding residue of its
        # neighbours in float64 (1e-16 against an exact 0), which the near-tie rule would count by the thousand.
        ego, o = [], 0
        for k in rl:
            ego.append(o)
            o += k
        keep = x[ego].copy()
        x = np.maximum(x, 0.0)
        x[ego] = keep
    elif kind == "equal":                   # every agent of a scene carries the ego's map: all-agent ties everywhere
        o = 0
        for k in rl:
            x[o:o + k] = x[o]
            o += k
    elif kind == "quant":
        # multiples of 1/4. Agents 1 and 2 share one transform (half a pixel along H = 16: tap weights exactly 1/2) and hold integers
        # 0..3, so their warped values are half-integers; rows 0-3 and 8-11 of agent 2 equal agent 1's (exact non-zero ties: agent 1 must
        # win), rows 4-7 are one higher and rows 12-15 one lower (no tie). The ego holds odd multiples of 1/4: it never ties with them.
        x1 = rng.randint(0, 4, size=(C, H, W)).astype(np.float64)
        band = np.zeros((1, H, 1))
        band[:, 4:8], band[:, 12:16] = 1.0, -1.0
        x[1], x[2] = x1, x1 + band
        x[0] = (2 * rng.randint(0, 6, size=(C, H, W)) + 1) / 4.0
    return x.astype(np.float32), rl, affine_of(_scenes(name, H, W)), probe(seed + 1, (len(rl), C, H, W))


def reference_grads(x, rl, affine, G):
    """The restatement on the CPU in float64 and float32 (ATen autograd): {dtype: (out, dx)} as numpy."""
    res = {}
    for dtype in (torch.float64, torch.float32):
        xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
        out = max_fusion_forward(xx, rl, torch.from_numpy(affine))
        (out * torch.from_numpy(G).to(dtype)).sum().backward()
        res[dtype] = (out.detach().numpy(), xx.grad.numpy())
    return res
