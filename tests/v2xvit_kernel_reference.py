"""Plain-torch restatements of the V2X-ViT building blocks behind gencomm_amd/csrc/v2xvit_kernels.h (test_gpu_v2xvit_kernels.py).

Every function is generic in dtype: called on float64 tensors it is the truth, called on the same values in float32 it is torch's own
fp32 error (the yardstick of bn_reference.Report.check). CPU only; gradients come from autograd.

  win_attn     BaseWindowAttention's core (sub_modules/mswin.py:47-83) with a relative position table
  hgt_attn     HGTCavAttention's core with one agent type and one relation (sub_modules/hmsa.py:117-150): attention across the agents of
               a scene, per pixel and head
  warp_affine  warp_affine_simple (utils/torch_transformation_utils.py:323-332)
  split3       SplitAttn (sub_modules/split_attn.py:31-62), radix 3, LayerNorm eps 1e-5, plus the residual the kernel adds"""
import torch
import torch.nn.functional as F


def window_cut(t, heads, dh, ws):
    """[n][heads dh][H][W] (head-major channels) -> [n][heads][windows, row-major][ws ws tokens, row-major][dh]"""
    n, _, H, W = t.shape
    return t.reshape(n, heads, dh, H // ws, ws, W // ws, ws).permute(0, 1, 3, 5, 4, 6, 2).reshape(n, heads, -1, ws * ws, dh)


def window_logits(qkv, pos, heads, dh, ws):
    """q k^T / sqrt(dh) + pos[ky - qy + ws - 1][kx - qx + ws - 1]: [n][heads][windows][query][key]"""
    inner = heads * dh
    q, k = (window_cut(qkv[:, i * inner:(i + 1) * inner], heads, dh, ws) for i in range(2))
    dots = torch.einsum("nmwic,nmwjc->nmwij", q, k) * dh ** -0.5
    ty = torch.arange(ws).repeat_interleave(ws)      # token = y * ws + x
    tx = torch.arange(ws).repeat(ws)
    ry = ty[None, :] - ty[:, None] + ws - 1          # [query][key] = key - query + ws - 1
    rx = tx[None, :] - tx[:, None] + ws - 1
    return dots + pos[ry, rx]


def win_attn(qkv, pos, heads, dh, ws):
    """qkv [n][3 heads dh][H][W] (q | k | v), pos [2 ws - 1][2 ws - 1] -> [n][heads dh][H][W]"""
    n, _, H, W = qkv.shape
    inner = heads * dh
    v = window_cut(qkv[:, 2 * inner:], heads, dh, ws)
    out = torch.einsum("nmwij,nmwjc->nmwic", window_logits(qkv, pos, heads, dh, ws).softmax(-1), v)
    out = out.reshape(n, heads, H // ws, W // ws, ws, ws, dh).permute(0, 1, 6, 2, 4, 3, 5)
    return out.reshape(n, inner, H, W)


def hgt_attn(qkv, lens, heads, dh):
    """qkv [n][3 heads dh][HW] (q | k | v), lens = agents per scene -> [n][heads dh][HW]"""
    n, _, HW = qkv.shape
    inner = heads * dh
    q, k, v = (qkv[:, i * inner:(i + 1) * inner].reshape(n, heads, dh, HW) for i in range(3))
    outs, off = [], 0
    for N in lens:
        sl = slice(off, off + N)
        s = torch.einsum("ihdp,jhdp->hpij", q[sl], k[sl]) * dh ** -0.5
        outs.append(torch.einsum("hpij,jhdp->ihdp", s.softmax(-1), v[sl]))
        off += N
    return torch.cat(outs).reshape(n, inner, HW)


def warp_affine(x, theta):
    """x [n][C][H][W], theta [n][2][3] float64 (normalised, ego <- agent). The grid is always made in float64 and cast to x's dtype: with
    x float64 this is the truth, with x float32 it is exactly warp_affine_simple."""
    grid = F.affine_grid(theta.double(), list(x.shape), align_corners=False).to(x.dtype)
    return F.grid_sample(x, grid, align_corners=False)


def split3_gates(a, b, c, fc1, ln_w, ln_b, fc2):
    """branch maps [n][C][HW] -> gates [n][3][C]"""
    n, C, _ = a.shape
    gap = (a + b + c).mean(-1)
    h = F.relu(F.layer_norm(F.linear(gap, fc1), (C,), ln_w, ln_b, 1e-5))
    return F.linear(h, fc2).reshape(n, 3, C).softmax(1)


def split3(a, b, c, fc1, ln_w, ln_b, fc2, res=None):
    g = split3_gates(a, b, c, fc1, ln_w, ln_b, fc2)
    out = a * g[:, 0, :, None] + b * g[:, 1, :, None] + c * g[:, 2, :, None]
    return out if res is None else out + res
