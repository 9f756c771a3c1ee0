"""Plain-torch restatement of the reference's CoBEVT fusion (opencood/models/fuse_modules/fusion_in_one.py:409-464, the blocks of
fuse_modules/swap_fusion_modules.py:13-192, regroup of fuse_utils.py:13-64), and the case table of tests/golden/cobevt.npz
(tools/make_golden_cobevt.py). Written from the formulas, with reshapes and permutes in place of einops; never reads the reference.
It works from a ``state_dict`` (the reference's keys), in the dtype of ``x``: float32 like the reference's run, or float64.

Per block: x = x + to_out(attention(to_qkv(LN(x)))), x = x + FFN(LN(x)), once over ws x ws windows and once over the strided grid
partition; the attention is over the (agent, w1, w2) tokens of a group jointly, with the 3-D relative position bias and the keys of
padded agents masked. Padded agents are zero rows going in, queries like any other, and part of the final mean over all L rows.
"""
import numpy as np
import torch
import torch.nn.functional as F

# case -> input_dim (= mlp_dim), dim_head, window_size, agent_size L, H, W, depth, record_len   (the table of the issue)
CASES = {
    "a": dict(C=32, dim_head=16, ws=4, L=3, H=8, W=12, depth=2, record_len=[2, 3]),
    "b": dict(C=64, dim_head=32, ws=4, L=5, H=8, W=16, depth=1, record_len=[1, 4]),
    "c": dict(C=64, dim_head=32, ws=8, L=5, H=16, W=24, depth=1, record_len=[5, 2]),
    "d": dict(C=256, dim_head=32, ws=4, L=5, H=16, W=16, depth=3, record_len=[3]),     # the shipped `cobevt:` block
    "e": dict(C=64, dim_head=64, ws=4, L=2, H=8, W=8, depth=1, record_len=[2]),
}


def case_args(c):
    return {"input_dim": c["C"], "mlp_dim": c["C"], "agent_size": c["L"], "window_size": c["ws"], "dim_head": c["dim_head"],
            "drop_out": 0.1, "depth": c["depth"]}


def make_affine(record_len, L, H, W, seed, identity_scenes=()):
    """Normalised ego <- agent matrices [B, L, L, 2, 3] float64 (what normalize_pairwise_tfm hands the fusion): rotations of a few tenths
    of a radian plus translations; the LAST valid agent of every scene is shifted by about 0.9 of the half-extent, partly out of the map.
    Only row [b, 0, j] is read by the fusion. Scenes in `identity_scenes` keep identity poses."""
    rng = np.random.RandomState(seed)
    aff = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (len(record_len), L, L, 1, 1))
    for b, n in enumerate(record_len):
        if b in identity_scenes:
            continue
        for j in range(1, n):
            yaw = rng.uniform(0.1, 0.4) * rng.choice([-1.0, 1.0])
            tx, ty = rng.uniform(-0.4, 0.4, 2)
            if j == n - 1:
                tx = 0.9 * rng.choice([-1.0, 1.0])
            c, s = np.cos(yaw), np.sin(yaw)
            aff[b, 0, j] = [[c, -s * H / W, tx], [s * W / H, c, ty]]
    return aff


def make_inputs(c, seed):
    """Post-ReLU normals [sumN, C, H, W] float32 and the affine matrices of a case."""
    rng = np.random.RandomState(seed)
    x = np.maximum(rng.standard_normal((sum(c["record_len"]), c["C"], c["H"], c["W"])), 0.0).astype(np.float32)
    return x, make_affine(c["record_len"], c["L"], c["H"], c["W"], seed + 1)


def relative_position_index(L, ws):
    """[L ws ws, L ws ws] int64, the buffer the module registers (swap_fusion_modules.py:63-85)."""
    l, h, w = torch.meshgrid(torch.arange(L), torch.arange(ws), torch.arange(ws), indexing="ij")
    l, h, w = l.reshape(-1), h.reshape(-1), w.reshape(-1)
    p = 2 * ws - 1
    return (l[:, None] - l[None, :] + L - 1) * p * p + (h[:, None] - h[None, :] + ws - 1) * p + (w[:, None] - w[None, :] + ws - 1)


def to_groups(x, ws, grid):
    """[B, L, C, H, W] -> [B X Y, L ws ws, C]: tokens (l, w1, w2) of window (x, y) -- '(x w1) (y w2)' -- or of grid cell (x, y) -- '(w1 x) (w2 y)'."""
    B, L, C, H, W = x.shape
    X, Y = H // ws, W // ws
    if grid:
        t = x.reshape(B, L, C, ws, X, ws, Y).permute(0, 4, 6, 1, 3, 5, 2)   # b x y l w1 w2 c
    else:
        t = x.reshape(B, L, C, X, ws, Y, ws).permute(0, 3, 5, 1, 4, 6, 2)
    return t.reshape(B * X * Y, L * ws * ws, C)


def from_groups(t, shape, ws, grid):
    B, L, C, H, W = shape
    X, Y = H // ws, W // ws
    t = t.reshape(B, X, Y, L, ws, ws, C)
    if grid:
        return t.permute(0, 3, 6, 4, 1, 5, 2).reshape(B, L, C, H, W)     # b l c w1 x w2 y
    return t.permute(0, 3, 6, 1, 4, 2, 5).reshape(B, L, C, H, W)         # b l c x w1 y w2


def swap_attention(qkv, table, index, nvalid, L, ws, heads, grid):
    """The attention core on projected maps: qkv [B, L, 3 inner, H, W] (q | k | v, head-major), table [n_idx, heads], index [T, T],
    nvalid [B] -> [B, L, inner, H, W]."""
    B, _, c3, H, W = qkv.shape
    inner = c3 // 3
    dh = inner // heads
    g = to_groups(qkv, ws, grid)                                          # [G, T, 3 inner]
    G, T, _ = g.shape
    q, k, v = (g[:, :, i * inner:(i + 1) * inner].reshape(G, T, heads, dh).permute(0, 2, 1, 3) for i in range(3))
    sim = torch.matmul(q * dh ** -0.5, k.transpose(-1, -2)) + table[index.to(table.device)].permute(2, 0, 1).to(q.dtype)[None]
    agent_of_key = torch.arange(T, device=qkv.device) // (ws * ws)
    per_scene = (H // ws) * (W // ws)
    valid = agent_of_key[None, :] < torch.as_tensor(nvalid, device=qkv.device).repeat_interleave(per_scene)[:, None]          # [G, T]
    sim = sim.masked_fill(~valid[:, None, None, :], -float("inf"))
    out = torch.matmul(torch.softmax(sim, dim=-1), v)                     # [G, heads, T, dh]
    return from_groups(out.permute(0, 2, 1, 3).reshape(G, T, inner), (B, L, inner, H, W), ws, grid)


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def cobevt_forward(sd, args, x, record_len, affine_matrix):
    """sd: state_dict with the reference's keys; x [sumN, C, H, W]; affine_matrix [B, L, L, 2, 3] -> [B, C, H, W] in x's dtype."""
    dt = x.dtype
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    n, C, H, W = x.shape
    B, L = affine_matrix.shape[:2]
    ws, heads = args["window_size"], args["input_dim"] // args["dim_head"]
    lens = [int(v) for v in record_len]
    feat = x.new_zeros(B, L, C, H, W)
    off = 0
    for b, k in enumerate(lens):
        feat[b, :k] = x[off:off + k]
        off += k
    for b in range(B):   # warp_affine_simple: the float64 grid is cast to the map's dtype before sampling
        grid = F.affine_grid(affine_matrix[b, 0], [L, C, H, W], align_corners=False).to(dt)
        feat[b] = F.grid_sample(feat[b], grid, align_corners=False)
    for i in range(args["depth"]):
        for part, is_grid in (("window", False), ("grid", True)):
            p = f"layers.{i}.{part}_attention."
            hn = _ln(feat.permute(0, 1, 3, 4, 2), sd[p + "norm.weight"], sd[p + "norm.bias"])
            qkv = (hn @ sd[p + "fn.to_qkv.weight"].t()).permute(0, 1, 4, 2, 3)
            att = swap_attention(qkv, sd[p + "fn.relative_position_bias_table.weight"], sd[p + "fn.relative_position_index"], lens, L, ws,
                                 heads, is_grid)
            feat = feat + (att.permute(0, 1, 3, 4, 2) @ sd[p + "fn.to_out.0.weight"].t()).permute(0, 1, 4, 2, 3)
            p = f"layers.{i}.{part}_ffd."
            hn = _ln(feat.permute(0, 1, 3, 4, 2), sd[p + "norm.weight"], sd[p + "norm.bias"])
            mid = F.gelu(hn @ sd[p + "fn.net.0.weight"].t() + sd[p + "fn.net.0.bias"])
            feat = feat + (mid @ sd[p + "fn.net.3.weight"].t() + sd[p + "fn.net.3.bias"]).permute(0, 1, 4, 2, 3)
    m = feat.mean(dim=1).permute(0, 2, 3, 1)
    m = _ln(m, sd["mlp_head.2.weight"], sd["mlp_head.2.bias"])
    return (m @ sd["mlp_head.3.weight"].t() + sd["mlp_head.3.bias"]).permute(0, 3, 1, 2).contiguous()
