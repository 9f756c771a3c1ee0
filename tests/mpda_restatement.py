"""Plain-torch restatement of MPDA's feature aligner (``opencood/models/mpda_modules``; the loop of
``heter_model_baseline_w_mpda.py:232-262``), written without einops from the modules' definitions: the float64 reference of the two
new kernels, the case table of tests/golden/mpda.npz (tools/make_golden_mpda.py) and the inputs of every case (drawn from seeds on
both sides, never stored).

Partitions of an NCHW map into 2 x 2 groups, X = H / 2, Y = W / 2, token t = 2 w1 + w2:
  window  'b d (x w1) (y w2) -> b x y w1 w2 d'   pixel (2 x + w1, 2 y + w2)
  grid    'b d (w1 x) (w2 y) -> b x y w1 w2 d'   pixel (w1 X + x, w2 Y + y)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

SEED = 5200

# ---------------------------------------------------------------------------------------------------------------- case tables
# Module cases. H x W is the ego's map (X != Y everywhere, so a swapped partition shows); `cav_hw` the collaborators' map where the
# resizer really resizes; `record_len` the scenes of the MPDAAlign run (an ego-only scene, one with several collaborators, one with one).
CASES = {
    "c32": dict(C=32, cin=32, dim_head=32, heads=2, mlp_dim=64, H=4, W=6, cav_hw=(4, 6), n_cav=3, record_len=[1, 3, 2], rebuttal=False),
    "c32_resize": dict(C=32, cin=48, dim_head=32, heads=2, mlp_dim=64, H=4, W=6, cav_hw=(6, 10), n_cav=2, record_len=None, rebuttal=False),
    "c32_rebuttal": dict(C=32, cin=32, dim_head=32, heads=2, mlp_dim=64, H=4, W=6, cav_hw=(4, 6), n_cav=1, record_len=[1, 3, 2], rebuttal=True),
    "c128": dict(C=128, cin=128, dim_head=32, heads=16, mlp_dim=256, H=4, W=6, cav_hw=(4, 6), n_cav=1, record_len=[2], rebuttal=False),   # the shipped widths
}

# gencomm_quad_attn_fwd: (H, W) maps -- a single group; 4 x 6; 6 x 10 = 15 groups, odd against any tile of lanes; 8 x 132 = 264 groups,
# more than one 256-thread workgroup
QUAD_MAPS = ((2, 2), (4, 6), (6, 10), (8, 132))
QUAD_HEADS = (1, 4, 16)
# gencomm_resize_bilinear_fwd: (Hi, Wi) -> (Ho, Wo)
RESIZE_CASES = (((8, 12), (4, 6)), ((4, 6), (6, 10)), ((5, 7), (5, 7)), ((2, 2), (7, 3)))


def shipped_args():
    """``resizer`` / ``cdt`` as in GenComm_yamls/baselines/stage2/MPDA/m1m3_att.yaml (no ``classifier`` key: DAImgHead(128))."""
    return {"resizer": {"input_channel": 128, "output_channel": 128,
                        "wg_att": {"input_dim": 128, "mlp_dim": 256, "window_size": 2, "dim_head": 32, "drop_out": 0.1, "depth": 1},
                        "residual": {"input_dim": 128, "depth": 2}},
            "cdt": {"input_dim": 128, "window_size": 2, "dim_head": 32, "heads": 16, "depth": 1}}


def case_args(c):
    """The ``model.args`` keys MPDAAlign reads, at a case's widths (cdt.window_size 8 on purpose: the block ignores it)."""
    C = c["C"]
    return {"resizer": {"input_channel": c["cin"], "output_channel": C,
                        "wg_att": {"input_dim": C, "mlp_dim": c["mlp_dim"], "window_size": 2, "dim_head": c["dim_head"], "drop_out": 0.1, "depth": 1},
                        "residual": {"input_dim": C, "depth": 2}},
            "cdt": {"input_dim": C, "window_size": 8, "dim_head": c["dim_head"], "heads": c["heads"], "depth": 1},
            "classifier": C, "rebuttal": c["rebuttal"]}


def case_seeds(tag):
    """(resizer, cdt, classifier, aligner) parameter seeds of a case; BatchNorm statistics use seed + 50."""
    base = SEED + 100 * list(CASES).index(tag)
    return base, base + 1, base + 2, base + 3


def case_inputs(tag):
    """float32 arrays of a case: ego [1, C, H, W], cav [n_cav, cin, h, w] (the resizer's input), cdt_cav [n_cav, C, H, W] (the
    encoder's own input), and x [sum(record_len), C, H, W] for the aligner (None where the case has no record_len)."""
    c = CASES[tag]
    rng = np.random.RandomState(SEED + 100 * list(CASES).index(tag) + 10)
    draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    ego = draw(1, c["C"], c["H"], c["W"])
    cav = draw(c["n_cav"], c["cin"], *c["cav_hw"])
    cdt_cav = draw(c["n_cav"], c["C"], c["H"], c["W"])
    x = draw(sum(c["record_len"]), c["C"], c["H"], c["W"]) if c["record_len"] else None
    return ego, cav, cdt_cav, x


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


# ---------------------------------------------------------------------------------------------------------------- the two kernels
def to_groups(x, grid):
    """[b, d, H, W] -> [b, X Y, 4, d], token t = 2 w1 + w2."""
    b, d, H, W = x.shape
    X, Y = H // 2, W // 2
    if grid:
        t = x.reshape(b, d, 2, X, 2, Y).permute(0, 3, 5, 2, 4, 1)     # b x y w1 w2 d
    else:
        t = x.reshape(b, d, X, 2, Y, 2).permute(0, 2, 4, 3, 5, 1)
    return t.reshape(b, X * Y, 4, d)


def from_groups(t, grid, H, W):
    """The inverse: [b, X Y, 4, d] -> [b, d, H, W]."""
    b, _, _, d = t.shape
    X, Y = H // 2, W // 2
    t = t.reshape(b, X, Y, 2, 2, d)
    if grid:
        return t.permute(0, 5, 3, 1, 4, 2).reshape(b, d, H, W)          # b d w1 x w2 y
    return t.permute(0, 5, 1, 3, 2, 4).reshape(b, d, H, W)              # b d x w1 y w2


def rel_pos_indices(window_size=2):
    """The ``rel_pos_indices`` buffer of wg_fusion_modules.Attention, restated: [ws ws, ws ws] rows of the bias table."""
    pos = torch.arange(window_size)
    hh, ww = torch.meshgrid(pos, pos, indexing="ij")
    g = torch.stack([hh.reshape(-1), ww.reshape(-1)], dim=1)
    rel = g[:, None, :] - g[None, :, :] + window_size - 1
    return rel[..., 0] * (2 * window_size - 1) + rel[..., 1]


def quad_attention(q, k, v, table, index, heads, dim_head, grid):
    """softmax(dim_head^-0.5 q k^T + table[index]) v inside every 2 x 2 group, per head: q [N, heads dim_head, H, W], k and v [N or 1, ...]
    in the dtype of q; table [9, heads] or None, index [4, 4] -> [N, heads dim_head, H, W]."""
    N, _, H, W = q.shape
    if k.shape[0] != N:
        k, v = k.expand(N, -1, -1, -1), v.expand(N, -1, -1, -1)
    split = lambda t: to_groups(t, grid).reshape(N, -1, 4, heads, dim_head).permute(0, 3, 1, 2, 4)     # N heads G 4 d
    qg, kg, vg = split(q), split(k), split(v)
    sim = dim_head ** -0.5 * (qg @ kg.transpose(-1, -2))
    if table is not None:
        sim = sim + table[index].permute(2, 0, 1)[None, :, None]                                        # [4, 4, heads] -> 1 heads 1 4 4
    out = sim.softmax(dim=-1) @ vg
    return from_groups(out.permute(0, 2, 3, 1, 4).reshape(N, -1, 4, heads * dim_head), grid, H, W)


def resize(x, size):
    return F.interpolate(x, size=list(size), mode="bilinear", align_corners=False)


# ---------------------------------------------------------------------------------------------------------------- the modules
def _ln(x, sd, p):
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5).permute(0, 3, 1, 2)


def _lin(x, sd, p):
    return F.linear(x.permute(0, 2, 3, 1), sd[p + ".weight"], sd.get(p + ".bias")).permute(0, 3, 1, 2)


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _mlp_head(sd, q, x):
    """q: the module's prefix with its dot, or ''."""
    return _lin(_ln(x, sd, q + "mlp_head.1"), sd, q + "mlp_head.2")


def swap_encoder(sd, p, x, dim_head, depth=1):
    """SwapFusionEncoder (unmasked): per block window attention, FeedForward, grid attention, FeedForward; then mlp_head."""
    heads, index, q_ = x.shape[1] // dim_head, rel_pos_indices(2), (p + ".") if p else ""
    for i in range(depth):
        for at, grid in ((1, False), (5, True)):
            a, f = f"{q_}layers.{i}.block.{at}", f"{q_}layers.{i}.block.{at + 1}"
            q, k, v = _lin(_ln(x, sd, a + ".norm"), sd, a + ".fn.to_qkv").chunk(3, dim=1)
            x = x + _lin(quad_attention(q, k, v, sd[a + ".fn.rel_pos_bias.weight"], index, heads, dim_head, grid), sd, a + ".fn.to_out.0")
            x = x + _lin(F.gelu(_lin(_ln(x, sd, f + ".norm"), sd, f + ".fn.net.0")), sd, f + ".fn.net.3")
    return _mlp_head(sd, q_, x)


def resizer(sd, p, ego, cav, dim_head, res_depth=2):
    """LearnableResizer.forward(ego_feature, cav_feature)."""
    q = (p + ".") if p else ""
    size = ego.shape[2:]
    cav = F.conv2d(cav, sd[q + "channel_selector.weight"], sd[q + "channel_selector.bias"])
    one = resize(swap_encoder(sd, q + "wg_att_1", cav, dim_head), size)
    two = one
    for i in range(res_depth):
        m = f"{q}res_blocks.{i}.module"
        h = F.leaky_relu(_bn(F.conv2d(two, sd[m + ".0.weight"], sd[m + ".0.bias"], padding=1), sd, m + ".1"), 0.01)
        two = two + _bn(F.conv2d(h, sd[m + ".3.weight"], sd[m + ".3.bias"], padding=1), sd, m + ".4")
    two = swap_encoder(sd, q + "wg_att_2", two + one, dim_head)
    return resize(cav, size) + two


def cdt(sd, p, ego, cav, heads, dim_head, depth=1):
    """CrossDomainFusionEncoder.forward(ego_feature, cav_feature): queries from the collaborator, keys and values from the ego."""
    q_ = (p + ".") if p else ""
    x = cav
    for i in range(depth):
        b = f"{q_}layers.{i}"
        for cw, norm, mlp, grid in (("cross_win_1", "prenorm1", "mlp_1", False), ("cross_win_2", "prenorm2", "mlp_2", True)):
            c = f"{b}.{cw}"
            q = _lin(_ln(x, sd, c + ".to_q.0"), sd, c + ".to_q.1")
            k = _lin(_ln(ego, sd, c + ".to_k.0"), sd, c + ".to_k.1")
            v = _lin(_ln(ego, sd, c + ".to_v.0"), sd, c + ".to_v.1")
            x = _lin(quad_attention(q, k, v, None, None, heads, dim_head, grid), sd, c + ".proj") + x
            x = x + _lin(F.gelu(_lin(_ln(x, sd, f"{b}.{norm}"), sd, f"{b}.{mlp}.0")), sd, f"{b}.{mlp}.2")
        x = _ln(x, sd, b + ".post_norm")
    return _mlp_head(sd, q_, x)


def da_head(sd, p, x):
    q = (p + ".") if p else ""
    return F.conv2d(F.relu(F.conv2d(x, sd[q + "conv1_da.weight"], sd[q + "conv1_da.bias"])), sd[q + "conv2_da.weight"], sd[q + "conv2_da.bias"])


def mpda_align(sd, args, x, record_len):
    """heter_model_baseline_w_mpda.py:232-262 on a state_dict with the prefixes resizer / cdt / classifier -> (features, logits)."""
    dh_r, c = args["resizer"]["wg_att"]["dim_head"], args["cdt"]
    feats, logits, off = [], [], 0
    for n in record_len:
        ego = x[off:off + 1]
        if n == 1:
            scene = ego          # the reference aligns the ego to itself here and discards the result
        else:
            cav = x[off + 1:off + n]
            if not args.get("rebuttal", False):
                cav = cdt(sd, "cdt", ego.expand(n - 1, -1, -1, -1), resizer(sd, "resizer", ego, cav, dh_r), c["heads"], c["dim_head"])
            scene = torch.cat((ego, cav), dim=0)
        feats.append(scene)
        logits.append(da_head(sd, "classifier", scene))
        off += n
    return torch.cat(feats, dim=0), torch.cat(logits, dim=0)


def double_sd(module):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in module.state_dict().items()}
