"""Training restatement of the CoBEVT fusion: ``cobevt_restatement.cobevt_forward`` with the dropouts of ``train()`` mode as explicit
masks, and its gradients by torch autograd, in float64 or float32. Built from the pieces of tests/cobevt_restatement.py (``swap_attention``,
``_ln``); never reads the reference.

``masks``: None (dropout inactive: ``eval()``), or the list of already scaled masks ``(rand >= p) / (1 - p)`` in the order the module draws
them -- per block: window ``to_out``, window FFN after the GELU, window FFN after the last Linear, then the same three for grid -- each
in the shape of the padded NCHW batch it multiplies, ``[B L, channels, H, W]``.
"""
import torch
import torch.nn.functional as F

import cobevt_restatement as R


def param_names(sd):
    """The trainable entries of a CoBEVT state_dict, in order (everything but the relative_position_index buffers)."""
    return [k for k, v in sd.items() if v.is_floating_point()]


def cobevt_train_forward(sd, args, x, record_len, affine_matrix, masks=None):
    """As R.cobevt_forward; differentiable in x and every floating entry of sd (which must already have x's dtype)."""
    dt = x.dtype
    n, C, H, W = x.shape
    B, L = affine_matrix.shape[:2]
    ws, heads = args["window_size"], args["input_dim"] // args["dim_head"]
    lens = [int(v) for v in record_len]
    masks = None if masks is None else list(masks)

    def drop(t):   # t [B, L, C', H, W]
        if masks is None:
            return t
        m = masks.pop(0)
        assert m.shape == (B * L, t.shape[2], H, W), (m.shape, t.shape)
        return t * m.to(dt).reshape(B, L, t.shape[2], H, W)

    rows, off = [], 0
    for b, k in enumerate(lens):
        grid = F.affine_grid(affine_matrix[b, 0, :k], [k, C, H, W], align_corners=False).to(dt)
        rows.append(torch.cat([F.grid_sample(x[off:off + k], grid, align_corners=False), x.new_zeros(L - k, C, H, W)]))
        off += k
    feat = torch.stack(rows)                                              # [B, L, C, H, W], zero rows for the padded agents
    for i in range(args["depth"]):
        for part, is_grid in (("window", False), ("grid", True)):
            p = f"layers.{i}.{part}_attention."
            hn = R._ln(feat.permute(0, 1, 3, 4, 2), sd[p + "norm.weight"], sd[p + "norm.bias"])
            qkv = (hn @ sd[p + "fn.to_qkv.weight"].t()).permute(0, 1, 4, 2, 3)
            att = R.swap_attention(qkv, sd[p + "fn.relative_position_bias_table.weight"], sd[p + "fn.relative_position_index"], lens, L, ws,
                                   heads, is_grid)
            feat = feat + drop((att.permute(0, 1, 3, 4, 2) @ sd[p + "fn.to_out.0.weight"].t()).permute(0, 1, 4, 2, 3))
            p = f"layers.{i}.{part}_ffd."
            hn = R._ln(feat.permute(0, 1, 3, 4, 2), sd[p + "norm.weight"], sd[p + "norm.bias"])
            mid = drop(F.gelu(hn @ sd[p + "fn.net.0.weight"].t() + sd[p + "fn.net.0.bias"]).permute(0, 1, 4, 2, 3))
            feat = feat + drop((mid.permute(0, 1, 3, 4, 2) @ sd[p + "fn.net.3.weight"].t() + sd[p + "fn.net.3.bias"]).permute(0, 1, 4, 2, 3))
    assert not masks, "more masks than dropouts"
    m = R._ln(feat.mean(dim=1).permute(0, 2, 3, 1), sd["mlp_head.2.weight"], sd["mlp_head.2.bias"])
    return (m @ sd["mlp_head.3.weight"].t() + sd["mlp_head.3.bias"]).permute(0, 3, 1, 2).contiguous()


def cobevt_grads(sd, args, x, record_len, affine_matrix, g, dtype=torch.float64, masks=None):
    """(y, dx, {parameter name: gradient}) of the loss (y * g).sum(), everything computed in `dtype` on x's device."""
    dev = x.device
    leaf = {k: (v.detach().to(dev, dtype).requires_grad_(True) if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
    xl = x.detach().to(dtype).requires_grad_(True)
    y = cobevt_train_forward(leaf, args, xl, record_len, affine_matrix.to(dev), masks)
    names = param_names(sd)
    gs = torch.autograd.grad((y * g.to(dev, dtype)).sum(), [xl] + [leaf[k] for k in names])
    return y.detach(), gs[0], dict(zip(names, gs[1:]))


def rel_rms(a, b):
    """||a - b|| / ||b|| in float64 (b is the truth)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())
