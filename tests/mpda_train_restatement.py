"""Plain-torch restatement of the TRAINABLE MPDA feature aligner, on tests/mpda_restatement.py (imported, not edited): the same
modules with externally supplied dropout masks, BatchNorm batch statistics in the resizer's residual blocks, and the gradient-reversal
layer of the classifier. Differentiable by torch autograd in float64 (truth) and float32 (yardstick). tests/test_mpda_train.py first
verifies it against the gradients the reference's own modules produced (tests/golden/mpda_train_*.npz, tools/make_golden_mpda_train.py);
the GPU tests then use it as truth for fresh inputs and for dropout.

Dropout masks arrive as a flat list in the order gencomm_amd/mpda_bwd.py documents, per SwapFusionEncoder call, per block, window then
grid: the attention's keep mask (bool [n, heads, X Y, 16], element 4 i + j, survivors scaled by 1 / (1 - p)), then the three
multiplicative masks (already scaled) after to_out, after the GELU and after the FeedForward's last Linear.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

import mpda_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 6100

# The golden cases: all at C = 32 on 4 x 6 maps. `kind` selects what runs; `mode` the module's mode; `cav_hw` / `cin` the resizer's input.
TRAIN_CASES = {
    "resizer_eval": dict(kind="resizer", mode="eval", cin=32, cav_hw=(4, 6), n_cav=3, drop_out=0.1),
    "resizer_train": dict(kind="resizer", mode="train", cin=32, cav_hw=(4, 6), n_cav=2, drop_out=0.0),     # BatchNorm over 2 x 4 x 6 = 48 values
    "resizer_resize": dict(kind="resizer", mode="eval", cin=48, cav_hw=(6, 10), n_cav=2, drop_out=0.1),
    "cdt": dict(kind="cdt", mode="eval", n_cav=3),
    "da": dict(kind="da", mode="eval", n_cav=3),
    "align": dict(kind="align", mode="eval", record_len=[1, 3, 2], rebuttal=False, drop_out=0.1),
    "rebuttal": dict(kind="align", mode="eval", record_len=[1, 3, 2], rebuttal=True, drop_out=0.1),
}
C, H, W, DIM_HEAD, HEADS, MLP_DIM = 32, 4, 6, 32, 2, 64


def case_args(tag):
    c = TRAIN_CASES[tag]
    return {"resizer": {"input_channel": c.get("cin", C), "output_channel": C,
                        "wg_att": {"input_dim": C, "mlp_dim": MLP_DIM, "window_size": 2, "dim_head": DIM_HEAD, "drop_out": c.get("drop_out", 0.1),
                                   "depth": 1},
                        "residual": {"input_dim": C, "depth": 2}},
            "cdt": {"input_dim": C, "window_size": 8, "dim_head": DIM_HEAD, "heads": HEADS, "depth": 1},
            "classifier": C, "rebuttal": c.get("rebuttal", False)}


def case_seed(tag):
    """The parameter seed of a case (BatchNorm statistics: seed + 50; inputs: seed + 10; the loss's functionals: seed + 20)."""
    return SEED + 100 * list(TRAIN_CASES).index(tag)


def case_inputs(tag):
    """float32 arrays: resizer (ego, cav), cdt (ego, cav), da (x,), align (x,)."""
    c = TRAIN_CASES[tag]
    rng = np.random.RandomState(case_seed(tag) + 10)
    draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    if c["kind"] == "resizer":
        return draw(1, C, H, W), draw(c["n_cav"], c["cin"], *c["cav_hw"])
    if c["kind"] == "cdt":
        return draw(1, C, H, W), draw(c["n_cav"], C, H, W)
    if c["kind"] == "da":
        return (draw(c["n_cav"], C, H, W),)
    return (draw(sum(c["record_len"]), C, H, W),)


def functional(tag, shape, which=0):
    """The seeded linear functional of a case's output: loss = sum(out * functional). float32 array."""
    return np.random.RandomState(case_seed(tag) + 20 + which).standard_normal(tuple(shape)).astype(np.float32)


def class_labels(record_len, H_, W_):
    """The shell's class labels (0 for an ego, 1 for a collaborator) per map, broadcast over the logits' pixels: [n, 1, H, W]."""
    lab = []
    for k in record_len:
        lab += [0.0] + [1.0] * (k - 1)
    return torch.tensor(lab).view(-1, 1, 1, 1).expand(-1, 1, H_, W_)


def align_loss(aligned, logits, g_aligned, record_len):
    """One aligner step's loss: a linear functional of `aligned` plus BCE-with-logits of the domain classifier (so the reversal layer
    is exercised)."""
    labels = class_labels(record_len, *logits.shape[2:]).to(logits.dtype).to(logits.device)
    return (aligned * g_aligned).sum() + F.binary_cross_entropy_with_logits(logits, labels)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def load_golden(tag):
    """The case's stored arrays; a case too large for one committed file has its d64 arrays in a second one."""
    rec = {}
    for name in (f"mpda_train_{tag}.npz", f"mpda_train_{tag}_f64.npz"):
        path = os.path.join(GOLDEN, name)
        if os.path.exists(path):
            z = np.load(path)
            rec.update({k: z[k] for k in z.files})
    return rec


def stored_names(rec):
    return sorted(k[4:] for k in rec if k.startswith("y32/"))


def stored(rec, name):
    """(y32, y64, e_ref) of a stored tensor: y64 = y32 - d64 in float64; e_ref is the float32 run's own relative rms error."""
    y32 = rec["y32/" + name]
    y64 = y32.astype(np.float64) - rec["d64/" + name].astype(np.float64)
    return y32, y64, R.rel_rms(y32, y64)


# ---------------------------------------------------------------------------------------------------------------- the modules
def leaf_sd(module, dtype):
    """state_dict as CPU tensors of `dtype`; the parameters are leaves that require grad (frozen ones do not), buffers are copies."""
    req = {k: p.requires_grad for k, p in module.named_parameters()}
    sd = {}
    for k, v in module.state_dict().items():
        t = v.detach().cpu()
        t = t.to(dtype).clone() if t.is_floating_point() else t.clone()
        sd[k] = t.requires_grad_(True) if req.get(k, False) else t
    return sd


class _Scale(torch.autograd.Function):
    """gradient_layer.py: the identity whose backward multiplies by `weight`."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.weight = weight
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.weight * g, None


def quad_attention(q, k, v, table, index, heads, dim_head, grid, keep=None, keep_scale=1.0):
    """R.quad_attention with dropout on the probabilities: keep bool [N, heads, G, 16] or None."""
    N, _, H_, W_ = q.shape
    if k.shape[0] != N:
        k, v = k.expand(N, -1, -1, -1), v.expand(N, -1, -1, -1)
    split = lambda t: R.to_groups(t, grid).reshape(N, -1, 4, heads, dim_head).permute(0, 3, 1, 2, 4)     # N heads G 4 d
    qg, kg, vg = split(q), split(k), split(v)
    sim = dim_head ** -0.5 * (qg @ kg.transpose(-1, -2))
    if table is not None:
        sim = sim + table[index].permute(2, 0, 1)[None, :, None]
    p = sim.softmax(dim=-1)
    if keep is not None:
        p = p * (keep.reshape(N, heads, -1, 4, 4).to(p.dtype) * keep_scale)
    out = p @ vg
    return R.from_groups(out.permute(0, 2, 3, 1, 4).reshape(N, -1, 4, heads * dim_head), grid, H_, W_)


def swap_encoder(sd, p, x, dim_head, depth=1, masks=None, drop_p=0.0):
    """R.swap_encoder with dropout: `masks` an iterator over the documented order (None: no dropout)."""
    heads, index, q_ = x.shape[1] // dim_head, R.rel_pos_indices(2), (p + ".") if p else ""
    take = (lambda: next(masks).to(x.dtype)) if masks is not None else (lambda: None)
    mul = lambda t, m: t if m is None else t * m
    for i in range(depth):
        for at, grid in ((1, False), (5, True)):
            a, f = f"{q_}layers.{i}.block.{at}", f"{q_}layers.{i}.block.{at + 1}"
            keep = next(masks) if masks is not None else None
            q, k, v = R._lin(R._ln(x, sd, a + ".norm"), sd, a + ".fn.to_qkv").chunk(3, dim=1)
            att = quad_attention(q, k, v, sd[a + ".fn.rel_pos_bias.weight"], index, heads, dim_head, grid, keep, 1.0 / (1.0 - drop_p))
            x = x + mul(R._lin(att, sd, a + ".fn.to_out.0"), take())
            mid = mul(F.gelu(R._lin(R._ln(x, sd, f + ".norm"), sd, f + ".fn.net.0")), take())
            x = x + mul(R._lin(mid, sd, f + ".fn.net.3"), take())
    return R._mlp_head(sd, q_, x)


def _bn(x, sd, p, batch_stats):
    if not batch_stats:
        return R._bn(x, sd, p)
    # nn.BatchNorm2d in train(): batch statistics; the running statistics (sd's buffers) are updated in place, momentum 0.1
    sd[p + ".num_batches_tracked"] += 1
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], True, 0.1, 1e-5)


def resizer(sd, p, ego, cav, dim_head, res_depth=2, batch_stats=False, masks=None, drop_p=0.0):
    """R.resizer with BatchNorm batch statistics (`batch_stats`) and dropout (`masks`: wg_att_1's masks first, then wg_att_2's)."""
    q = (p + ".") if p else ""
    size = ego.shape[2:]
    cav = F.conv2d(cav, sd[q + "channel_selector.weight"], sd[q + "channel_selector.bias"])
    one = R.resize(swap_encoder(sd, q + "wg_att_1", cav, dim_head, 1, masks, drop_p), size)
    two = one
    for i in range(res_depth):
        m = f"{q}res_blocks.{i}.module"
        h = F.leaky_relu(_bn(F.conv2d(two, sd[m + ".0.weight"], sd[m + ".0.bias"], padding=1), sd, m + ".1", batch_stats), 0.01)
        two = two + _bn(F.conv2d(h, sd[m + ".3.weight"], sd[m + ".3.bias"], padding=1), sd, m + ".4", batch_stats)
    two = swap_encoder(sd, q + "wg_att_2", two + one, dim_head, 1, masks, drop_p)
    return R.resize(cav, size) + two


def da_head(sd, p, x, reversal=-9.1):
    """DAImgHead with its gradient-reversal layer (`reversal` None: the layer removed)."""
    return R.da_head(sd, p, x if reversal is None else _Scale.apply(x, reversal))


def mpda_align(sd, args, x, record_len, batch_stats=False, masks=None, reversal=-9.1):
    """R.mpda_align, trainable: the ego-only scene contributes the ego alone (the reference's discarded branch has no gradient)."""
    dh_r, c = args["resizer"]["wg_att"]["dim_head"], args["cdt"]
    drop_p = args["resizer"]["wg_att"]["drop_out"]
    feats, off = [], 0
    for n in record_len:
        ego = x[off:off + 1]
        feats.append(ego)
        if n > 1:
            cav = x[off + 1:off + n]
            if not args.get("rebuttal", False):
                cav = R.cdt(sd, "cdt", ego, resizer(sd, "resizer", ego, cav, dh_r, args["resizer"]["residual"]["depth"], batch_stats, masks, drop_p),
                            c["heads"], c["dim_head"], c["depth"])
            feats.append(cav)
        off += n
    aligned = torch.cat(feats, dim=0)
    return aligned, da_head(sd, "classifier", aligned, reversal)


def grads_of(loss, sd, inputs):
    """({input name: gradient or None}, {parameter name: gradient}) of a scalar loss."""
    names = [k for k, v in sd.items() if v.requires_grad]
    ins = [k for k, v in inputs.items() if v.requires_grad]
    got = torch.autograd.grad(loss, [inputs[k] for k in ins] + [sd[k] for k in names], allow_unused=True)
    zero = lambda t, ref: torch.zeros_like(ref) if t is None else t
    gi = {k: zero(g, inputs[k]) for k, g in zip(ins, got[:len(ins)])}
    gp = {k: zero(g, sd[k]) for k, g in zip(names, got[len(ins):])}
    return gi, gp


def run_case(tag, module, dtype, inputs=None):
    """One golden case on the restatement with `module`'s state (the package's or the reference's: the same keys) -> dict of
    float64 / float32 numpy arrays under the fixture's names: out (or aligned, logits), d_<input>, g:<parameter>, rs:<buffer>."""
    c = TRAIN_CASES[tag]
    sd = leaf_sd(module, dtype)
    arrs = case_inputs(tag) if inputs is None else inputs
    t = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrs]
    rec = {}
    if c["kind"] == "resizer":
        out = resizer(sd, "", t[0], t[1], DIM_HEAD, 2, c["mode"] == "train")
        loss, ins = (out * torch.from_numpy(functional(tag, out.shape)).to(dtype)).sum(), {"cav": t[1]}
        rec["out"] = out
    elif c["kind"] == "cdt":
        out = R.cdt(sd, "", t[0], t[1], HEADS, DIM_HEAD)
        loss, ins = (out * torch.from_numpy(functional(tag, out.shape)).to(dtype)).sum(), {"ego": t[0], "cav": t[1]}
        rec["out"] = out
    elif c["kind"] == "da":
        out = da_head(sd, "", t[0])
        loss, ins = (out * torch.from_numpy(functional(tag, out.shape)).to(dtype)).sum(), {"x": t[0]}
        rec["out"] = out
    else:
        aligned, logits = mpda_align(sd, case_args(tag), t[0], c["record_len"])
        loss, ins = align_loss(aligned, logits, torch.from_numpy(functional(tag, aligned.shape)).to(dtype), c["record_len"]), {"x": t[0]}
        rec["aligned"], rec["logits"] = aligned, logits
    gi, gp = grads_of(loss, sd, ins)
    rec.update({"d_" + k: v for k, v in gi.items()})
    rec.update({"g:" + k: v for k, v in gp.items()})
    if c["mode"] == "train":
        rec.update({"rs:" + k: v for k, v in sd.items() if k.endswith(("running_mean", "running_var"))})
    return {k: v.detach().numpy() for k, v in rec.items()}


# ---------------------------------------------------------------------------------------------------------------- the resize adjoint
def resize_source(o, scale, n_in):
    """mpda_kernels.h resize_source in float32: (lower index, upper index, upper weight) of output index o."""
    f = np.float32
    src = max(f(f(scale) * f(f(o) + f(0.5))) - f(0.5), f(0.0))
    i0 = min(int(src), n_in - 1)
    i1 = min(i0 + 1, n_in - 1)
    l1 = min(max(f(src) - f(i0), f(0.0)), f(1.0))
    return i0, i1, f(l1)


def first_output(i, scale, n_in, n_out):
    """mpda_bwd_kernels.h resize_first_output: the first output index whose lower source index is >= i."""
    if i <= 0:
        return 0
    if i >= n_in:
        return n_out
    o = int(np.ceil(np.float32((np.float32(i) + np.float32(0.5)) / np.float32(scale) - np.float32(0.5))))
    o = max(0, min(o, n_out))
    while o > 0 and resize_source(o - 1, scale, n_in)[0] >= i:
        o -= 1
    while o < n_out and resize_source(o, scale, n_in)[0] < i:
        o += 1
    return o


def resize_adjoint_matrix(n_in, n_out):
    """[n_in, n_out] float64: the gather of the kernel along one axis -- row i holds, for the outputs of its contiguous range
    [lo(i - 1), lo(i + 1)), the weight resize_weight() gives (float32 values); every other entry is 0."""
    scale = np.float32(n_in) / np.float32(n_out)
    A = np.zeros((n_in, n_out))
    for i in range(n_in):
        for o in range(first_output(i - 1, scale, n_in, n_out), first_output(i + 1, scale, n_in, n_out)):
            i0, i1, l1 = resize_source(o, scale, n_in)
            w = np.float32(0.0)
            if i0 == i:
                w = np.float32(1.0) - l1
            if i1 == i and l1 != 0:
                w = np.float32(w + l1)
            A[i, o] = float(w)
    return A
