"""STAMP's adapter / reverter (opencood/models/stamp_modules/adapter.py: AdapterConvNext, AdapterConv, AdapterIdentity; the ConvNeXtBlock of
stamp_modules/feature_alignnet_modules.py:303-348) restated in plain torch, in any dtype, from a state_dict with the reference's keys.
Used by the CPU tests against tests/golden/stamp_adapter.npz (written by tools/make_golden_stamp_adapter.py from the reference's own
modules), by the GPU tests as the float64 reference of the shapes the fixture does not hold, and as the torch baseline of
tools/stamp_adapter_bench.py.

The fixture stores generator seeds, not parameters or inputs: ``make_params`` / ``make_x`` regenerate them bit for bit from numpy's PCG64
streams, and the fixture carries a float64 checksum of each.

Parameter scale. The reference initialises ``gamma = 1e-6``, under which a block is invisible next to its residual and a test of it
tests nothing. EVERY parameter here is drawn from a normal distribution, gamma included (``STD``); LayerNorm's weight is centred on 1 so
that the normalised pixel keeps a channel variance of order 1 into pwconv1. ``branch_share`` measures what a block adds.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

RANGE = [-102.4, -51.2, -3, 102.4, 51.2, 1]
STD = 0.2                      # every weight, bias and gamma: normal(0, std); norm.weight: normal(1, std)
STD_WIDE = 0.15                # in 256 / dim 128: the closing 1x1 convolution sums 128 products of |h| ~ 5 and |w| ~ STD, and the rounding of that
                               # sum alone (6e-8 relative per product) put the reference's OWN float32 run at 0.95 of the tolerance with STD;
                               # at 0.15 it sits at 0.3, which leaves a second float32 summation order room to differ
STD_CHAIN = 0.1                # the reverter of the adapter -> reverter chain: it is fed the adapter's output (standard deviation 5, not 1), and
                               # with STD the restatement's OWN float32 chain is 1.5 x the tolerance away from its float64 chain; at 0.1 it is 0.43
MIN_BRANCH_SHARE = 0.1         # median |block(x) - x| must exceed this share of median |block(x)| for every block of the fixture


def base_args(cin, cout=None, sub=None, in_range=None, out_range=None, in_shape=(128, 256), out_shape=(128, 256)):
    args = dict(in_channels=cin, out_channels=cin if cout is None else cout, in_cav_lidar_range=list(in_range or RANGE),
                out_cav_lidar_range=list(out_range or RANGE), in_feature_shape=list(in_shape), out_feature_shape=list(out_shape))
    if sub is not None:
        args["submodule_args"] = dict(sub)
    return args


def shipped(cin, dim, **sub):
    """The constructor dict of the shipped yamls (in == out channels, 128 x 256 maps, 3 blocks)."""
    return {"core_method": "adapterconvnext", "args": base_args(cin, sub=dict(num_of_blocks=3, dim=dim, **sub))}


# The fixture's cases: (class, constructor dict, input shape, parameter std).  conv: in range 16 x 8 m on a 8 x 16 map, out range 20 x 12 m on a 12 x 20 map --
# feature ratio 1, two cells of padding on every side.
CASES = {
    "cnx64": ("Adapter", shipped(128, 64), (2, 128, 12, 20), STD),
    "cnx128": ("Adapter", shipped(256, 128, early_scale=0.5), (1, 256, 9, 11), STD_WIDE),
    "rev64": ("Reverter", shipped(128, 64), (1, 128, 12, 20), STD),
    "identity": ("Adapter", {"core_method": "identity", "args": base_args(128)}, (1, 128, 3, 5), STD),
    "conv": ("Adapter", {"core_method": "adapterconv",
                         "args": base_args(128, 32, in_range=[-8, -4, -3, 8, 4, 1], out_range=[-10, -6, -3, 10, 6, 1], in_shape=(8, 16), out_shape=(12, 20))},
             (1, 128, 8, 16), STD),
}
SHIPPED = {"in128_dim64": shipped(128, 64), "in256_dim128": shipped(256, 128)}


def block_shapes(dim):
    return {"gamma": (dim,), "dwconv.weight": (dim, 1, 7, 7), "dwconv.bias": (dim,), "norm.weight": (dim,), "norm.bias": (dim,),
            "pwconv1.weight": (4 * dim, dim), "pwconv1.bias": (4 * dim,), "pwconv2.weight": (dim, 4 * dim), "pwconv2.bias": (dim,)}


def param_shapes(cfg, prefix):
    """{key: shape} in the reference's state_dict order."""
    a, out = cfg["args"], {}
    if cfg["core_method"] == "adapterconvnext":
        sub = a["submodule_args"]
        dim = sub.get("dim", 64)
        out[f"{prefix}.channel_convert1.weight"] = (dim, a["in_channels"], 1, 1)
        out[f"{prefix}.channel_convert1.bias"] = (dim,)
        for i in range(sub["num_of_blocks"]):
            for k, s in block_shapes(dim).items():
                out[f"{prefix}.conv.model.{i}.{k}"] = s
        out[f"{prefix}.channel_convert2.weight"] = (a["out_channels"], dim, 1, 1)
        out[f"{prefix}.channel_convert2.bias"] = (a["out_channels"],)
        out[f"{prefix}.smoothing.weight"] = (a["out_channels"], a["out_channels"], 3, 3)
        out[f"{prefix}.smoothing.bias"] = (a["out_channels"],)
    elif cfg["core_method"] == "adapterconv":
        out[f"{prefix}.conv.weight"] = (a["out_channels"], a["in_channels"], 1, 1)
        out[f"{prefix}.conv.bias"] = (a["out_channels"],)
    return out


def make_params(cfg, prefix, seed, std=STD):
    """A float32 state_dict with the reference's keys: normal(0, std) everywhere, normal(1, std) for LayerNorm's weight."""
    rng = np.random.default_rng(seed)
    return {k: torch.from_numpy(rng.normal(1.0 if k.endswith("norm.weight") else 0.0, std, s).astype(np.float32))
            for k, s in param_shapes(cfg, prefix).items()}


def make_block_params(dim, seed, std=STD):
    rng = np.random.default_rng(seed)
    return {k: torch.from_numpy(rng.normal(1.0 if k == "norm.weight" else 0.0, std, s).astype(np.float32)) for k, s in block_shapes(dim).items()}


def make_x(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(0.0, 1.0, shape).astype(np.float32))


def checksum(tensors):
    return float(sum(t.double().sum() + (t.double() ** 2).sum() for t in tensors))


def convnext_block(p, x, dtype=None):
    """feature_alignnet_modules.py:332-348 from {gamma, dwconv.weight, ...}; gamma may be None."""
    dtype = dtype or x.dtype
    p = {k: (None if v is None else v.to(dtype)) for k, v in p.items()}
    x = x.to(dtype)
    dim = x.shape[1]
    h = F.conv2d(x, p["dwconv.weight"], p["dwconv.bias"], padding=3, groups=dim).permute(0, 2, 3, 1)
    h = F.layer_norm(h, (dim,), p["norm.weight"], p["norm.bias"], 1e-6)
    h = F.linear(F.gelu(F.linear(h, p["pwconv1.weight"], p["pwconv1.bias"])), p["pwconv2.weight"], p["pwconv2.bias"])
    if p.get("gamma") is not None:
        h = p["gamma"] * h
    return x + h.permute(0, 3, 1, 2)


def pad_of(a):
    """BaseAdapter's arithmetic (adapter.py:62-92): (feat_ratio, (left, right, top, bottom))."""
    ir, orr = a["in_cav_lidar_range"], a["out_cav_lidar_range"]
    in_lidar, out_lidar = np.array([ir[3] - ir[0], ir[4] - ir[1]]), np.array([orr[3] - orr[0], orr[4] - orr[1]])
    in_ratio = np.array([a["in_feature_shape"][1], a["in_feature_shape"][0]]) / in_lidar
    out_ratio = np.array([a["out_feature_shape"][1], a["out_feature_shape"][0]]) / out_lidar
    fr = out_ratio / in_ratio
    left = ir[0] * in_ratio[0] * fr[0] - orr[0] * out_ratio[0]
    right = orr[3] * out_ratio[0] - ir[3] * in_ratio[0] * fr[0]
    top = ir[1] * in_ratio[1] * fr[1] - orr[1] * out_ratio[1]
    bottom = orr[4] * out_ratio[1] - ir[4] * in_ratio[1] * fr[1]
    return fr, (round(left), round(right), round(top), round(bottom))


def block_params(sd, prefix, i):
    pre = f"{prefix}.conv.model.{i}."
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def adapter_forward(cfg, sd, prefix, x, dtype=None, trace=None):
    """Adapter(cfg) / Reverter(cfg) .forward at feature ratio (1, 1); `trace` (a list) receives (input, output) of every block."""
    dtype = dtype or x.dtype
    a, x = cfg["args"], x.to(dtype)
    fr, pad = pad_of(a)
    assert fr[0] == 1.0 and fr[1] == 1.0, "the restatement covers feature ratio (1, 1): nn.Upsample is then the identity"
    if cfg["core_method"] == "identity":
        return x
    sd = {k: v.to(dtype) for k, v in sd.items()}
    if cfg["core_method"] == "adapterconv":
        return F.pad(F.conv2d(x, sd[f"{prefix}.conv.weight"], sd[f"{prefix}.conv.bias"]), pad)
    assert cfg["core_method"] == "adapterconvnext"
    sub = a["submodule_args"]
    h = F.conv2d(x * sub.get("early_scale", 1.0), sd[f"{prefix}.channel_convert1.weight"], sd[f"{prefix}.channel_convert1.bias"])
    for i in range(sub["num_of_blocks"]):
        y = convnext_block(block_params(sd, prefix, i), h)
        if trace is not None:
            trace.append((h, y))
        h = y
    return F.conv2d(h, sd[f"{prefix}.channel_convert2.weight"], sd[f"{prefix}.channel_convert2.bias"])


def branch_share(x, y):
    """median |y - x| / median |y| of one block."""
    return float((y - x).abs().median() / y.abs().median())


def prefix_of(cls):
    return {"Adapter": "adapter", "Reverter": "reverter"}[cls]


def case_data(name, seed):
    cls, cfg, shape, std = CASES[name]
    return cls, cfg, make_params(cfg, prefix_of(cls), seed, std), make_x(shape, seed + 1)


def chain_data(seed_adapter, seed_reverter):
    """Adapter -> Reverter once: (adapter cfg, its params, reverter cfg, its params (STD_CHAIN), x)."""
    _, cfg_a, sd_a, x = case_data("cnx64", seed_adapter)
    _, cfg_r, _, _ = CASES["rev64"]
    return cfg_a, sd_a, cfg_r, make_params(cfg_r, "reverter", seed_reverter, STD_CHAIN), x


def chain_forward(cfg_a, sd_a, cfg_r, sd_r, x, dtype):
    return adapter_forward(cfg_r, sd_r, "reverter", adapter_forward(cfg_a, sd_a, "adapter", x, dtype), dtype)


def within(got, ref64):
    """The project's tolerance, elementwise: (ok, worst |got - ref| / (1e-5 + 1e-4 |ref|))."""
    ratio = (got.double() - ref64).abs() / (1e-5 + 1e-4 * ref64.abs())
    return bool((ratio <= 1.0).all()), float(ratio.max())
