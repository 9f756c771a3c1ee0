"""Plain-torch restatement of the HEAL and MPDA training criteria (``opencood/loss/point_pillar_pyramid_loss.py``,
``opencood/loss/point_pillar_mpda_loss.py``) in the dtype of its inputs, and the cases of tests/golden/baseline_criteria.npz
(tools/make_golden_baseline_criteria.py runs the reference's own modules on these inputs; tests/test_baseline_criteria.py holds this
restatement to the stored float64 values at 1e-10).

The occupancy labels are written with reshapes and any / all over the windows instead of the reference's max_pool2d: the windows of a
floor-pooled map are the k x k blocks of its top-left (H // k * k) x (W // k * k) corner. The detection-head terms are the
framework-operator composition the package keeps for CPU tensors (``PointPillarDepthLoss`` with ``fuse_heads = False``)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_criteria.npz")

HEAD_ARGS = {  # the loss block the HEAL / MPDA yamls share with every PointPillar baseline
    "pos_cls_weight": 2.0, "cls": {"type": "SigmoidFocalLoss", "alpha": 0.25, "gamma": 2.0, "weight": 2.0},
    "reg": {"type": "WeightedSmoothL1Loss", "sigma": 3.0, "codewise": True, "weight": 2.0},
    "dir": {"type": "WeightedSoftmaxClassificationLoss", "weight": 0.2, "args": {"dir_offset": 0.7853, "num_bins": 2, "anchor_yaw": [0, 90]}},
    "depth": {"weight": 1.0}}


def pyramid_args(levels, weights, gamma=2.0):
    a = json.loads(json.dumps(HEAD_ARGS))
    a["cls"]["gamma"] = gamma
    a["pyramid"] = {"relative_downsample": list(levels), "weight": list(weights)}
    return a


MPDA_ARGS = dict(json.loads(json.dumps(HEAD_ARGS)), da=True)

# name: (seed, B, H, W, levels, weights, gamma)
OCC_CASES = {
    "occ_even": (7101, 3, 12, 20, [1, 2, 4], [0.4, 0.2, 0.1], 2.0),
    "occ_floor": (7102, 2, 10, 14, [1, 2, 4], [0.4, 0.2, 0.1], 2.0),
    "occ_k3": (7103, 2, 10, 16, [1, 3], [0.4, 0.2], 1.5),
    "occ_wide": (7104, 2, 40, 72, [1, 2, 4], [0.4, 0.2, 0.1], 2.0),
}
# name: (seed, record_len, da_feature shape, validate)
MPDA_CASES = {
    "mpda": (7201, [2, 3], (5, 1, 6, 10), False),
    "mpda_val": (7201, [2, 3], (5, 1, 6, 10), True),
    "mpda_b": (7202, [1, 2], (3, 2, 7, 9), False),
}
PYR_SEED = 7301   # pyr_single / pyr_collab: B = 2 head maps of 12 x 20, levels [1, 2, 4], one depth_items entry [2, 6, 5, 8]


def occ_inputs(name):
    """pos / neg_equal_one [B, H, W, 2] and one logit map per level (normal: none is exactly 0, where the focal term has a kink)."""
    seed, B, H, W, levels, _, _ = OCC_CASES[name]
    r = np.random.RandomState(seed)
    u = r.rand(B, H, W, 2)
    pos = (u < 0.02).astype(np.float32)
    neg = (u > 0.05).astype(np.float32)
    if name == "occ_even":
        pos[1] = 0                                   # a sample without any positive: clamp(min = 1)
        pos[2] = 0
        pos[2, 5, 7, 1] = 1                          # a sample whose only positive sits on anchor 1
        neg[2, 5, 7] = 0
        pos[0, 3, 4] = 0
        neg[0, 3, 4] = (1, 0)                        # negative on anchor 0 only: negative at no level
    if name == "occ_floor":
        pos[:] = 0                                   # positives only in the rows and columns the 4-level drops
        pos[0, 8, 12, 0] = pos[0, 9, 13, 1] = pos[1, 9, 12, 0] = 1
        neg[pos > 0] = 0
    out = {"pos_equal_one": pos, "neg_equal_one": neg}
    for i, k in enumerate(levels):
        out[f"occ{i}"] = r.normal(-1.0, 1.5, (B, 1, H // k, W // k)).astype(np.float32)
    assert all((out[f"occ{i}"] != 0).all() for i in range(len(levels)))
    return out


def head_inputs(seed, B, H, W):
    from gencomm_amd import synth
    inp = synth.make_loss_inputs(seed, B, H, W, 2, 4, pos_frac=0.04)
    return {("psm", "rm", "dm")[("cls_preds", "reg_preds", "dir_preds").index(k)] if k.endswith("_preds") else k: v
            for k, v in inp.items() if k not in ("gt_feature", "pred_feature")}


def mpda_inputs(name):
    seed, rl, shape, _ = MPDA_CASES[name]
    out = head_inputs(seed, len(rl), 6, 10)
    out["da_feature"] = np.random.RandomState(seed + 1).normal(0.2, 1.2, shape).astype(np.float32)
    assert (out["da_feature"] != 0).all()
    return out


def pyr_inputs():
    out = head_inputs(PYR_SEED, 2, 12, 20)
    r = np.random.RandomState(PYR_SEED + 1)
    for i, k in enumerate((1, 2, 4)):
        out[f"occ{i}"] = r.normal(-1.0, 1.5, (2, 1, 12 // k, 20 // k)).astype(np.float32)
    out["depth_logit"] = r.normal(0, 1, (2, 6, 5, 8)).astype(np.float32)
    out["depth_gt"] = r.randint(0, 6, (2, 5, 8)).astype(np.int64)
    return out


LOGITS = ("psm", "rm", "dm", "occ0", "occ1", "occ2", "depth_logit", "da_feature")   # every input that carries a gradient


# ----------------------------------------------------------------------------------------------------------------- the arithmetic
def occ_level_labels(pos, neg, k):
    """(pos_l, neg_l) [B, H // k, W // k], float32 whatever the dtype of pos: the reference's `.float()` (:71-72)."""
    B, H, W, _ = pos.shape
    Hl, Wl = H // k, W // k
    win = lambda m: m[:, :Hl * k, :Wl * k].reshape(B, Hl, k, Wl, k)
    occ_pos = (pos[..., 0] != 0) | (pos[..., 1] != 0)
    occ_neg = (neg[..., 0] != 0) & (neg[..., 1] != 0)
    return win(occ_pos).any(4).any(2).float(), win(occ_neg).all(4).all(2).float()


def focal(x, t, w, gamma, alpha):
    t = t.type_as(x)
    ce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    p = torch.sigmoid(x)
    p_t = t * p + (1 - t) * (1 - p)
    return (1.0 - p_t) ** gamma * (t * alpha + (1 - t) * (1 - alpha)) * ce * w


def occ_loss(occ_list, pos, neg, levels, weights, pos_cls_weight, gamma, alpha):
    """(total, [level losses]). As in the reference the labels and the cell weights -- the division by the normaliser included -- are
    float32 whatever the logits' dtype: its float64 run, the fixture's truth, carries that one float32 rounding per cell weight."""
    B = pos.shape[0]
    out = []
    for occ, k, wt in zip(occ_list, levels, weights):
        pos_l, neg_l = occ_level_labels(pos, neg, k)
        norm = pos_l.flatten(1).sum(1).clamp(min=1.0).view(B, 1, 1)
        w = (pos_l * pos_cls_weight + neg_l * 1.0) / norm
        out.append(focal(occ[:, 0], pos_l, w, gamma, alpha).sum() / B * wt)
    return sum(out), out


def domain_targets(x, record_len):
    t = torch.zeros_like(x, dtype=torch.float32)   # float32 whatever the logits' dtype (:135-136)
    s = 0
    for n in record_len:
        t[s] = 1
        s += int(n)
    return t


def domain_bce(x, record_len):
    """The reference's call (:143). With float64 logits torch returns a float32 VALUE for float32 targets (and an exact float64
    gradient): the fixture's "float64" da_loss is float32-precise, which domain_bce_stable, the form the kernel uses, is not."""
    return F.binary_cross_entropy_with_logits(x, domain_targets(x, record_len))


def domain_bce_stable(x, record_len):
    t = domain_targets(x, record_len).type_as(x)
    return (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()


def _head_criterion(args):
    from gencomm_amd.point_pillar_depth_loss import PointPillarDepthLoss
    crit = PointPillarDepthLoss({k: v for k, v in args.items() if k not in ("pyramid", "da")})
    crit.fuse_heads = False
    return crit


def pyramid_loss(args, output_dict, target_dict, suffix=""):
    """(total, loss_dict) of PointPillarPyramidLoss.forward."""
    crit = _head_criterion(args)
    occ = lambda: occ_loss(output_dict["occ_single_list"], target_dict["pos_equal_one"], target_dict["neg_equal_one"],
                           args["pyramid"]["relative_downsample"], args["pyramid"]["weight"], args["pos_cls_weight"], args["cls"]["gamma"],
                           args["cls"]["alpha"])[0]
    if output_dict["pyramid"] == "collab" and suffix == "_single":
        o = occ()
        return o, {"pyramid_loss": o.detach(), "total_loss": o.detach()}
    total = crit(output_dict, target_dict, suffix if output_dict["pyramid"] == "single" else "")
    d = dict(crit.loss_dict)
    if output_dict["pyramid"] == "single":
        o = occ()
        total = total + o
        d.update({"pyramid_loss": o.detach(), "total_loss": total.detach()})
    return total, d


def mpda_loss(args, output_dict, target_dict, validate=False):
    """(total, loss_dict) of PointPillarMPDALoss.forward."""
    crit = _head_criterion(args)
    total = crit({k: v for k, v in output_dict.items() if k not in ("record_len", "da_feature")}, target_dict)
    d = {k: v for k, v in crit.loss_dict.items() if k != "total_loss"}
    da = torch.zeros((), dtype=total.dtype)
    if args.get("da") and not validate:
        da = domain_bce(output_dict["da_feature"], output_dict["record_len"])
        total = total + da + da
    d.update({"total_loss": total.detach(), "da_loss": da.detach()})
    return total, d


# ------------------------------------------------------------------------------------------------------------ cases as dictionaries
def tensors(inp, dtype, device="cpu", grad=True):
    out = {}
    for k, v in inp.items():
        t = torch.from_numpy(np.asarray(v))
        t = (t if t.dtype == torch.int64 else t.to(dtype)).to(device)
        out[k] = t.requires_grad_(True) if grad and k in LOGITS else t
    return out


def dicts(kind, t, record_len=None):
    """(output_dict, target_dict) of a case from its tensors; kind: 'occ' (collab, "_single"), 'single', 'collab', 'mpda'."""
    tgt = {k: t[k] for k in ("pos_equal_one", "neg_equal_one", "targets") if k in t}
    out = {k: t[k] for k in ("psm", "rm", "dm") if k in t}
    if kind in ("occ", "single"):
        out["occ_single_list"] = [t[f"occ{i}"] for i in range(4) if f"occ{i}" in t]
    if kind in ("single", "collab"):
        out["depth_items"] = [t["depth_logit"], t["depth_gt"]]
    if kind == "mpda":
        out.update(da_feature=t["da_feature"], record_len=torch.tensor(record_len))
    if kind != "mpda":
        out["pyramid"] = "single" if kind == "single" else "collab"
    return out, tgt


def all_cases():
    """name -> (kind, args, inputs, extra): every case of the fixture."""
    cases = {}
    for name, (_, _, _, _, levels, weights, gamma) in OCC_CASES.items():
        cases[name] = ("occ", pyramid_args(levels, weights, gamma), occ_inputs(name), {})
    cases["pyr_single"] = ("single", pyramid_args([1, 2, 4], [0.4, 0.2, 0.1]), pyr_inputs(), {})
    cases["pyr_collab"] = ("collab", pyramid_args([1, 2, 4], [0.4, 0.2, 0.1]), {k: v for k, v in pyr_inputs().items() if not k.startswith("occ")}, {})
    for name, (_, rl, _, validate) in MPDA_CASES.items():
        cases[name] = ("mpda", MPDA_ARGS, mpda_inputs(name), {"record_len": rl, "validate": validate})
    return cases


def run_restatement(kind, args, t, extra):
    out, tgt = dicts(kind, t, extra.get("record_len"))
    if kind == "mpda":
        return mpda_loss(args, out, tgt, extra["validate"])
    return pyramid_loss(args, out, tgt, "_single" if kind == "occ" else "")


def rel(a, b):
    """|a - b| / |b| of two scalars (absolute where b is 0)."""
    a, b = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (a, b))
    return abs(a - b) / abs(b) if b != 0 else abs(a - b)


def rms_rel(a, b):
    """rms(a - b) / rms(b) of two arrays (rms(a) where b is all zero)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.sqrt((b ** 2).mean())
    return float(np.sqrt(((a - b) ** 2).mean()) / den) if den > 0 else float(np.sqrt((a ** 2).mean()))
