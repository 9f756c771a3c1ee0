"""Helpers of the V2VNet training tests (tests/test_v2vnet_train.py, tests/test_gpu_v2vnet_train.py) and of
tools/make_golden_v2vnet_train.py: the training fixture's case table and loader, the messages of every (round, node) of the decomposed
forward with the margin between the winner and the runner-up of the max, and torch autograd of the restatement. Framework operators
only: nothing here touches the HIP library."""
import numpy as np
import torch
import torch.nn.functional as F

import v2vnet_restatement as R
from helpers import load_case

# `bt` replaces the forward fixture's max case `b` (whose smallest float64 margin between winner and runner-up, 1.1e-7, is the size of
# float32 rounding: one flipped winner would fail any tolerance without anything being wrong). Its weights, input and poses come from the
# first seed s in 0..31 that meets `margin_report`'s condition: synth.fill_params_(m, 100 + s), make_x(.., 200 + s), make_affine(.., 300 + s).
BT = dict(C=8, H=6, W=10, agg="max", gru=True, layers=2, iters=2, record_len=[3, 1, 4], L=5, kernel_size=[[3, 3], [1, 1]], off_map=(2, 3))
TRAIN_CASES = ("a", "bt", "c", "d")
MARGIN_FACTOR = 16.0     # margin >= 16 x the float32 run's message error: 8 x over the 2 x of that error the HIP path is allowed


def case_args(tag):
    if tag != "bt":
        return R.case_args(R.CASES[tag])
    a = R.case_args(BT)
    a["conv_gru"]["kernel_size"] = [list(k) for k in BT["kernel_size"]]
    return a


def bt_inputs(seed):
    from gencomm_amd import synth, V2VNetFusion
    m = V2VNetFusion(case_args("bt")).eval()
    synth.fill_params_(m, 100 + seed)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    n = sum(BT["record_len"])
    x = R.make_x(n, BT["C"], BT["H"], BT["W"], 200 + seed)
    aff = R.make_affine(BT["record_len"], BT["L"], BT["H"], BT["W"], 300 + seed, off_map=BT["off_map"])
    return sd, x, aff


_FIXTURES = {}


def _file(tag):
    return "v2vnet_train_d" if tag == "d" else "v2vnet_train"


def load_train_case(tag):
    """dict(args, sd, x float32, record_len, affine float64, grad_out float32, gx64, g64 {name: float64 gradient; absent = None in the
    reference}, ref {name or 'x': the reference float32 run's relative rms error against its float64 run}) of a fixture case."""
    name = _file(tag)
    if name not in _FIXTURES:
        _FIXTURES[name] = load_case(name)
    g = _FIXTURES[name]
    if tag == "bt":
        sd = {k.split("/", 1)[1]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w_bt/")}
        x, rl, aff = g["x_bt"], list(BT["record_len"]), g["affine_bt"]
    else:
        from test_v2vnet import load_v2vnet_case
        _, sd, x, rl, aff, *_ = load_v2vnet_case(tag)     # weights, input and poses are the forward fixture's: not duplicated
    g64 = {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(f"g64_{tag}/")}
    ref = {k.split("/", 1)[1]: float(v) for k, v in g.items() if k.startswith(f"ref_rel_rms_{tag}/")}
    return dict(args=case_args(tag), sd=sd, x=x, record_len=rl, affine=aff, grad_out=g[f"grad_out_{tag}"], gx64=g[f"gx64_{tag}"], g64=g64, ref=ref)


def reset_and_hidden_blocks(name, grad, C):
    """The blocks of a ConvGRU gradient that multiply the zero hidden state: (reset-gate rows, hidden-state columns) or None."""
    layer = int(name.split(".")[2])
    cin = 2 * C if layer == 0 else C
    if name.endswith("conv_gates.weight"):
        return [grad[:C], grad[:, cin:]]
    if name.endswith("conv_gates.bias"):
        return [grad[:C]]
    if name.endswith("conv_can.weight"):
        return [grad[:, cin:]]
    return []


def messages(sd, args, x, record_len, affine):
    """[(messages [n, C, H, W], masks [n, 1, H, W])] of every (round, node) of R.v2vnet_forward, in x's dtype (no autograd)."""
    dt = x.dtype
    p = {k: v.detach().to(dt) for k, v in sd.items()}
    C = args["in_channels"]
    out = []
    off = np.concatenate([[0], np.cumsum(record_len)]).tolist()
    cells = []
    for l in range(args["conv_gru"]["num_layers"]):
        cin = 2 * C if l == 0 else C
        pre = f"conv_gru.cell_list.{l}."
        cells.append((torch.cat([p[pre + "conv_gates.weight"][C:, :cin], p[pre + "conv_can.weight"][:, :cin]], 0),
                      torch.cat([p[pre + "conv_gates.bias"][C:], p[pre + "conv_can.bias"]], 0)))
    h = x
    with torch.no_grad():
        for it in range(args["num_iteration"]):
            last = it == args["num_iteration"] - 1
            new = []
            for b, n in enumerate(record_len):
                hb = h[off[b]:off[b + 1]]
                for i in range(1 if last else n):
                    th = affine[b, i, :n]
                    mask = R.warp(torch.ones(n, 1, *x.shape[2:], dtype=dt), th)
                    m = (F.conv2d(R.warp(hb, th), p["msg_cnn.weight"][:, :C], None, padding=1)
                         + F.conv2d(hb[i:i + 1], p["msg_cnn.weight"][:, C:], p["msg_cnn.bias"], padding=1)) * mask
                    out.append((m, mask))
                    agg = m.mean(0) if args["agg_operator"] == "avg" else m.max(0)[0]
                    if not args["gru_flag"]:
                        new.append(hb[i] + agg)
                        continue
                    s = torch.cat([hb[i], agg], 0)[None]
                    for w, bias in cells:
                        s = R.gate(F.conv2d(s, w, bias, padding=w.shape[-1] // 2))
                    new.append(s[0])
            h = torch.stack(new)
    return out


def winners(m):
    """torch.max's rule over dim 0, spelled out: a strictly greater value replaces the current one. -> (winner index, runner-up index)."""
    n = m.shape[0]
    best, win = m[0].clone(), torch.zeros(m.shape[1:], dtype=torch.int64)
    for j in range(1, n):
        up = m[j] > best
        best, win = torch.where(up, m[j], best), torch.where(up, torch.full_like(win, j), win)
    rest = m.clone()
    rest.scatter_(0, win[None], float("-inf"))
    return win, rest.argmax(0)


def margin_report(sd, args, x, record_len, affine):
    """The condition a max case must meet to be a training fixture. Over every position of every node with more than one pair where the
    winner's or the runner-up's mask is > 0: the smallest float64 margin between the two; against the largest |message32 - message64|.
    -> dict(live, margin, err, ratio, same_winners)."""
    x32 = torch.from_numpy(np.asarray(x, np.float32))
    aff = torch.from_numpy(np.asarray(affine))
    m64, m32 = messages(sd, args, x32.double(), record_len, aff), messages(sd, args, x32, record_len, aff)
    live, margin, err, same = 0, float("inf"), 0.0, True
    for (a, mask), (b, _) in zip(m64, m32):
        err = max(err, float((a - b.double()).abs().max()))
        if a.shape[0] < 2:
            continue
        win, run = winners(a)
        same = same and bool(torch.equal(win, winners(b)[0]))
        mk = mask.expand_as(a)
        on = (mk.gather(0, win[None])[0] > 0) | (mk.gather(0, run[None])[0] > 0)
        gap = (a.gather(0, win[None]) - a.gather(0, run[None]))[0]
        live += int(on.sum())
        if on.any():
            margin = min(margin, float(gap[on].min()))
    return dict(live=live, margin=margin, err=err, ratio=margin / max(err, 1e-300), same_winners=same)


def restatement_grads(sd, args, x, record_len, affine, grad_out, dtype):
    """torch autograd of R.v2vnet_forward in `dtype`: (output, d x, {name: gradient or None}) as numpy arrays."""
    p = {k: v.detach().to(dtype).requires_grad_() for k, v in sd.items()}
    xx = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_()
    # v2vnet_forward detaches what it reads: hand it tensors whose detach() keeps the graph
    live = {k: KeepGraph(v) for k, v in p.items()}
    out = R.v2vnet_forward(live, args, xx, record_len, torch.from_numpy(np.asarray(affine)))
    out.backward(torch.from_numpy(np.asarray(grad_out)).to(dtype))
    return out.detach().numpy(), xx.grad.numpy(), {k: (None if v.grad is None else v.grad.numpy()) for k, v in p.items()}


class KeepGraph:
    """Stands in for a state-dict entry: `.detach().to(dt)` (what the restatement calls) returns the graph-carrying tensor itself."""

    def __init__(self, t):
        self.t = t

    def detach(self):
        return self

    def to(self, dt):
        assert self.t.dtype == dt
        return self.t
