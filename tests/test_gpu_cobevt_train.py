"""Training of the CoBEVT fusion on the GPU: gencomm_swap_attn_train_fwd / gencomm_swap_attn_bwd called directly through the C ABI
against float64 autograd of the restated attention on the CPU, then ``CoBEVT(args, trainable=True)`` against the reference's stored
float64 gradients (tests/golden/cobevt_train*.npz), fresh shapes, dropout with replayed masks, the stage-2 pattern (frozen parameters),
determinism, and one training step of the stage-1 shell.

Criterion (as test_gpu_v2vnet_train.py): truth = float64 on the CPU, yardstick = the same computation in float32 (for the fixture cases:
the reference's own float32 run, stored); the HIP result's relative rms error against the truth <= max(2 x the yardstick's, 1e-6).
Gradient buffers are pre-filled with NaN where the kernel must overwrite them, so an element left unwritten fails the test."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import cobevt_restatement as R
import cobevt_train_restatement as TR
from helpers import GOLDEN, load_case
from gencomm_amd import CoBEVT, _lib, synth
from gencomm_amd.runtime import ptr, stream_ptr
from test_cobevt_train import FULL, load_golden, restated_grads, stored

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, truth):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    truth = truth.detach().cpu().numpy() if torch.is_tensor(truth) else truth
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.linalg.norm(a - truth) / np.linalg.norm(truth))


def check(what, got, truth, yard):
    """`yard`: the yardstick's own relative rms error (a number), or the float32 result it is computed from."""
    assert np.isfinite(got.detach().cpu().numpy() if torch.is_tensor(got) else got).all(), f"{what}: not finite"
    e = rel(got, truth)
    y = float(yard) if np.ndim(yard) == 0 and not torch.is_tensor(yard) else rel(yard, truth)
    print(f"{what}: relative rms against float64: HIP {e:.3e}, float32 yardstick {y:.3e}")
    assert e <= max(2.0 * y, 1e-6), (what, e, y)
    return e, y


def poison():
    junk = torch.full((8 << 20,), float("nan"), device=DEV)   # NaNs in the memory the allocator hands out next
    del junk


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
def _attention_truth(qkv, table, dout, nvalid, L, ws, heads, grid, dtype):
    """(out, lse [B L, heads, H, W], dqkv, dtable) of R.swap_attention by torch autograd on the CPU in `dtype`."""
    n, c3, H, W = qkv.shape
    B, dh = n // L, c3 // 3 // heads
    q = qkv.to(dtype).view(B, L, c3, H, W).requires_grad_(True)
    t = table.to(dtype).requires_grad_(True)
    index = R.relative_position_index(L, ws)
    out = R.swap_attention(q, t, index, nvalid, L, ws, heads, bool(grid))
    dq, dt = torch.autograd.grad((out * dout.to(dtype).view_as(out)).sum(), [q, t])
    with torch.no_grad():   # the log-sum-exp of the same scores
        g = R.to_groups(q, ws, bool(grid))
        inner = c3 // 3
        qq, kk = (g[:, :, i * inner:(i + 1) * inner].reshape(g.shape[0], -1, heads, dh).permute(0, 2, 1, 3) for i in range(2))
        sim = torch.matmul(qq * dh ** -0.5, kk.transpose(-1, -2)) + t[index].permute(2, 0, 1)[None]
        per_scene = (H // ws) * (W // ws)
        valid = (torch.arange(L * ws * ws) // (ws * ws))[None, :] < torch.as_tensor(nvalid).repeat_interleave(per_scene)[:, None]
        lse = torch.logsumexp(sim.masked_fill(~valid[:, None, None, :], -float("inf")), dim=-1)      # [G, heads, T]
        lse = R.from_groups(lse.permute(0, 2, 1), (B, L, heads, H, W), ws, bool(grid)).reshape(n, heads, H, W)
    return out.detach().reshape(n, -1, H, W), lse, dq.reshape(n, c3, H, W), dt


@pytest.mark.parametrize("ws,dh", [(4, 16), (4, 32), (4, 64), (8, 16), (8, 32), (8, 64)])
def test_swap_attention_backward_kernel_vs_float64(ws, dh):
    """B 2, H = W = 2 ws (four groups per scene: window and grid partitions differ), two heads, L in {1, 3, 5, 8} with the agent counts
    [L, 1] and [max(1, L - 2), L], both partitions. Token counts 16 .. 128 at ws 4 (48 and 80 are no multiple of 32; partial 64-key
    tiles; a single valid agent of 16 keys) and 64 .. 512 at ws 8 (320 and 512 are split over workgroups)."""
    heads, B, H, W = 2, 2, 2 * ws, 2 * ws
    inner = heads * dh
    rng = np.random.RandomState(1000 * ws + dh)
    l = _lib.lib()
    for L in (1, 3, 5, 8):
        qkv = rng.standard_normal((B * L, 3 * inner, H, W)).astype(np.float32)
        qkv[:, :inner] *= 1.5                                   # scores of a few units: a softmax that is far from uniform
        table = rng.uniform(-1.0, 1.0, ((2 * L - 1) * (2 * ws - 1) ** 2, heads)).astype(np.float32)
        dout = rng.standard_normal((B * L, inner, H, W)).astype(np.float32)
        qkv, table, dout = torch.from_numpy(qkv), torch.from_numpy(table), torch.from_numpy(dout)
        q_dev, t_dev, d_dev = qkv.to(DEV), table.to(DEV), dout.to(DEV)
        for nvalid in sorted({(L, 1), (max(1, L - 2), L)}):
            nv = torch.tensor(nvalid, dtype=torch.int32, device=DEV)
            for grid in (0, 1):
                what = f"swap attention backward ws {ws} dh {dh} L {L} agents {list(nvalid)} grid {grid}"
                dims = (B, L, heads, dh, ws, H, W, grid, stream_ptr(q_dev.device))
                out0 = torch.full((B * L, inner, H, W), float("nan"), device=DEV)
                out, lse = torch.full_like(out0, float("nan")), torch.full((B * L, heads, H, W), float("nan"), device=DEV)
                _lib.check(l.gencomm_swap_attn_fwd(ptr(q_dev), ptr(t_dev), ptr(nv), ptr(out0), *dims), "gencomm_swap_attn_fwd")
                _lib.check(l.gencomm_swap_attn_train_fwd(ptr(q_dev), ptr(t_dev), ptr(nv), ptr(out), ptr(lse), *dims), "gencomm_swap_attn_train_fwd")
                dqkv, dtable = torch.full_like(q_dev, float("nan")), torch.zeros_like(t_dev)
                _lib.check(l.gencomm_swap_attn_bwd(ptr(q_dev), ptr(t_dev), ptr(nv), ptr(out), ptr(lse), ptr(d_dev), ptr(dqkv), ptr(dtable), *dims),
                           "gencomm_swap_attn_bwd")
                torch.cuda.synchronize()
                assert torch.isfinite(out0).all() and torch.equal(out, out0), what          # the inference entry's bits
                _, lse64, dq64, dt64 = _attention_truth(qkv, table, dout, list(nvalid), L, ws, heads, grid, torch.float64)
                _, _, dq32, dt32 = _attention_truth(qkv, table, dout, list(nvalid), L, ws, heads, grid, torch.float32)
                assert torch.isfinite(lse).all() and float((lse.cpu().double() - lse64).abs().max()) <= 1e-5, what
                assert torch.isfinite(dqkv).all(), f"{what}: elements of dqkv left unwritten"
                got = dqkv.cpu()
                for i, part in enumerate(("dq", "dk", "dv")):
                    sl = slice(i * inner, (i + 1) * inner)
                    check(f"{what} {part}", got[:, sl], dq64[:, sl], dq32[:, sl])
                check(f"{what} dtable", dtable, dt64, dt32)
                for b, k in enumerate(nvalid):                  # keys and values of masked agents: exact zeros
                    assert not got[b * L + k:(b + 1) * L, inner:].any(), what


def test_table_gradient_is_accumulated():
    """dtable is added to: a second call on the same buffer doubles it (to rounding), and what it held before is kept."""
    ws, dh, heads, L, B, H, W = 4, 16, 1, 2, 1, 8, 8
    rng = np.random.RandomState(3)
    q = torch.from_numpy(rng.standard_normal((B * L, 3 * dh, H, W)).astype(np.float32)).to(DEV)
    t = torch.from_numpy(rng.uniform(-1, 1, ((2 * L - 1) * 49, heads)).astype(np.float32)).to(DEV)
    d = torch.from_numpy(rng.standard_normal((B * L, dh, H, W)).astype(np.float32)).to(DEV)
    nv = torch.tensor([2], dtype=torch.int32, device=DEV)
    dims = (B, L, heads, dh, ws, H, W, 0, stream_ptr(q.device))
    out, lse = torch.empty_like(d), torch.empty(B * L, heads, H, W, device=DEV)
    l = _lib.lib()
    _lib.check(l.gencomm_swap_attn_train_fwd(ptr(q), ptr(t), ptr(nv), ptr(out), ptr(lse), *dims), "gencomm_swap_attn_train_fwd")
    dqkv, once, twice = torch.empty_like(q), torch.zeros_like(t), torch.full_like(t, 3.0)
    _lib.check(l.gencomm_swap_attn_bwd(ptr(q), ptr(t), ptr(nv), ptr(out), ptr(lse), ptr(d), ptr(dqkv), ptr(once), *dims), "gencomm_swap_attn_bwd")
    _lib.check(l.gencomm_swap_attn_bwd(ptr(q), ptr(t), ptr(nv), ptr(out), ptr(lse), ptr(d), ptr(dqkv), ptr(twice), *dims), "gencomm_swap_attn_bwd")
    assert float(once.abs().max()) > 0.1
    assert torch.allclose(twice, once + 3.0, rtol=1e-5, atol=1e-5)


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def _module(args, seed, trainable=True):
    m = CoBEVT(args, trainable=trainable).eval()
    synth.fill_params_(m, seed)
    return m.to(DEV)


def _step(m, x, rl, aff, g, x_grad=True):
    """One forward + backward of the loss (y * g).sum(): (y, dx or None, {parameter name: gradient or None})."""
    for p in m.parameters():
        p.grad = None
    xd = torch.from_numpy(x).to(DEV).requires_grad_(x_grad)
    y = m(xd, list(rl), torch.from_numpy(aff).to(DEV))
    (y * torch.from_numpy(g).to(DEV)).sum().backward()
    return y.detach(), xd.grad, {k: p.grad for k, p in m.named_parameters()}


@pytest.mark.parametrize("tag", list(R.CASES))
def test_module_gradients_vs_reference_golden(tag):
    """eval() mode. a, b, c, e: dx and every parameter gradient against the reference's stored float64 gradients; d: against the float64
    restatement computed here (which test_cobevt_train.py holds to the stored dx, norms and dot products). Yardstick: the reference's
    float32 run against its float64 run, stored per gradient."""
    rec = load_golden()
    args, x, rl, aff, g, seed, y64, dx64, g64 = restated_grads(tag)
    names, yard = json.loads(str(rec[f"names_{tag}"])), rec[f"yard_{tag}"]
    m = _module(args, seed)
    poison()
    y, dx, grads = _step(m, x, rl, aff, g)
    with torch.no_grad():
        plain = _module(args, seed, trainable=False)(torch.from_numpy(x).to(DEV), rl, torch.from_numpy(aff).to(DEV))
        assert torch.equal(m(torch.from_numpy(x).to(DEV), rl, torch.from_numpy(aff).to(DEV)), plain)
    assert torch.equal(y, plain)                                    # the grad-enabled forward has the no_grad forward's bits
    assert list(grads) == names
    check(f"cobevt train case {tag} dx", dx, stored(rec, "dx", tag) if tag in FULL else dx64, yard[0])
    for i, k in enumerate(names):
        truth = stored(rec, f"p{i}", tag) if tag in FULL else g64[k]
        assert grads[k] is not None and tuple(grads[k].shape) == tuple(truth.shape), k
        check(f"cobevt train case {tag} {k}", grads[k], truth, yard[1 + i])


FRESH = dict(C=64, dim_head=32, ws=4, L=5, H=12, W=8, depth=2, record_len=[1, 5, 2])
_FRESH = {}


def _fresh(masks=None, key="eval"):
    """The fresh case (three scenes of 1, 5 and 2 agents, identity poses for the full one) with its float64 truth and float32 yardstick
    from the restatement; computed once per `key` and left unchanged."""
    if key not in _FRESH:
        args = R.case_args(FRESH)
        rng = np.random.RandomState(78)
        x = np.maximum(rng.standard_normal((8, 64, 12, 8)), 0.0).astype(np.float32)
        aff = R.make_affine(FRESH["record_len"], 5, 12, 8, 79, identity_scenes=(1,))
        g = rng.standard_normal((3, 64, 12, 8)).astype(np.float32)
        m = CoBEVT(args, trainable=True).eval()
        synth.fill_params_(m, 77)
        sd = m.state_dict()
        cpu = None if masks is None else [t.cpu() for t in masks]
        t64 = TR.cobevt_grads(sd, args, torch.from_numpy(x), FRESH["record_len"], torch.from_numpy(aff), torch.from_numpy(g), torch.float64, cpu)
        t32 = TR.cobevt_grads(sd, args, torch.from_numpy(x), FRESH["record_len"], torch.from_numpy(aff), torch.from_numpy(g), torch.float32, cpu)
        _FRESH[key] = (args, x, aff, g, t64, t32)
    return _FRESH[key]


def _check_step(what, got, t64, t32, names=None):
    y, dx, grads = got
    check(f"{what} output", y, t64[0], t32[0])
    check(f"{what} dx", dx, t64[1], t32[1])
    for k in (names if names is not None else t64[2]):
        assert grads[k] is not None, k
        check(f"{what} {k}", grads[k], t64[2][k], t32[2][k])


def test_module_gradients_vs_restatement_on_fresh_inputs():
    args, x, aff, g, t64, t32 = _fresh()
    m = _module(args, 77)
    poison()
    _check_step("cobevt train record_len [1, 5, 2]", _step(m, x, FRESH["record_len"], aff, g), t64, t32)


def _draw_masks(args, n_rows, H, W, p):
    """The masks in the module's documented order, from the device generator's current state."""
    shape = (n_rows, args["input_dim"], H, W)
    assert args["mlp_dim"] == args["input_dim"]
    return [(torch.rand_like(torch.empty(shape, device=DEV)) >= p).float() / (1.0 - p) for _ in range(args["depth"] * 2 * 3)]


def test_dropout_masks_are_drawn_in_the_documented_order_and_replayed():
    """train() mode, p = 0.1: the test re-seeds, draws the masks itself (per block: window to_out, window FFN after the GELU, window FFN
    after the last Linear, the same three for grid; each [B L, C, H, W]) and feeds them to the float64 restatement."""
    args, x, aff, g, _, _ = _fresh()
    rl = FRESH["record_len"]
    m = _module(args, 77).train()
    assert m.drop_out == 0.1
    torch.manual_seed(1234)
    got = _step(m, x, rl, aff, g)
    again = _step(m, x, rl, aff, g)[0]                              # the generator moved on: other masks
    assert not torch.equal(got[0], again)
    torch.manual_seed(1234)
    masks = _draw_masks(args, len(rl) * FRESH["L"], FRESH["H"], FRESH["W"], 0.1)
    dropped = float(torch.stack([(t == 0).float().mean() for t in masks]).mean())
    assert 0.08 < dropped < 0.12, dropped
    _, _, _, _, t64, t32 = _fresh(masks, "dropout")
    _check_step("cobevt train() with dropout 0.1", got, t64, t32)
    with torch.no_grad():                                           # train() mode draws masks without gradients too
        torch.manual_seed(1234)
        y = m(torch.from_numpy(x).to(DEV), rl, torch.from_numpy(aff).to(DEV))
    assert torch.equal(y, got[0])


def test_stage2_pattern_frozen_parameters_still_pass_the_input_gradient():
    args, x, aff, g, t64, t32 = _fresh()
    rl = FRESH["record_len"]
    m = _module(args, 77)
    full = _step(m, x, rl, aff, g)
    frozen = [k for k, _ in m.named_parameters() if k.startswith("layers.0.grid_attention.")]
    assert len(frozen) == 5
    for k, p in m.named_parameters():
        p.requires_grad_(k not in frozen)
    y, dx, grads = _step(m, x, rl, aff, g)
    assert all(grads[k] is None for k in frozen)
    rest = [k for k in grads if k not in frozen]
    _check_step("cobevt train, one attention frozen", (y, dx, grads), t64, t32, rest)
    for k in rest:                                                  # unchanged: the same sums, to the float atomics' reordering
        assert rel(grads[k], full[2][k]) <= 1e-6, k
    for p in m.parameters():
        p.requires_grad_(False)
    y, dx, grads = _step(m, x, rl, aff, g)
    assert all(v is None for v in grads.values()) and torch.equal(y, full[0])
    check("cobevt train, every parameter frozen: dx", dx, t64[1], t32[1])
    with pytest.raises(RuntimeError, match="does not require grad"):      # nothing requires grad: a plain forward
        _step(m, x, rl, aff, g, x_grad=False)


def test_two_steps_are_bit_identical_where_the_order_is_fixed():
    """Covered: the output and dx. Every parameter gradient meets in float atomics (gencomm_amd/cobevt_bwd.py: the table in
    gencomm_swap_attn_bwd, the Linears in gencomm_conv2d_wgrad, the LayerNorms in gencomm_ln_nchw_bwd) and is declared NOT order-fixed; so
    is the warp's scatter into dx, which under identity poses (one warped pixel with a non-zero weight per input pixel) has nothing to
    reorder -- the poses used here, so that dx shows the whole chain in front of the warp: dq, dk, dv of gencomm_swap_attn_bwd included.
    NaNs are planted in the allocator's free memory before each step; the parameter gradients must agree to the atomics' reordering."""
    c = dict(C=64, dim_head=32, ws=4, L=3, H=8, W=12, depth=1, record_len=[3, 1])
    args = R.case_args(c)
    m = _module(args, 5)
    rng = np.random.RandomState(6)
    x = np.maximum(rng.standard_normal((4, 64, 8, 12)), 0.0).astype(np.float32)
    aff = R.make_affine([3, 1], 3, 8, 12, 7, identity_scenes=(0, 1))
    g = rng.standard_normal((2, 64, 8, 12)).astype(np.float32)
    poison()
    y_a, dx_a, g_a = _step(m, x, [3, 1], aff, g)
    poison()
    y_b, dx_b, g_b = _step(m, x, [3, 1], aff, g)
    assert torch.isfinite(dx_a).all() and float(dx_a.abs().max()) > 0
    assert torch.equal(y_a, y_b) and torch.equal(dx_a, dx_b)
    for k in g_a:
        assert rel(g_a[k], g_b[k]) <= 1e-6, k


def test_stage1_shell_trains_with_cobevt():
    """One forward + backward of the stage-1 shell in train() mode with `fusion_method: cobevt` (drop_out 0.1) on the small shell spec:
    every fusion_net parameter and every trained module upstream of it receives a finite gradient that is not all zero."""
    from test_cobevt import _shell_args
    from gencomm_amd.heter_model_baseline_w_gencomm_stage1 import HeterModelBaselineWGenCommStage1 as Shell
    s = load_case("shell")
    args = _shell_args()
    model = Shell(copy.deepcopy(args))
    synth.fill_params_(model, int(s["weight_seed"]))
    synth.fill_bn_stats_(model, int(s["bn_seed"]))
    model = model.to(DEV).train()
    assert model.fusion_net.trainable and model.fusion_net.training
    rl = [int(v) for v in s["record_len"]]
    pil = synth.make_pillars(int(s["M"]), sum(rl), int(s["nx"]), int(s["ny"]), int(s["data_seed"]), voxel_size=[0.4, 0.4, 4.0],
                             pc_range=args["lidar_range"])
    ptm = synth.make_pairwise_t_matrix(rl, 5, int(s["pose_seed"]), max_shift=float(s["max_shift"]))
    data = {"agent_modality_list": ["m1"] * sum(rl), "record_len": torch.tensor(rl), "pairwise_t_matrix": torch.from_numpy(ptm).to(DEV),
            "inputs_m1": {k: torch.from_numpy(pil[k]).to(DEV) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}}
    torch.manual_seed(11)
    out = model(data)
    loss = (out["cls_preds"].square().mean() + out["reg_preds"].square().mean() + out["dir_preds"].square().mean()
            + (out["pred_feature"] - out["gt_feature"].detach()).square().mean())
    loss.backward()
    upstream = ("encoder_m1.", "backbone_m1.", "shrinker_m1.", "message_extractor_m1.", "gencomm.", "enhancer.", "fusion_net.")
    dead = {n for n, _ in model.enhancer.named_parameters() if not n.startswith(("block_1.norm", "block_1.mlp", "split_attn"))}   # never run by the reference's forward
    checked = fusion = 0
    for n, p in model.named_parameters():
        if not p.requires_grad or not n.startswith(upstream) or (n.startswith("enhancer.") and n[len("enhancer."):] in dead):
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0.0, n
        checked += 1
        fusion += n.startswith("fusion_net.")
    assert fusion == len(list(model.fusion_net.parameters())) == 26 and checked > 60
    print(f"stage-1 training step with fusion_method cobevt: loss {float(loss.detach()):.4f}, {checked} parameters with a non-zero gradient")
