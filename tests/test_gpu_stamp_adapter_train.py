"""The backward of the fused ConvNeXt block (gencomm_convnext_block_bwd) and the trainable STAMP adapter / reverter on the GPU.

The block against float64 autograd of the restated block (tests/stamp_adapter_train_restatement.py), per tensor relative rms error
<= max(2 x the float32 restatement's own error, 1e-6), no tensor left out, at the smallest shapes where it can go wrong: maps smaller than
the window, batches, ragged tiles on both axes, several tiles per slab with a ragged last slab (slabs forced), both widths. The taps, x
(standard deviation 2) and dy are random and asymmetric: the float64 gradient with a flipped or transposed window is far outside the
criterion. The modules against the reference's own float64 autograd stored in tests/golden/stamp_adapter_train_*.npz.
"""
import os
import re

import pytest
import torch

import stamp_adapter_restatement as R
import stamp_adapter_train_restatement as T
from gencomm_amd import Adapter, Reverter, _lib
from gencomm_amd import convnext_bwd as B
from gencomm_amd.runtime import ptr, stream_ptr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda:0")
ORDER = T.ORDER
_cache = {}


def _tile():
    src = open(os.path.join(HERE, "..", "gencomm_amd", "csrc", "convnext_kernels.h")).read()
    return int(re.search(r"kCnxTileH = (\d+)", src).group(1)), int(re.search(r"kCnxTileW = (\d+)", src).group(1))


TILE_H, TILE_W = _tile()
BLOCK_SHAPES = [   # (C, n, H, W, slabs)
    (64, 1, 1, 1, 0), (64, 1, 3, 5, 0), (64, 1, 6, 7, 0),     # smaller than the window
    (64, 2, 8, 8, 0),                                         # W % 4 == 0 (the 16-byte path), batch stride
    (64, 3, 9, 17, 0),
    (64, 1, TILE_H + 1, 2 * TILE_W + 1, 0),                   # ragged on both axes
    (64, 1, 19, 35, 4), (64, 1, 19, 35, 0),                   # 15 tiles: 4 slabs of 4, 4, 4, 3 tiles; then one tile per slab
    (128, 1, 3, 5, 0), (128, 2, 9, 17, 0), (128, 1, 19, 35, 4),
]


def _gold(name):
    if ("gold", name) not in _cache:
        _cache[("gold", name)] = T.load_fixture(name)
    return _cache[("gold", name)]


def _block_case(C, n, H, W, gamma=True):
    """(params, x, dy, float64 gradients, float32 yardstick per tensor), computed once and shared."""
    key = (C, n, H, W, gamma)
    if key not in _cache:
        seed = 7000 + 131 * C + 17 * n + 5 * H + W
        p = R.make_block_params(C, seed)
        if not gamma:
            p["gamma"] = None
        x = 2.0 * R.make_x((n, C, H, W), seed + 1)
        dy = R.make_x((n, C, H, W), seed + 2)
        truth = T.block_grads(p, x, dy, torch.float64)
        g32 = T.block_grads(p, x, dy, torch.float32)
        _cache[key] = (p, x, dy, truth, {k: T.rel_rms(g32[k], truth[k]) for k in truth})
    return _cache[key]


def _raw_bwd(p, x, dy, dx_only=False, slabs=0, C=None):
    """One direct ABI call on NaN-filled outputs: (status, dx, {name: gradient})."""
    n, Cx, H, W = x.shape
    C = C or Cx
    pd = [None if p[k] is None else p[k].to(DEV) for k in ORDER]
    xd, dyd = x.to(DEV), dy.to(DEV)
    dx = torch.full_like(xd, float("nan"))
    grads = [None if t is None else torch.full_like(t, float("nan")) for t in pd]
    need = _lib.lib().gencomm_convnext_block_bwd_workspace_bytes(n, C if C in (64, 128) else 64, H, W, int(dx_only), slabs)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = _lib.lib().gencomm_convnext_block_bwd(ptr(xd), ptr(dyd), *[ptr(t) for t in pd], ptr(dx), *[ptr(g) for g in grads],
                                               int(dx_only), slabs, n, C, H, W, ptr(ws), ws.numel(), stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, dx, {k: g for k, g in zip(ORDER, grads) if g is not None}


@pytest.mark.parametrize("C,n,H,W,slabs", BLOCK_SHAPES)
def test_block_backward_against_float64(C, n, H, W, slabs):
    p, x, dy, truth, yard = _block_case(C, n, H, W)
    rc, dx, grads = _raw_bwd(p, x, dy, slabs=slabs)
    assert rc == 0, _lib.lib().gencomm_last_error().decode()
    got = dict(grads, x=dx)
    assert sorted(got) == sorted(truth)
    worst = 0.0
    for k in sorted(truth):
        assert not torch.isnan(got[k]).any(), f"{k}: an element was not written"
        e = T.rel_rms(got[k].cpu(), truth[k])
        print(f"C {C} [{n}, {C}, {H}, {W}] slabs {slabs} {k}: rel rms {e:.3e} (float32 restatement {yard[k]:.3e})")
        worst = max(worst, e)
    print(f"worst {worst:.3e}")
    for k in sorted(truth):
        T.check(k, got[k].cpu(), truth[k], yard[k])


def test_the_truth_would_catch_a_flipped_or_transposed_window():
    """The taps are asymmetric: float64 gradients computed with the window flipped or transposed are far outside the criterion."""
    p, x, dy, truth, yard = _block_case(64, 3, 9, 17)
    for name, w in (("flipped", p["dwconv.weight"].flip(-1, -2)), ("transposed", p["dwconv.weight"].transpose(-1, -2))):
        bad = T.block_grads(dict(p, **{"dwconv.weight": w.contiguous()}), x, dy, torch.float64)
        assert T.rel_rms(bad["x"], truth["x"]) > 1e-2, name
        back = bad["dwconv.weight"].flip(-1, -2) if name == "flipped" else bad["dwconv.weight"].transpose(-1, -2)
        assert T.rel_rms(bad["dwconv.weight"], truth["dwconv.weight"]) > 1e-2 and T.rel_rms(back, truth["dwconv.weight"]) > 1e-2, name


@pytest.mark.parametrize("C,n,H,W,slabs", [(64, 3, 9, 17, 0), (128, 2, 9, 17, 0), (64, 1, 19, 35, 4), (128, 1, 19, 35, 4)])
def test_two_runs_are_bit_identical_and_autograd_is_the_abi_call(C, n, H, W, slabs):
    p, x, dy, _, _ = _block_case(C, n, H, W)
    rc0, dx0, g0 = _raw_bwd(p, x, dy, slabs=slabs)
    rc1, dx1, g1 = _raw_bwd(p, x, dy, slabs=slabs)
    assert rc0 == 0 and rc1 == 0
    assert torch.equal(dx0, dx1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    dx2, g2 = B.convnext_block_bwd(x.to(DEV), dy.to(DEV), [p[k].to(DEV) for k in ORDER], slabs=slabs)
    assert torch.equal(dx0, dx2) and all(torch.equal(g0[k], g) for k, g in zip(ORDER, g2))
    dyd = dy.to(DEV)   # dx may be dy itself
    dx3, g3 = B.convnext_block_bwd(x.to(DEV), dyd, [p[k].to(DEV) for k in ORDER], slabs=slabs, out=dyd)
    assert dx3 is dyd and torch.equal(dx0, dx3) and all(torch.equal(g0[k], g) for k, g in zip(ORDER, g3))


def test_block_backward_without_gamma():
    p, x, dy, truth, yard = _block_case(64, 2, 8, 8, gamma=False)
    rc, dx, grads = _raw_bwd(p, x, dy)
    assert rc == 0 and "gamma" not in grads and "gamma" not in truth
    for k, g in dict(grads, x=dx).items():
        T.check(k, g.cpu(), truth[k], yard[k])


def test_dx_only_and_launch_counts():
    p, x, dy, _, _ = _block_case(64, 1, 19, 35)
    with _lib.kernel_log() as full:
        rc0, dx0, g0 = _raw_bwd(p, x, dy, slabs=4)
    with _lib.kernel_log() as only:
        rc1, dx1, g1 = _raw_bwd(p, x, dy, dx_only=True, slabs=4)
    assert rc0 == 0 and rc1 == 0
    assert torch.equal(dx0, dx1)
    assert all(torch.isnan(g).all() for g in g1.values())          # untouched
    assert sum(full.counts.values()) == B.LAUNCHES <= 6, full.counts
    assert sum(only.counts.values()) == B.LAUNCHES_DX_ONLY < B.LAUNCHES, only.counts


def test_refusals_launch_nothing():
    p, x, dy, _, _ = _block_case(64, 2, 8, 8)
    err = lambda: _lib.lib().gencomm_last_error().decode()
    with _lib.kernel_log() as kl:
        p32 = {k: torch.zeros(s) for k, s in R.block_shapes(32).items()}
        rc = _raw_bwd(p32, torch.zeros(1, 32, 4, 4), torch.zeros(1, 32, 4, 4), C=32)[0]
        assert rc == 1 and "C must be 64 or 128" in err() and "32" in err()
        xd = x.to(DEV)
        pd = [p[k].to(DEV) for k in ORDER]
        gr = [torch.empty_like(t) for t in pd]
        ws = torch.empty(B.workspace_bytes(2, 64, 8, 8), dtype=torch.uint8, device=DEV)
        call = lambda dxp, dyp, nbytes: _lib.lib().gencomm_convnext_block_bwd(ptr(xd), dyp, *[ptr(t) for t in pd], dxp, *[ptr(g) for g in gr], 0, 0, 2, 64,
                                                                             8, 8, ptr(ws), nbytes, stream_ptr(DEV))
        dyd = dy.to(DEV)
        assert call(ptr(xd), ptr(dyd), ws.numel()) == 1 and "dx must not alias x" in err()
        assert call(ptr(xd.view(-1)[64:]), ptr(dyd), ws.numel()) == 1 and "dx must not alias x" in err()
        other = torch.empty(xd.numel() + 64, device=DEV)
        assert call(ptr(other[4:]), ptr(other), ws.numel()) == 1 and "dy" in err()       # a partial overlap with dy
        assert call(ptr(other), ptr(dyd), ws.numel() - 16) == 2 and "workspace" in err()
        assert call(0, ptr(dyd), ws.numel()) == 1 and "null pointer" in err()
    torch.cuda.synchronize()
    assert not kl.counts, kl.counts


# ----------------------------------------------------------------------------------------------------------- modules
def _trainable(cls, cfg, sd):
    mod = {"Adapter": Adapter, "Reverter": Reverter}[cls](cfg, trainable=True)
    mod.load_state_dict(sd, strict=True)
    return mod.to(DEV)


def _named_grads(mod):
    return {k: p.grad for k, p in mod.named_parameters()}


@pytest.mark.parametrize("name", T.TRAIN_CASES)
def test_modules_against_the_references_float64_gradients(name):
    g = _gold(name)
    cls, cfg, sd, x = R.case_data(name, int(g["seed"]))
    mod = _trainable(cls, cfg, sd)
    xd = x.to(DEV).requires_grad_(True)
    y = mod(xd)
    G = T.make_G(tuple(y.shape), int(g["seed"]) + 2)
    (y * G.to(DEV)).sum().backward()
    got = dict(_named_grads(mod), x=xd.grad)
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(T.trained(sd) + ["x"])
    for k in list(sd):
        if ".smoothing." in k:
            assert got[k] is None
    worst = 0.0
    for i, k in enumerate(keys):
        yard = float(g[f"yard/{k}"])
        if f"grad64/{k}" in g:
            e = T.check(k, got[k].cpu(), torch.from_numpy(g[f"grad64/{k}"]), yard)
        else:   # a big matrix of the dim-128 case: its digest (the block tests compare these matrices element by element)
            e = T.check_digest(k, got[k].cpu(), g[f"digest64/{k}"], yard, int(g["seed"]), i)
        print(f"{name} {k}: {'rel rms' if f'grad64/{k}' in g else 'digest projection'} {e:.3e} (the reference's float32 {yard:.3e})")
        worst = max(worst, e)
    print(f"{name}: worst {worst:.3e}")


def _step_modules():
    g = _gold("step")
    data = T.step_data(int(g["seed"]))
    cfg_a, sd_a, cfg_r, sd_r, FM, FP = data
    return g, data, _trainable("Adapter", cfg_a, sd_a), _trainable("Reverter", cfg_r, sd_r)


def _device_step_loss(a, r, FM, FP):
    mse = torch.nn.functional.mse_loss
    FM2P = a(FM)
    return T.ALPHA["alpha_P2M"] * mse(r(FP), FM) + T.ALPHA["alpha_M2P2M"] * mse(r(FM2P), FM) + T.ALPHA["alpha_M2P"] * mse(FM2P, FP)


def test_adapter_training_step_against_the_references_gradients_and_one_sgd_step():
    g, data, a, r = _step_modules()
    FM, FP = data[4].to(DEV), data[5].to(DEV)
    loss = _device_step_loss(a, r, FM, FP)          # the reverter is called twice in the step
    loss.backward()
    assert FM.grad is None
    got = dict(_named_grads(a), **_named_grads(r))
    keys = [str(k) for k in g["keys"]]
    assert sorted(keys) == sorted(T.trained(data[1]) + T.trained(data[3]))
    assert all(got[k] is None for k in got if ".smoothing." in k)
    ref_loss = float(g["loss64"])
    assert abs(float(loss) - ref_loss) <= 1e-5 + 1e-4 * abs(ref_loss)
    worst = 0.0
    for k in keys:
        e = T.check(k, got[k].cpu(), torch.from_numpy(g[f"grad64/{k}"]), float(g[f"yard/{k}"]))
        print(f"step {k}: rel rms {e:.3e} (the reference's float32 {float(g['yard/' + k]):.3e})")
        worst = max(worst, e)
    print(f"step: worst {worst:.3e}")
    # one SGD step: lr such that the first-order decrease is 5 % of the loss
    truth = {k: torch.from_numpy(g[f"grad64/{k}"]) for k in keys}
    lr = 0.05 * ref_loss / float(sum(v.pow(2).sum() for v in truth.values()))
    after64 = T.sgd_step(data, truth, lr, torch.float64)
    opt = torch.optim.SGD([p for m in (a, r) for n, p in m.named_parameters() if ".smoothing." not in n], lr=lr)
    opt.step()
    with torch.no_grad():
        after = float(_device_step_loss(a, r, FM, FP))
    print(f"loss {float(loss):.6f} -> {after:.6f} (float64 restatement {ref_loss:.6f} -> {after64:.6f})")
    assert after < float(loss) and abs(after - after64) <= 1e-5 + 1e-4 * abs(after64)


def test_frozen_module_with_trainable_input_gives_dx_only():
    cls, cfg, sd, x = R.case_data("cnx64", 4242)
    mod = _trainable(cls, cfg, sd)
    for p in mod.parameters():
        p.requires_grad_(False)
    G = T.make_G((2, 128, 12, 20), 4244)
    truth = T.module_grads(cfg, sd, "adapter", x, G, torch.float64)["x"]
    yard = T.rel_rms(T.module_grads(cfg, sd, "adapter", x, G, torch.float32)["x"], truth)
    xd = x.to(DEV).requires_grad_(True)
    with _lib.kernel_log() as kl:
        (mod(xd) * G.to(DEV)).sum().backward()
    assert all(p.grad is None for p in mod.parameters())
    assert "cnx_bwd_weight_kernel<64>" not in kl.counts and kl.counts.get("cnx_bwd_pixel_kernel<64>") == 3
    T.check("x", xd.grad.cpu(), truth, yard)


def test_inference_is_unchanged():
    cls, cfg, sd, x = R.case_data("cnx64", 4242)
    mod, plain = _trainable(cls, cfg, sd), Adapter(cfg)
    plain.load_state_dict(sd, strict=True)
    plain.to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        y0 = plain(xd)
        with _lib.kernel_log() as kl:
            y1 = mod(xd)
    assert torch.equal(y0, y1) and kl.counts.get("convnext_block_kernel<64>") == 3 and not [k for k in kl.counts if k.startswith("cnx_bwd")]
    y2 = mod(xd)                                    # grad-enabled: the same forward launches, the same bits
    assert y2.requires_grad and torch.equal(y0, y2.detach())
    for p in mod.parameters():
        p.requires_grad_(False)
    assert not mod(xd).requires_grad                # nothing to differentiate: the inference path


def test_identity_passes_the_gradient_through():
    mod = Adapter(R.CASES["identity"][1], trainable=True)
    x = torch.randn(1, 128, 3, 5, device=DEV, requires_grad=True)
    G = torch.randn(1, 128, 3, 5, device=DEV)
    (mod(x) * G).sum().backward()
    assert torch.equal(x.grad, G)
