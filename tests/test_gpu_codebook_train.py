"""Training the fused CodeFilling codec on the GPU: gencomm_umgm_bwd behind ``UMGMQuantizer(..., trainable=True)``.

Criterion (as test_gpu_cobevt_train.py / test_gpu_v2vnet_train.py): truth = float64 on the CPU; yardstick = the same computation in
float32; the HIP gradient's relative rms error against the truth is <= max(2 x the yardstick's, 1e-6), per tensor. Fixture cases
(tests/golden/codebook_train.npz) use the reference's own stored float32 yardstick and the float64 restatement's full gradients, after
the kernel's sampled indices have been asserted equal to the reference's; every other case forces the kernel's own sampled indices on
the restatement (float64 truth, float32 yardstick), which makes the function smooth: no near-tie margin, no excluded rows. Every case
also runs the ABI entry directly into NaN-filled gradient buffers and must get the autograd path's bits back.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import codebook_restatement as R
import codebook_train_restatement as T
from gencomm_amd import UMGMQuantizer, _lib
from gencomm_amd import codebook_bwd as B
from gencomm_amd.runtime import ptr, stream_ptr

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebook_train.npz"))
DEV = torch.device("cuda:0")
_cache = {}


def _module(c, sd, trainable=True):
    mod = UMGMQuantizer(c["C"], c["m"], list(c["k"]), 0.0, R.components(c["C"]), trainable=trainable)
    mod.load_state_dict(sd, strict=True)
    return mod.to(DEV).eval()


def _abi_bwd(mod, x, HW, keep, noise_args, sampled, g_restored, g_loss, dx_only=False):
    """gencomm_umgm_bwd into NaN-filled buffers -> (dx, gradient blob or None)"""
    l, (mode, u, seed) = _lib.lib(), noise_args
    rows = x.shape[0] if HW == 0 else x.shape[0] * HW
    blob = mod._params(DEV)
    dx = torch.full_like(x, float("nan"))
    dblob = None if dx_only else torch.full_like(blob, float("nan"))
    need = l.gencomm_umgm_bwd_workspace_bytes(rows, mod._channel, mod._m, mod._k_arr, len(mod._k))
    assert need > 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(l.gencomm_umgm_bwd(ptr(blob), ptr(x), ptr(keep), ptr(u), seed, mode, ptr(sampled), ptr(g_restored), ptr(g_loss), ptr(dx), ptr(dblob),
                                  int(dx_only), x.shape[0], HW, mod._channel, mod._m, mod._k_arr, len(mod._k), ptr(ws), need, stream_ptr(DEV)),
               "gencomm_umgm_bwd")
    torch.cuda.synchronize()
    return dx, dblob


def _hip(mod, x, G, lw, uniforms=None, seed=None, noise=True, map_shape=None, keep=None, check_abi=True):
    """One training step's gradients through autograd -> (dict key -> gradient (CPU) with "x", sampled (CPU list), restored, loss).
    x, G: CPU rows [n, C]; map_shape (A, H, W) sends them through forward_map as NCHW."""
    for p in mod.parameters():
        p.grad = None
    n, C = x.shape
    u_dev = None if uniforms is None else [t.to(DEV) for t in uniforms]
    with torch.no_grad():
        sampled = mod(x.to(DEV), uniforms=u_dev, seed=seed, noise=noise, return_sampled=True)[4]
    to_dev = (lambda t: t.to(DEV)) if map_shape is None else (lambda t: t.reshape(map_shape[0], map_shape[1], map_shape[2], C).permute(0, 3, 1, 2).contiguous().to(DEV))
    xd = to_dev(x).requires_grad_(True)
    Gd = None if G is None else to_dev(G)
    if map_shape is None:
        restored, _, _, loss, s2 = mod(xd, uniforms=u_dev, seed=seed, noise=noise, return_sampled=True)
        assert all(torch.equal(a, b) for a, b in zip(sampled, s2))
    else:
        restored, _, _, loss = mod.forward_map(xd, keep=keep, uniforms=u_dev, seed=seed, noise=noise)
    assert restored.requires_grad and loss.requires_grad
    obj = lw * loss if lw else None
    if Gd is not None:
        obj = (restored * Gd).sum() if obj is None else obj + (restored * Gd).sum()
    obj.backward()
    torch.cuda.synchronize()
    if check_abi:
        HW = 0 if map_shape is None else map_shape[1] * map_shape[2]
        kp = None if keep is None else torch.as_tensor(keep).to(device=DEV, dtype=torch.uint8)
        rows = n
        na = mod._noise_args(rows, u_dev, seed, noise, DEV)
        gl = torch.tensor(float(lw), dtype=torch.float32, device=DEV) if lw else None
        dx, dblob = _abi_bwd(mod, xd.detach(), HW, kp, na, torch.stack(sampled).contiguous(), Gd, gl)
        assert torch.equal(dx, xd.grad), "dx: the ABI entry on NaN-filled buffers differs from the autograd path"
        assert not bool(torch.isnan(dblob).any()), "a slot of the gradient blob was not written"
        for p, g in zip(B._unique_params(mod), B._slice_grads(mod, dblob)):
            assert torch.equal(p.grad, g)
    back = (lambda t: t.cpu()) if map_shape is None else (lambda t: t.permute(0, 2, 3, 1).reshape(n, C).cpu())
    grads = {"x": back(xd.grad)}
    for key, p in mod.named_parameters():
        grads[key] = p.grad.cpu()
    return grads, [s.cpu() for s in sampled], back(restored.detach()), float(loss.detach())


def _judge(label, hip, truth, yard):
    """per tensor: print the HIP error and the yardstick, then assert"""
    bad = []
    for key in sorted(truth):
        if float(truth[key].abs().max()) == 0.0:
            assert float(hip[key].abs().max()) == 0.0, key
            continue
        e, y = T.rel_rms(hip[key], truth[key]), yard[key]
        print(f"{label} {key}: HIP rel rms {e:.3e}, float32 yardstick {y:.3e}")
        if not e <= max(2.0 * y, 1e-6):
            bad.append((key, e, y))
    assert not bad, bad


def _forced_case(tag, hip_kw=None, n=128, C=64, m=2, k=(16, 16, 16), scales=(1.0, 1.0), lw=T.LOSS_WEIGHT, with_G=True, noise="uniforms", seed=4200,
                 map_shape=None, keep=None, mutate=None):
    c = dict(C=C, m=m, k=list(k), n=n)
    sd = R.make_params(C, m, c["k"], seed, *scales)
    if mutate is not None:
        mutate(sd)
    x, u = R.make_x(n, C, seed + 1), R.make_uniforms(n, m, c["k"], seed + 2)
    G = torch.from_numpy(np.random.default_rng(seed + 3).normal(0.0, 1.0, (n, C)).astype(np.float32)) if with_G else None
    mod = _module(c, sd)
    kw = dict(hip_kw or {})
    if noise == "uniforms":
        kw["uniforms"] = u
    elif noise == "philox":
        kw["seed"] = 77
        u = [t.cpu() for t in mod.philox_uniforms(77, n)]
    else:
        kw["noise"], u = False, None
    hip, sampled, _, _ = _hip(mod, x, G, lw, map_shape=map_shape, keep=keep, **kw)
    keep_rows = None
    if keep is not None:
        HW = map_shape[1] * map_shape[2]
        keep_rows = torch.tensor(keep, dtype=torch.bool).repeat_interleave(HW)
    g64, _ = T.gradients(sd, x, m, c["k"], u, sampled, G, lw, torch.float64, keep_rows=keep_rows)
    g32, _ = T.gradients(sd, x, m, c["k"], u, sampled, G, lw, torch.float32, keep_rows=keep_rows)
    _judge(tag, hip, g64, {key: T.rel_rms(g32[key], g64[key]) for key in g64})
    return hip, g64, mod, sd, x, u, G, sampled


@pytest.mark.parametrize("name", list(T.STRICT))
def test_fixture_strict_cases(name):
    c, sd, x, u, G = T.case_data(name, int(GOLD[f"{name}/seed"]))
    mod = _module(c, sd)
    hip, sampled, _, loss = _hip(mod, x, G, T.LOSS_WEIGHT, uniforms=u)
    for l, s in enumerate(sampled):
        assert torch.equal(s, torch.from_numpy(GOLD[f"{name}/sampled64_{l}"].astype(np.int64))), f"level {l}: sampled indices differ from the reference's"
    g64, _ = T.gradients(sd, x, c["m"], c["k"], u, None, G, T.LOSS_WEIGHT, torch.float64)
    assert abs(loss - float(GOLD[f"{name}/loss64"])) <= 1e-5 * float(GOLD[f"{name}/loss64"])
    _judge(name, hip, g64, {key: float(GOLD[f"{name}/yard32/{key}"]) for key in g64})


def test_fixture_soft_case_forced_indices():
    c, sd, x, u, G = T.case_data("soft", int(GOLD["soft/seed"]))
    mod = _module(c, sd)
    hip, sampled, _, _ = _hip(mod, x, G, T.LOSS_WEIGHT, uniforms=u)
    g64, _ = T.gradients(sd, x, c["m"], c["k"], u, sampled, G, T.LOSS_WEIGHT, torch.float64)
    g32, _ = T.gradients(sd, x, c["m"], c["k"], u, sampled, G, T.LOSS_WEIGHT, torch.float32)
    _judge("soft", hip, g64, {key: T.rel_rms(g32[key], g64[key]) for key in g64})


@pytest.mark.parametrize("n", [1, 63, 65])
def test_row_counts_around_a_tile(n):
    _forced_case(f"n{n}", n=n)


def test_forward_map_with_a_kept_agent():
    """3 x 64 x 5 x 7, keep = [1, 0, 0]: HW = 35, tiles straddle agents. The truth replaces the kept agent's restored rows by x, so its
    dx is g_restored plus the code_loss term through the codec."""
    hip, g64, *_ = _forced_case("map", n=105, map_shape=(3, 5, 7), keep=[1, 0, 0], scales=(4.0, 2.0))
    assert float(hip["x"][:35].abs().max()) > 0.0


def test_noise_off():
    _forced_case("noise_off", noise=None)


def test_philox_noise_in_the_kernel():
    _forced_case("philox", noise="philox", n=100)


def test_one_level():
    _forced_case("one_level", k=(16,), n=70)


def test_d_restored_only():
    _forced_case("d_restored_only", lw=0.0, n=70)


def test_d_loss_only():
    _forced_case("d_loss_only", with_G=False, n=70)


def test_lower_bound_rule():
    """One group's temperature below the bound: its gradient passes where it is negative and is exactly zero where it is positive.
    The objective is linear in G (no loss term, forced indices), so G and -G give the two signs; which is which is read off the
    restatement."""
    key = "_encoders.0._quantizer._temperature"

    def low(sd):
        sd[key] = sd[key].clone()
        sd[key][1, 0] = 1e-7

    hip_a, g64_a, mod, sd, x, u, G, sampled = _forced_case("lower_bound(+G)", lw=0.0, n=70, mutate=low)
    hip_b, _, _, _ = _hip(mod, x, -G, 0.0, uniforms=u)
    g64_b, _ = T.gradients(sd, x, 2, [16, 16, 16], u, sampled, -G, 0.0, torch.float64)
    ta, tb = float(g64_a[key][1, 0]), float(g64_b[key][1, 0])
    assert (ta < 0.0 and tb == 0.0) or (ta == 0.0 and tb < 0.0), (ta, tb)
    neg, neg64, pos = (hip_a, g64_a, hip_b) if ta < 0.0 else (hip_b, g64_b, hip_a)
    assert float(pos[key][1, 0]) == 0.0
    assert float(neg[key][1, 0]) < 0.0 and abs(float(neg[key][1, 0]) - float(neg64[key][1, 0])) <= 1e-4 * abs(float(neg64[key][1, 0]))
    assert float(pos[key][0, 0]) == -float(neg[key][0, 0]) != 0.0        # the group above the bound passes both signs


def test_two_backward_runs_give_the_same_bits():
    c, sd, x, u, G = T.case_data("c128_three_tiles", int(GOLD["c128_three_tiles/seed"]))
    mod = _module(c, sd)
    a, _, _, _ = _hip(mod, x, G, T.LOSS_WEIGHT, uniforms=u, check_abi=False)
    b, _, _, _ = _hip(mod, x, G, T.LOSS_WEIGHT, uniforms=u, check_abi=False)
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_frozen_parameters_pass_dx_through():
    c, sd, x, u, G = T.case_data("strict_a", int(GOLD["strict_a/seed"]))
    mod = _module(c, sd)
    full, sampled, _, _ = _hip(mod, x, G, T.LOSS_WEIGHT, uniforms=u, check_abi=False)
    for p in mod.parameters():
        p.requires_grad_(False)
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    restored, _, _, loss = mod(xd, uniforms=[t.to(DEV) for t in u])
    ((restored * G.to(DEV)).sum() + T.LOSS_WEIGHT * loss).backward()
    assert torch.equal(xd.grad.cpu(), full["x"])
    assert all(p.grad is None for p in mod.parameters())
    dx, none = _abi_bwd(mod, xd.detach(), 0, None, mod._noise_args(c["n"], [t.to(DEV) for t in u], None, True, DEV),
                        torch.stack([s.to(DEV) for s in sampled]).contiguous(), G.to(DEV),
                        torch.tensor(T.LOSS_WEIGHT, dtype=torch.float32, device=DEV), dx_only=True)
    assert none is None and torch.equal(dx.cpu(), full["x"])


def test_no_grad_on_a_trainable_module_is_the_default_module():
    c, sd, x, u, _ = T.case_data("strict_b", int(GOLD["strict_b/seed"]))
    a, b = _module(c, sd, True), _module(c, sd, False)
    ud = [t.to(DEV) for t in u]
    with torch.no_grad():
        oa, ob = a(x.to(DEV), uniforms=ud), b(x.to(DEV), uniforms=ud)
    xg = x.to(DEV).requires_grad_(True)
    og = a(xg, uniforms=ud)                     # and the grad-enabled forward has the same bits
    for o in (oa, og):
        assert torch.equal(o[0], ob[0]) and torch.equal(o[3], ob[3])
        assert all(torch.equal(p, q) for p, q in zip(o[1], ob[1])) and all(torch.equal(p, q) for p, q in zip(o[2], ob[2]))
    assert not og[1][0].requires_grad and not og[2][0].requires_grad
    with pytest.raises(NotImplementedError, match="codebook training is not implemented"):
        b(xg, uniforms=ud)


def test_two_sgd_steps_lower_code_loss():
    """also checks that the parameter blob cache follows the parameters' versions"""
    c, sd, x, u, _ = T.case_data("soft", int(GOLD["soft/seed"]))
    mod = _module(c, sd)
    opt = torch.optim.SGD(mod.parameters(), lr=0.05)
    xd, ud = x.to(DEV), [t.to(DEV) for t in u]
    losses, restored = [], []
    for _ in range(3):
        opt.zero_grad()
        out = mod(xd, uniforms=ud)
        losses.append(float(out[3].detach()))
        restored.append(out[0].detach().clone())
        out[3].backward()
        opt.step()
    print("code_loss over two SGD steps:", losses)
    assert losses[2] < losses[1] < losses[0]
    assert not torch.equal(restored[0], restored[1]) and not torch.equal(restored[1], restored[2])


def test_workspace_offsets_past_2_to_the_31():
    """2 803 200 rows at C = 64, one level: the row slots hold 2.15e9 floats, so the last slot's offsets pass 2^31 elements (and every
    slot's pass 2^32 bytes). The rows are one 128-row block repeated K times, without noise and without the loss term (whose scale
    depends on n): a row's result depends on nothing but the row, so dx of the first and the last block are the small run's bits, and
    every parameter gradient is K times the small run's. Bound on the latter: a weight gradient's wave adds 43 800 rows in one fp32
    chain, worst case N u = 43 800 x 6e-8 = 2.6e-3 of the summed magnitudes; 1e-3 relative rms (the typical sqrt(N) u is 1.2e-5) --
    a wrapped offset leaves NaN-filled workspace or another slot's values in the sum, an error of order 1."""
    K, c = 21900, dict(C=64, m=2, k=[16], n=128)
    sd = R.make_params(64, 2, c["k"], 4300, 4.0, 2.0)
    mod = _module(c, sd)
    xs, Gs = R.make_x(128, 64, 4301).to(DEV), R.make_x(128, 64, 4302).to(DEV)
    na = mod._noise_args(128, None, None, False, DEV)
    with torch.no_grad():
        s_small = torch.stack(mod(xs, noise=False, return_sampled=True)[4]).contiguous()
    dx_small, db_small = _abi_bwd(mod, xs, 0, None, na, s_small, Gs, None)
    xb, Gb = xs.repeat(K, 1), Gs.repeat(K, 1)
    s_big = s_small.repeat(1, K, 1).contiguous()
    dx_big, db_big = _abi_bwd(mod, xb, 0, None, na, s_big, Gb, None)
    assert torch.equal(dx_big[:128], dx_small) and torch.equal(dx_big[-128:], dx_small)
    assert torch.equal(dx_big.view(K, 128, 64)[K // 2], dx_small)
    e = T.rel_rms(db_big.cpu(), db_small.cpu() * K)
    print(f"gradient blob of {128 * K} rows against {K} x the block's: rel rms {e:.3e}")
    assert e <= 1e-3


def test_rows_wgrad_fixed_entry():
    """dW = G^T A over rows that are no multiple of 4 and span several row ranges, against float64; twice, the same bits."""
    l, rng = _lib.lib(), np.random.default_rng(5)
    rows, Co, Ci = 1027, 64, 128
    g, a = torch.from_numpy(rng.normal(size=(rows, Co)).astype(np.float32)), torch.from_numpy(rng.normal(size=(rows, Ci)).astype(np.float32))
    want = g.double().t() @ a.double()
    yard = T.rel_rms(g.t() @ a, want)
    need = l.gencomm_rows_wgrad_fixed_scratch_floats(rows, Co, Ci)
    outs, gd, ad = [], g.to(DEV), a.to(DEV)
    for _ in range(2):
        dw = torch.full((Co, Ci), float("nan"), dtype=torch.float32, device=DEV)
        scratch = torch.full((need,), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(l.gencomm_rows_wgrad_fixed(ptr(gd), ptr(ad), ptr(dw), rows, Co, Ci, ptr(scratch), need, stream_ptr(DEV)), "gencomm_rows_wgrad_fixed")
        torch.cuda.synchronize()
        outs.append(dw.cpu())
    e = T.rel_rms(outs[0], want)
    print(f"rows_wgrad_fixed: HIP rel rms {e:.3e}, float32 yardstick {yard:.3e}")
    assert e <= max(2.0 * yard, 1e-6) and torch.equal(outs[0], outs[1])
