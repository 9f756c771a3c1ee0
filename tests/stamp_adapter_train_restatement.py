"""Autograd of the restated STAMP adapter / reverter (tests/stamp_adapter_restatement.py, imported unmodified) in any dtype: the float64
truth and the float32 yardstick of the backward tests, the gradient criterion, and the adapter-training step objective
(opencood/loss/adapter_loss.py:41-45 with the shipped yamls' alphas).

Criterion (the project's own for gradients, tests/test_gpu_codebook_train.py): per tensor, relative rms error against float64
``<= max(2 x the float32 yardstick, 1e-6)``; an all-zero truth demands exact zeros; no tensor is left out.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import stamp_adapter_restatement as R

ORDER = ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias", "gamma")
ALPHA = dict(alpha_P2M=9.0, alpha_M2P2M=1.0, alpha_M2P=10.0)    # loss_adapter.args of the shipped yamls
FLOOR = 1e-6
TRAIN_CASES = ("cnx64", "cnx128", "rev64", "conv")


def load_fixture(name):
    """tests/golden/stamp_adapter_train_<name>_<i>.npz merged into one dict (a case is split so that no file outgrows the largest
    committed fixture)."""
    import glob
    import os
    parts = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"stamp_adapter_train_{name}_*.npz")))
    assert parts, f"no fixture for case {name}"
    out = {}
    for f in parts:
        with np.load(f) as z:
            for k in z.files:
                assert k not in out, k
                out[k] = z[k]
    return out


def rel_rms(got, ref64):
    ref64 = ref64.double()
    den = float(ref64.pow(2).mean().sqrt())
    err = float((got.double() - ref64).pow(2).mean().sqrt())
    return err / den if den > 0 else (0.0 if err == 0 else float("inf"))


def check(name, got, ref64, yard):
    """Assert the criterion for one tensor; returns the relative rms error."""
    if float(ref64.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, f"{name}: the truth is all zero, the result is not"
        return 0.0
    e = rel_rms(got, ref64)
    bound = max(2.0 * yard, FLOOR)
    assert e <= bound, f"{name}: rel rms {e:.3e} > {bound:.3e} (float32 yardstick {yard:.3e})"
    return e


DIGEST_ABOVE = 16384    # a fixture stores a gradient with more elements than this (other than the input's) as a digest


def digest_vectors(numel, seed, index):
    """The two seeded normal vectors of the digest of tensor number `index` (sorted key order) of the fixture with `seed`."""
    rng = np.random.default_rng([seed, index, 77])
    return torch.from_numpy(rng.normal(0.0, 1.0, (2, numel)))


def digest(t, seed, index):
    """[sum, sum of squares, <t, v1>, <t, v2>] in float64."""
    t = t.double().reshape(-1)
    v = digest_vectors(t.numel(), seed, index)
    return np.array([float(t.sum()), float(t.pow(2).sum()), float(t @ v[0]), float(t @ v[1])], dtype=np.float64)


def check_digest(name, got, ref_digest, yard, seed, index):
    """The criterion on a digest. With d = got - ref and ||d|| <= b ||ref|| (b = max(2 yard, 1e-6), ||ref|| from the stored sum of
    squares): |sum d| <= sqrt(N) ||d|| and | ||got||^2 - ||ref||^2 | = |<d, got + ref>| <= ||d|| (2 ||ref|| + ||d||) by Cauchy-Schwarz
    (necessary conditions); <d, v> for a normal vector v independent of d has standard deviation ||d||, so |<d, v>| <= 3 b ||ref|| is
    asked of both projections (three standard deviations; a single wrong element of relative size 1e-3 in a 65 536-element matrix moves a
    projection by ~1e-3 |v_i| |ref_i| against a bound of 3e-6 * 256 rms(ref): it fails). Returns the larger |<d, v>| / ||ref||."""
    numel = got.numel()
    got = digest(got, seed, index)
    b = max(2.0 * yard, FLOOR)
    norm = float(np.sqrt(ref_digest[1]))
    assert norm > 0.0, name
    d = np.abs(got - ref_digest)
    assert d[0] <= np.sqrt(numel) * b * norm, f"{name}: sum {got[0]:.9e} against {ref_digest[0]:.9e}"
    assert d[1] <= b * norm * (2.0 * norm + b * norm), f"{name}: sum of squares {got[1]:.9e} against {ref_digest[1]:.9e}"
    proj = max(d[2], d[3]) / norm
    assert proj <= 3.0 * b, f"{name}: projection error {proj:.3e} > {3.0 * b:.3e}"
    return proj


def block_grads(p, x, dy, dtype):
    """{name: gradient} of sum(block(x) * dy) for x ("x") and every parameter of one restated block (gamma may be None)."""
    q = {k: (None if v is None else v.to(dtype).clone().requires_grad_(True)) for k, v in p.items()}
    xx = x.to(dtype).clone().requires_grad_(True)
    (R.convnext_block(q, xx) * dy.to(dtype)).sum().backward()
    out = {"x": xx.grad}
    out.update({k: v.grad for k, v in q.items() if v is not None})
    return out


def trained(sd):
    """The keys of a state_dict that a forward reaches (``smoothing`` is created and never used)."""
    return [k for k in sd if ".smoothing." not in k]


def module_grads(cfg, sd, prefix, x, G, dtype, x_grad=True):
    """Gradients of sum(module(x) * G): {"x": .., key: ..} over the trained keys."""
    q = {k: v.to(dtype).clone().requires_grad_(k in trained(sd)) for k, v in sd.items()}
    xx = x.to(dtype).clone().requires_grad_(x_grad)
    (R.adapter_forward(cfg, q, prefix, xx) * G.to(dtype)).sum().backward()
    out = {k: q[k].grad for k in trained(sd)}
    if x_grad:
        out["x"] = xx.grad
    return out


def make_G(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(0.0, 1.0, shape).astype(np.float32))


def step_loss(cfg_a, sd_a, cfg_r, sd_r, FM, FP, dtype):
    """adapter_loss of one adapter-training step: 9 mse(FM, R(FP)) + 1 mse(FM, R(A(FM))) + 10 mse(FP, A(FM))."""
    FM, FP = FM.to(dtype), FP.to(dtype)
    FM2P = R.adapter_forward(cfg_a, sd_a, "adapter", FM)
    FP2M = R.adapter_forward(cfg_r, sd_r, "reverter", FP)
    FM2P2M = R.adapter_forward(cfg_r, sd_r, "reverter", FM2P)
    return ALPHA["alpha_P2M"] * F.mse_loss(FP2M, FM) + ALPHA["alpha_M2P2M"] * F.mse_loss(FM2P2M, FM) + ALPHA["alpha_M2P"] * F.mse_loss(FM2P, FP)


def step_data(seed):
    """(adapter cfg, its params (STD), reverter cfg, its params (STD_CHAIN), FM, FP [2, 128, 12, 20])."""
    cfg_a, sd_a, cfg_r, sd_r, FM = R.chain_data(seed, seed + 7)
    return cfg_a, sd_a, cfg_r, sd_r, FM, R.make_x(tuple(FM.shape), seed + 13)


def step_grads(data, dtype):
    """(loss, {key: gradient}) of the step objective over the trained keys of both modules."""
    cfg_a, sd_a, cfg_r, sd_r, FM, FP = data
    qa = {k: v.to(dtype).clone().requires_grad_(k in trained(sd_a)) for k, v in sd_a.items()}
    qr = {k: v.to(dtype).clone().requires_grad_(k in trained(sd_r)) for k, v in sd_r.items()}
    loss = step_loss(cfg_a, qa, cfg_r, qr, FM, FP, dtype)
    loss.backward()
    grads = {k: qa[k].grad for k in trained(sd_a)}
    grads.update({k: qr[k].grad for k in trained(sd_r)})
    return float(loss.detach()), grads


def sgd_step(data, grads, lr, dtype):
    """The loss after one SGD step of size lr on the trained keys."""
    cfg_a, sd_a, cfg_r, sd_r, FM, FP = data
    with torch.no_grad():
        na = {k: v.to(dtype) - (lr * grads[k].to(dtype) if k in grads else 0) for k, v in sd_a.items()}
        nr = {k: v.to(dtype) - (lr * grads[k].to(dtype) if k in grads else 0) for k, v in sd_r.items()}
        return float(step_loss(cfg_a, na, cfg_r, nr, FM, FP, dtype))
