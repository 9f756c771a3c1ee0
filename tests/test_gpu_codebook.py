"""The fused CodeFilling codec kernel (gencomm_umgm_fwd and its encode / decode / noise entries) on the GPU.

Against the reference's float64 outputs (tests/golden/codebook.npz): restored rows and logits elementwise err <= 1e-5 + 1e-4 |ref|
(SURVEY 8c), codes and sampled indices exactly, on every clear row -- all rows of the strict cases --, and the loss on the strict
cases. Against the float64 restatement at the shapes where the kernel takes another path: a row tile is 64 rows (n = 1, 63, 65, 160),
C = 64 with m = 4 (d = 16), C = 256 with m = 1 (d = 256), k = 256, k per level, 1 and 2 levels. Those are strict cases by the fixture's recipe: a decision is clear
when its float64 top-2 gap is at least 16 x the restatement's own float32-against-float64 logit error, relative to the group's largest
|logit + gumbel|, measured here on the case, and the seed is the first under which every decision of every row is clear.
"""
import os

import numpy as np
import pytest
import torch

import codebook_restatement as R
from gencomm_amd import UMGMQuantizer

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebook.npz"))
DEV = torch.device("cuda:0")
_cache = {}


def _module(c, sd):
    mod = UMGMQuantizer(c["C"], c["m"], list(c["k"]), 0.0, R.components(c["C"]))
    mod.load_state_dict(sd, strict=True)
    return mod.to(DEV).eval()


def _worst(got, ref):
    ref = ref.double()
    return float(((got.double().cpu() - ref).abs() / (1e-5 + 1e-4 * ref.abs())).max()) if ref.numel() else 0.0


def _fixture(name):
    if name not in _cache:
        c, sd, x, u = R.case_data(name, int(GOLD[f"{name}/seed"]))
        _cache[name] = (c, sd, x, u, _module(c, sd))
    return _cache[name]


def _small(tag):
    """A case the fixture does not hold, with its float64 restatement (computed once, shared). As for the fixture's strict cases, the
    seed is the first under which every decision of every row is clear, so that nothing is left out of the comparison."""
    key = ("small", tag)
    if key not in _cache:
        c = dict(SMALL[tag], cb_scale=4.0, w_scale=2.0)
        for t in range(60):
            seed = 5000 + 1000 * list(SMALL).index(tag) + 3 * t
            sd = R.make_params(c["C"], c["m"], c["k"], seed, c["cb_scale"], c["w_scale"])
            x, u = R.make_x(c["n"], c["C"], seed + 1), R.make_uniforms(c["n"], c["m"], c["k"], seed + 2)
            r64, r32 = R.umgm_forward(sd, x, c["m"], c["k"], u, torch.float64), R.umgm_forward(sd, x, c["m"], c["k"], u, torch.float32)
            agree = torch.ones(c["n"], dtype=torch.bool)
            for l in range(len(c["k"])):
                agree &= ((r32["sampled"][l] == r64["sampled"][l]) & (r32["codes"][l] == r64["codes"][l])).all(-1)
            rel = 4 * 2.0 ** -23            # a handful of rows cannot measure it: never below the 4 ulp the reference shows at default init
            for l in range(len(c["k"])):
                e = ((r32["logits"][l].double() - r64["logits"][l]).abs() / r64["y"][l].abs().amax(-1, keepdim=True))[agree]
                rel = max(rel, float(e.max()) if e.numel() else 0.0)
            clear = R.clear_rows(r64["logits"], r64["y"], rel)
            if bool(clear.all()) and bool(agree.all()):
                break
        else:
            raise AssertionError(f"{tag}: no seed makes every decision clear")
        _cache[key] = (c, sd, x, u, r64, clear)
    return _cache[key]


SMALL = {
    "n1": dict(C=64, m=2, k=[16, 16, 16], n=1),
    "n63": dict(C=64, m=2, k=[16, 16, 16], n=63),
    "n65": dict(C=64, m=2, k=[16, 16, 16], n=65),
    "n160": dict(C=64, m=2, k=[16, 16, 16], n=160),
    "c64_m4_two_levels": dict(C=64, m=4, k=[16, 16], n=65),
    "c256_m1_one_level": dict(C=256, m=1, k=[16], n=70),
    "k256": dict(C=64, m=2, k=[256], n=65),
    "k_per_level": dict(C=128, m=2, k=[64, 16, 32], n=65),
}


def _compare(out, ref_restored, ref_codes, ref_sampled, ref_logits, clear, keep=slice(None)):
    restored, codes, logits, _, sampled = out
    assert float(clear.double().mean()) >= 1.0 - R.MAX_EXCLUDED
    kc = clear[keep]
    w = _worst(restored.cpu()[keep][kc], ref_restored[kc])
    print(f"restored: worst err / (1e-5 + 1e-4 |ref|) = {w:.4f} on {int(kc.sum())} rows")
    assert w <= 1.0
    for l in range(len(codes)):
        wl = _worst(logits[l].cpu()[keep][kc], ref_logits[l][kc])
        print(f"logits[{l}]: worst = {wl:.4f}")
        assert wl <= 1.0
        assert torch.equal(codes[l].cpu()[clear], ref_codes[l][clear]) and torch.equal(sampled[l].cpu()[clear], ref_sampled[l][clear])


@pytest.mark.parametrize("name", list(R.CASES))
def test_against_the_reference_float64(name):
    c, sd, x, u, mod = _fixture(name)
    L = len(c["k"])
    keep = slice(None) if name != "bulk" else slice(0, c["n"], c["n"] // R.BULK_KEPT_ROWS)
    clear = torch.from_numpy(GOLD[f"{name}/clear"])
    with torch.no_grad():
        out = mod(x.to(DEV), uniforms=[t.to(DEV) for t in u], return_sampled=True)
    _compare(out, torch.from_numpy(GOLD[f"{name}/restored64"]), [torch.from_numpy(GOLD[f"{name}/codes64_{l}"].astype(np.int64)) for l in range(L)],
             [torch.from_numpy(GOLD[f"{name}/sampled64_{l}"].astype(np.int64)) for l in range(L)],
             [torch.from_numpy(GOLD[f"{name}/logits64_{l}"]) for l in range(L)], clear, keep)
    if name != "bulk":
        assert bool(clear.all())
        ref = float(GOLD[f"{name}/loss64"])
        print(f"loss {float(out[3]):.8f} reference {ref:.8f}")
        assert abs(float(out[3]) - ref) <= 1e-5 + 1e-4 * abs(ref)
    assert out[0].dtype == torch.float32 and out[1][0].dtype == torch.int64 and list(out[2][0].shape) == [c["n"], c["m"], c["k"][0]]


@pytest.mark.parametrize("tag", list(SMALL))
def test_against_the_restatement_float64(tag):
    c, sd, x, u, r64, clear = _small(tag)
    mod = _module(c, sd)
    with torch.no_grad():
        out = mod(x.to(DEV), uniforms=[t.to(DEV) for t in u], return_sampled=True)
    _compare(out, r64["restored"], r64["codes"], r64["sampled"], r64["logits"], clear)
    own = float(((out[0].double().cpu() - x.double()) ** 2).mean())           # the loss is the kernel's own rows', flipped or not
    assert abs(float(out[3]) - own) <= 1e-5 + 1e-4 * own
    if bool(clear.all()):
        assert abs(float(out[3]) - float(r64["loss"])) <= 1e-5 + 1e-4 * float(r64["loss"])


def _map_case():
    c = dict(C=64, m=2, k=[16, 32, 16])
    sd = R.make_params(c["C"], c["m"], c["k"], 6100)          # default initialisation: the noise decides many samples
    A, H, W = 3, 13, 17
    x = R.make_x(A * H * W, c["C"], 6101)
    u = R.make_uniforms(A * H * W, c["m"], c["k"], 6102)
    return c, sd, A, H, W, x, u, _module(c, sd)


def test_nchw_entry_is_the_rows_entry_bit_for_bit():
    c, sd, A, H, W, x, u, mod = _map_case()
    xm = x.view(A, H * W, c["C"]).permute(0, 2, 1).reshape(A, c["C"], H, W).contiguous()
    ud = [t.to(DEV) for t in u]
    with torch.no_grad():
        rows = mod(x.to(DEV), uniforms=ud)
        maps = mod.forward_map(xm.to(DEV), uniforms=ud, return_logits=True)
        plain = mod.forward_map(xm.to(DEV), uniforms=ud)
    assert list(maps[0].shape) == [A, c["C"], H, W] and plain[2] is None
    back = maps[0].view(A, c["C"], H * W).permute(0, 2, 1).reshape(A * H * W, c["C"])
    assert torch.equal(back, rows[0]) and torch.equal(maps[3], rows[3]) and torch.equal(plain[0], maps[0]) and torch.equal(plain[3], rows[3])
    for l in range(len(c["k"])):
        assert torch.equal(maps[1][l], rows[1][l]) and torch.equal(maps[2][l], rows[2][l]) and torch.equal(plain[1][l], rows[1][l])


def test_pass_through_agent_keeps_its_input_and_the_loss():
    c, sd, A, H, W, x, u, mod = _map_case()
    xm = x.view(A, H * W, c["C"]).permute(0, 2, 1).reshape(A, c["C"], H, W).contiguous().to(DEV)
    ud = [t.to(DEV) for t in u]
    with torch.no_grad():
        plain = mod.forward_map(xm, uniforms=ud)
        kept = mod.forward_map(xm, keep=[False, True, False], uniforms=ud)
    assert torch.equal(kept[0][1], xm[1]) and torch.equal(kept[0][0], plain[0][0]) and torch.equal(kept[0][2], plain[0][2])
    assert not torch.equal(plain[0][1], xm[1]) and torch.equal(kept[3], plain[3])
    for l in range(len(c["k"])):
        assert torch.equal(kept[1][l], plain[1][l])


def test_exact_tie_resolves_to_the_lower_index():
    c = dict(C=64, m=2, k=[16, 16])
    sd = R.make_params(c["C"], c["m"], c["k"], 6200, 4.0, 2.0)
    for i in range(2):
        cb = sd[f"_encoders.{i}._quantizer._codebook"]
        cb[:, 9] = cb[:, 3]                      # two identical codewords (the three keys share the tensor); 9 sits in another wave's range
        cb[:, 2] = cb[:, 1]                      # ... and a pair inside one wave's range
    x = R.make_x(200, c["C"], 6201)
    ref = R.umgm_forward(sd, x, c["m"], c["k"], None, torch.float64)
    mod = _module(c, sd)
    with torch.no_grad():
        out = mod(x.to(DEV), noise=False, return_sampled=True)
        enc = mod.encode(x.to(DEV))
    for l in range(2):
        got = out[1][l].cpu()
        assert not bool(((got == 9) | (got == 2)).any()) and bool((got == 3).any()) and bool((got == 1).any())
        assert torch.equal(out[4][l], out[1][l])                       # no noise: the sampled index is the code
        e = enc[l].cpu()
        assert not bool(((e == 9) | (e == 2)).any()) and bool((e == 3).any())
    assert torch.equal(out[1][0].cpu(), ref["codes"][0]) or float((out[1][0].cpu() == ref["codes"][0]).double().mean()) > 0.98


def test_two_runs_are_bit_identical():
    c, sd, A, H, W, x, u, mod = _map_case()
    xd = x.to(DEV)
    with torch.no_grad():
        a, b = mod(xd, seed=77, return_sampled=True), mod(xd, seed=77, return_sampled=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    for l in range(len(c["k"])):
        assert torch.equal(a[1][l], b[1][l]) and torch.equal(a[2][l], b[2][l]) and torch.equal(a[4][l], b[4][l])


def test_philox_run_replays_from_its_exported_field_and_seeds_differ():
    c, sd, A, H, W, x, u, mod = _map_case()
    xd = x.to(DEV)
    with torch.no_grad():
        a = mod(xd, seed=1234, return_sampled=True)
        field = mod.philox_uniforms(1234, xd.shape[0])
        b = mod(xd, uniforms=field, return_sampled=True)
        other = mod(xd, seed=1235, return_sampled=True)
        torch.manual_seed(5)
        d1 = mod(xd, return_sampled=True)
        torch.manual_seed(5)
        d2 = mod(xd, return_sampled=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    for l in range(len(c["k"])):
        assert torch.equal(a[1][l], b[1][l]) and torch.equal(a[2][l], b[2][l]) and torch.equal(a[4][l], b[4][l])
        assert list(field[l].shape) == [xd.shape[0], c["m"], c["k"][l]]
    assert any(not torch.equal(a[4][l], a[1][l]) for l in range(len(c["k"])))         # the noise decides some samples
    assert any(not torch.equal(a[4][l], other[4][l]) for l in range(len(c["k"]))) and not torch.equal(a[0], other[0])
    assert torch.equal(d1[0], d2[0])                                                  # the default seed comes from torch's generator


def test_exported_field_is_uniform_and_does_not_depend_on_n():
    mod = _module(dict(C=64, m=2, k=[32]), R.make_params(64, 2, [32], 6300))
    u = mod.philox_uniforms(99, 1024)[0].double().cpu().reshape(-1)
    N = u.numel()
    assert N == 1 << 16 and float(u.min()) > 0.0 and float(u.max()) < 1.0
    mean, var = float(u.mean()), float(((u - 0.5) ** 2).mean())
    print(f"mean {mean:.6f} var {var:.6f}")
    assert abs(mean - 0.5) <= 5 * (1 / 12 / N) ** 0.5
    assert abs(var - 1 / 12) <= 5 * ((1 / 80 - 1 / 144) / N) ** 0.5
    # the same rows draw the same numbers whatever n (and the tiling) is
    c, sd, A, H, W, x, _, mod3 = _map_case()
    big, small = mod3.philox_uniforms(7, 160), mod3.philox_uniforms(7, 37)
    for l in range(len(c["k"])):
        assert torch.equal(big[l][:37], small[l])
    with torch.no_grad():
        a, b = mod3(x[:160].to(DEV), seed=7, return_sampled=True), mod3(x[:37].to(DEV), seed=7, return_sampled=True)
    assert torch.equal(a[0][:37], b[0])
    for l in range(len(c["k"])):
        assert torch.equal(a[4][l][:37], b[4][l]) and torch.equal(a[2][l][:37], b[2][l])


@pytest.mark.parametrize("name", ["strict_a", "strict_b", "bulk"])
def test_encode_decode_pack_against_the_fixture(name):
    c, sd, x, u, mod = _fixture(name)
    L = len(c["k"])
    keep = slice(None) if name != "bulk" else slice(0, c["n"], c["n"] // R.BULK_KEPT_ROWS)
    ref = [torch.from_numpy(GOLD[f"{name}/encode64_{l}"].astype(np.int64)) for l in range(L)]
    with torch.no_grad():
        enc = mod.encode(x.to(DEV))
        dec = mod.decode([t.to(DEV) for t in ref])
        fwd = mod(x.to(DEV), noise=False)
        again = mod.decode(enc)
    # the encode path's own near ties: the distances of the float64 restatement, the margin of the fixture
    sdd = {k: v.double() for k, v in sd.items()}
    clear, xx = torch.ones(c["n"], dtype=torch.bool), x.double()
    for i, k in enumerate(c["k"]):
        z = R._lin(sdd, f"_encoders.{i}._latentStageEncoder", xx)
        dist, _ = R._logits(sdd, i, R._lin(sdd, f"_encoders.{i}._quantizationHead", z), c["m"], k)
        clear &= (R.top2_gap(-dist) >= R.CLEAR_FACTOR * float(GOLD[f"{name}/logit_err32"]) * dist.abs().amax(-1)).all(-1)
        if i < L - 1:
            cb = sdd[f"_encoders.{i}._quantizer._codebook"]
            xx = R._lin(sdd, f"_encoders.{i}._latentHead", z) - cb[torch.arange(c["m"]).expand_as(ref[i]), ref[i]].reshape(c["n"], -1)
    assert float(clear.double().mean()) >= 1.0 - R.MAX_EXCLUDED
    for l in range(L):
        assert torch.equal(enc[l].cpu()[clear], ref[l][clear])
    assert _worst(dec.cpu()[keep], torch.from_numpy(GOLD[f"{name}/decode64"])) <= 1.0
    same = torch.stack([(a == b).all(-1) for a, b in zip(enc, fwd[1])]).all(0)
    assert float(same.double().mean()) > 0.98 and torch.equal(again[same], fwd[0][same])      # decode(encode(x)) is the noise-free forward
    payload = mod.pack(enc)
    assert payload.is_cuda and list(payload.shape) == [c["n"], mod.payload_bytes_per_row]
    assert torch.equal(payload.cpu(), mod.pack([t.cpu() for t in enc]))
    for a, b in zip(mod.unpack(payload), enc):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="outside the codebook"):
        mod.decode([t + (c["k"][0] if i == 0 else 0) for i, t in enumerate(enc)])


def test_grad_enabled_call_raises():
    c, sd, x, u, mod = _fixture("strict_a")
    with pytest.raises(NotImplementedError, match="codebook training"):
        mod(x.to(DEV))
    with pytest.raises(NotImplementedError, match="codebook training"):
        mod.forward_map(torch.zeros(1, c["C"], 4, 4, device=DEV))
