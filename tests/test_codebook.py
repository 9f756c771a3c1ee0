"""The CodeFilling codebook codec (gencomm_amd.UMGMQuantizer) without a GPU: the reference's state_dict, the restatement against the
reference's recorded float64 and float32 outputs (tests/golden/codebook.npz, tools/make_golden_codebook.py), the payload packing, the
refusals and the envelope errors. CPU only."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import codebook_restatement as R
from gencomm_amd import UMGMQuantizer, _lib

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codebook.npz"))


def _case(name):
    c, sd, x, u = R.case_data(name, int(GOLD[f"{name}/seed"]))
    keep = slice(None) if name != "bulk" else slice(0, c["n"], c["n"] // R.BULK_KEPT_ROWS)
    return c, sd, x, u, keep


def _module(c):
    return UMGMQuantizer(c["C"], c["m"], list(c["k"]), 0.0, R.components(c["C"]))


def _ok(got, ref):
    return bool(((got.double() - ref.double()).abs() <= 1e-5 + 1e-4 * ref.double().abs()).all())


@pytest.mark.parametrize("name", list(R.CASES))
def test_regenerated_data_is_the_fixtures(name):
    c, sd, x, u, _ = _case(name)
    assert R.checksum(sd.values()) == float(GOLD[f"{name}/checksum_params"])
    assert R.checksum([x]) == float(GOLD[f"{name}/checksum_x"])
    assert R.checksum(u) == float(GOLD[f"{name}/checksum_uniforms"])


@pytest.mark.parametrize("name", ["strict_a", "strict_b"])
def test_state_dict_keys_and_shapes(name):
    c = R.CASES[name]
    mod = _module(c)
    assert [f"{k} {list(v.shape)}" for k, v in mod.state_dict().items()] == list(GOLD[f"{name}/keys"])


def test_codebook_stays_tied_after_load():
    c, sd, _, _, _ = _case("strict_a")
    mod = _module(c)
    mod.load_state_dict(sd, strict=True)
    for i in range(len(c["k"])):
        a, b, d = mod._encoders[i]._quantizer._codebook, mod._encoders[i]._dequantizer._codebook, mod._decoders[i]._dequantizer._codebook
        assert a is b and b is d and torch.equal(a, sd[f"_encoders.{i}._quantizer._codebook"])
        assert isinstance(a, nn.Parameter)
    assert len(list(mod.parameters())) == len({id(p) for p in mod.parameters()})     # the tied codebook is listed once


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_the_reference(name):
    c, sd, x, u, keep = _case(name)
    L, clear = len(c["k"]), torch.from_numpy(GOLD[f"{name}/clear"])
    assert 1.0 - float(clear.double().mean()) == float(GOLD[f"{name}/excluded_share"]) <= (0.0 if name != "bulk" else R.MAX_EXCLUDED)
    r64 = R.umgm_forward(sd, x, c["m"], c["k"], u, torch.float64)
    assert torch.equal(R.clear_rows(r64["logits"], r64["y"], float(GOLD[f"{name}/logit_err32"])), clear)
    assert float((r64["restored"][keep] - torch.from_numpy(GOLD[f"{name}/restored64"])).abs().max()) < 1e-11
    assert abs(float(r64["loss"]) - float(GOLD[f"{name}/loss64"])) < 1e-12 * float(GOLD[f"{name}/loss64"])
    for l in range(L):
        assert np.array_equal(r64["codes"][l].numpy(), GOLD[f"{name}/codes64_{l}"]) and np.array_equal(r64["sampled"][l].numpy(), GOLD[f"{name}/sampled64_{l}"])
        assert float((r64["logits"][l][keep] - torch.from_numpy(GOLD[f"{name}/logits64_{l}"])).abs().max()) < 1e-10
    # float32: same decisions on every clear row (the reference's own float32 run took them too), values to float32 accuracy
    r32 = R.umgm_forward(sd, x, c["m"], c["k"], u, torch.float32)
    kept_clear = clear[keep]
    for l in range(L):
        for key in ("codes", "sampled"):
            assert np.array_equal(r32[key][l][clear].numpy(), GOLD[f"{name}/{key}32_{l}"][clear.numpy()])
            assert np.array_equal(GOLD[f"{name}/{key}32_{l}"][clear.numpy()], GOLD[f"{name}/{key}64_{l}"][clear.numpy()])
        assert _ok(r32["logits"][l][keep][kept_clear], torch.from_numpy(GOLD[f"{name}/logits32_{l}"])[kept_clear])
    assert _ok(r32["restored"][keep][kept_clear], torch.from_numpy(GOLD[f"{name}/restored32"])[kept_clear])
    # encode / decode
    enc = R.umgm_encode(sd, x, c["m"], c["k"], torch.float64)
    for l in range(L):
        assert np.array_equal(enc[l].numpy(), GOLD[f"{name}/encode64_{l}"])
    assert float((R.umgm_decode(sd, enc, c["m"], c["k"], torch.float64)[keep] - torch.from_numpy(GOLD[f"{name}/decode64"])).abs().max()) < 1e-11


def test_decode_of_encode_is_the_noise_free_forward():
    c, sd, x, _, _ = _case("strict_a")
    fwd = R.umgm_forward(sd, x, c["m"], c["k"], None, torch.float64)
    enc = R.umgm_encode(sd, x, c["m"], c["k"], torch.float64)
    same = torch.stack([(a == b).all(-1) for a, b in zip(enc, fwd["codes"])]).all(0)     # argmin(distance) = argmax(logit) off ties
    assert float(same.double().mean()) > 0.98
    assert torch.equal(R.umgm_decode(sd, enc, c["m"], c["k"], torch.float64)[same], fwd["restored"][same])


@pytest.mark.parametrize("name", ["strict_a", "strict_b"])
def test_pack_unpack_round_trip_and_payload_size(name):
    c = R.CASES[name]
    mod = _module(c)
    bits = sum(c["m"] * int(np.log2(k)) for k in c["k"])
    assert mod.payload_bits_per_row == bits and mod.payload_bytes_per_row == (bits + 7) // 8
    codes = [torch.from_numpy(GOLD[f"{name}/codes64_{l}"].astype(np.int64)) for l in range(len(c["k"]))]
    payload = mod.pack(codes)
    assert payload.dtype == torch.uint8 and list(payload.shape) == [c["n"], (bits + 7) // 8]
    for a, b in zip(mod.unpack(payload), codes):
        assert a.dtype == torch.int64 and torch.equal(a, b)
    # extreme values survive
    g = torch.Generator().manual_seed(3)
    rnd = [torch.randint(0, k, (50, c["m"]), generator=g) for k in c["k"]]
    rnd[0][0], rnd[-1][1] = 0, c["k"][-1] - 1
    for a, b in zip(mod.unpack(mod.pack(rnd)), rnd):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="payload must be uint8"):
        mod.unpack(payload[:, :-1])


def test_shipped_payload_is_24_bits():
    mod = _module(R.CASES["bulk"])
    assert mod.payload_bits_per_row == 24 and mod.payload_bytes_per_row == 3


def test_refusals():
    comp = R.components(64)
    with pytest.raises(NotImplementedError, match="permutationRate"):
        UMGMQuantizer(64, 2, [16], 0.1, comp)
    bad = dict(comp, sideHead=lambda: nn.Sequential(nn.Linear(64, 64)))
    with pytest.raises(NotImplementedError, match="'sideHead'"):
        UMGMQuantizer(64, 2, [16, 16], 0.0, bad)
    with pytest.raises(NotImplementedError, match="'quantizationHead'"):
        UMGMQuantizer(64, 2, [16], 0.0, dict(comp, quantizationHead=lambda: nn.Linear(64, 32)))
    UMGMQuantizer(64, 2, [16], 0.0, bad)                # one level has no side head: the factory is never called, as in the reference
    mod = UMGMQuantizer(64, 2, [16], 0.0, comp)
    with pytest.raises(NotImplementedError, match="codebook training"):
        mod(torch.zeros(4, 64))
    for p in mod.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="codebook training"):
        mod(torch.zeros(4, 64, requires_grad=True))
    with torch.no_grad():
        with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):
            mod(torch.zeros(4, 64))
        with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):
            mod.encode(torch.zeros(4, 64))


def test_envelope_errors_name_the_argument():
    comp = R.components(64)
    with pytest.raises(ValueError, match="channel 96"):
        UMGMQuantizer(96, 2, [16], 0.0, R.components(96))
    with pytest.raises(ValueError, match="m 3"):
        UMGMQuantizer(64, 3, [16], 0.0, comp)
    with pytest.raises(ValueError, match="k entry 8"):
        UMGMQuantizer(64, 2, [16, 8], 0.0, comp)
    with pytest.raises(ValueError, match="k entry 48"):
        UMGMQuantizer(64, 2, 48, 0.0, comp)
    with pytest.raises(ValueError, match="k entry 512"):
        UMGMQuantizer(64, 2, [512], 0.0, comp)
    with pytest.raises(ValueError, match="4 levels"):
        UMGMQuantizer(64, 2, [16] * 4, 0.0, comp)


def test_abi_argument_errors_are_status_codes():
    _lib.build()
    l = _lib.lib()
    k = lambda *v: (ctypes.c_int * len(v))(*v)
    assert l.gencomm_umgm_param_floats(128, 2, k(16, 16, 16), 3) == 16 * (128 * 128 + 128) + 2 * (128 * 128 + 128) + 3 * (16 * 128 + 4)
    for args, word in (((96, 2, k(16), 1), b"channel"), ((64, 3, k(16), 1), b"m must"), ((64, 2, k(16, 24), 2), b"k must"), ((64, 2, k(16), 0), b"levels"),
                       ((64, 2, k(16, 16, 16, 16), 4), b"levels")):
        assert l.gencomm_umgm_param_floats(*args) == -1 and word in l.gencomm_last_error(), args
    assert l.gencomm_umgm_workspace_bytes(0, 64) == -1 and l.gencomm_umgm_workspace_bytes(65, 64) == 8
    assert l.gencomm_umgm_fwd(None, None, None, None, 0, 0, None, None, None, None, None, 4, 0, 64, 2, k(16), 1, None, 0, None) == 1
    assert b"null pointer" in l.gencomm_last_error()
    assert l.gencomm_umgm_fwd(16, 16, None, None, 0, 3, 16, 16, None, None, 16, 4, 0, 64, 2, k(16), 1, None, 0, None) == 1 and b"noise must" in l.gencomm_last_error()
    assert l.gencomm_umgm_fwd(16, 16, None, None, 0, 1, 16, 16, None, None, 16, 4, 0, 64, 2, k(16), 1, None, 0, None) == 1 and b"uniforms" in l.gencomm_last_error()
    assert l.gencomm_umgm_fwd(16, 16, 16, None, 0, 0, 16, 16, None, None, 16, 4, 0, 64, 2, k(16), 1, None, 0, None) == 1 and b"keep" in l.gencomm_last_error()
    assert l.gencomm_umgm_fwd(16, 16, None, None, 0, 0, 16, 16, None, None, 16, 0, 0, 64, 2, k(16), 1, None, 0, None) == 1 and b"n must" in l.gencomm_last_error()
    assert l.gencomm_umgm_fwd(16, 20, None, None, 0, 0, 16, 16, None, None, 16, 4, 0, 64, 2, k(16), 1, None, 0, None) == 1 and b"aligned" in l.gencomm_last_error()
    assert l.gencomm_umgm_fwd(16, 16, None, None, 0, 0, 16, 16, None, None, 16, 4, 0, 64, 2, k(16), 1, None, 0, None) == 2 and b"workspace" in l.gencomm_last_error()
    assert l.gencomm_umgm_encode_fwd(16, None, 16, 4, 0, 64, 2, k(16), 1, None) == 1 and b"null pointer" in l.gencomm_last_error()
    assert l.gencomm_umgm_decode_fwd(16, 16, 16, 4, 0, 64, 5, k(16), 1, None) == 1 and b"m must" in l.gencomm_last_error()
    assert l.gencomm_umgm_noise_fwd(None, 1, 4, 2, k(16), 1, None) == 1 and b"out" in l.gencomm_last_error()
