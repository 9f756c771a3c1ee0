"""Training the CodeFilling codec, the parts that need no GPU: the fixture tests/golden/codebook_train.npz (gradients of the reference's
own UMGMQuantizer, tools/make_golden_codebook_train.py) against the float64 training restatement, the ``trainable=`` keyword, and the
new ABI entries' declarations and argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import codebook_restatement as R
import codebook_train_restatement as T
from gencomm_amd import UMGMQuantizer, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "codebook_train.npz"))
NEW_ENTRIES = ("gencomm_umgm_bwd_workspace_bytes", "gencomm_umgm_bwd", "gencomm_rows_wgrad_fixed_scratch_floats", "gencomm_rows_wgrad_fixed")


def _forced(name):
    return [torch.from_numpy(GOLD[f"{name}/sampled64_{l}"].astype(np.int64)) for l in range(len(T.CASES[name]["k"]))]


@pytest.mark.parametrize("name", list(T.CASES))
def test_regenerated_data_is_the_fixtures(name):
    c, sd, x, u, G = T.case_data(name, int(GOLD[f"{name}/seed"]))
    assert R.checksum(sd.values()) == float(GOLD[f"{name}/checksum_params"])
    assert R.checksum([x]) == float(GOLD[f"{name}/checksum_x"])
    assert R.checksum(u) == float(GOLD[f"{name}/checksum_uniforms"])
    assert R.checksum([G]) == float(GOLD[f"{name}/checksum_G"])


@pytest.mark.parametrize("name", list(T.CASES))
def test_restatement_gradients_are_the_references(name):
    """float64 restatement against the reference's float64 gradients: every stored element to 1e-10 of the tensor's maximum, and the
    two whole-tensor sums. The soft case forces the reference's sampled indices; the strict cases decide for themselves and must
    arrive at the same ones."""
    c, sd, x, u, G = T.case_data(name, int(GOLD[f"{name}/seed"]))
    strict = name in T.STRICT
    g64, out = T.gradients(sd, x, c["m"], c["k"], u, None if strict else _forced(name), G, T.LOSS_WEIGHT, torch.float64)
    for l, s in enumerate(_forced(name)):
        assert torch.equal(out["sampled"][l], s)
    assert abs(float(out["loss"].detach()) - float(GOLD[f"{name}/loss64"])) <= 1e-12 * max(1.0, float(GOLD[f"{name}/loss64"]))
    keys = list(GOLD[f"{name}/keys"])
    assert sorted(keys) == sorted(T.param_keys(sd) + ["x"])
    for key in keys:
        got, ref = T.subsample(g64[key]), torch.from_numpy(GOLD[f"{name}/grad64/{key}"])
        top = max(float(g64[key].abs().max()), 1e-300)
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-10 * top, key
        sumsq = float((g64[key] ** 2).sum())
        assert abs(float(g64[key].sum()) - float(GOLD[f"{name}/sum64/{key}"])) <= 1e-10 * top * g64[key].numel(), key
        assert abs(sumsq - float(GOLD[f"{name}/sumsq64/{key}"])) <= 1e-9 * max(sumsq, 1e-300), key


def test_lower_bound_rule_of_the_restatement():
    t, bound = torch.tensor([[1e-7], [1.0]], dtype=torch.float64, requires_grad=True), torch.tensor([1e-6], dtype=torch.float64)
    for sign, want in ((-1.0, [-1.0, -1.0]), (1.0, [0.0, 1.0])):       # below the bound: passes only a negative gradient
        (g,) = torch.autograd.grad((T._LowerBound.apply(t, bound) * sign).sum(), t)
        assert g.reshape(-1).tolist() == want


def test_trainable_keyword():
    comp = R.components(64)
    x = torch.zeros(4, 64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="codebook training is not implemented"):
        UMGMQuantizer(64, 2, [16], 0.0, comp)(x)
    mod = UMGMQuantizer(64, 2, [16], 0.0, comp, trainable=True)
    assert mod.trainable is True and UMGMQuantizer(64, 2, [16], 0.0, comp).trainable is False
    with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):
        mod(x)
    with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):
        mod.forward_map(torch.zeros(1, 64, 2, 2, requires_grad=True))
    with pytest.raises(NotImplementedError, match="permutationRate"):
        UMGMQuantizer(64, 2, [16], 0.1, comp, trainable=True)


def test_state_dict_is_unchanged_by_trainable():
    comp = R.components(64)
    a, b = UMGMQuantizer(64, 2, [16, 16], 0.0, comp), UMGMQuantizer(64, 2, [16, 16], 0.0, comp, trainable=True)
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    assert [k for k, _ in a.named_parameters()] == [k for k, _ in b.named_parameters()]


def test_header_and_signatures_agree_on_the_new_entries():
    header = open(os.path.join(os.path.dirname(HERE), "include", "gencomm_hip.h")).read()
    for name in NEW_ENTRIES:
        decl = re.search(r"\b(?:int|long long)\s+" + name + r"\(([^;]*)\);", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 12


def test_abi_argument_errors_are_status_codes():
    _lib.build()
    l = _lib.lib()
    k = lambda *v: (ctypes.c_int * len(v))(*v)
    err = l.gencomm_last_error
    assert l.gencomm_umgm_bwd_workspace_bytes(0, 64, 2, k(16), 1) == -1 and b"rows" in err()
    assert l.gencomm_umgm_bwd_workspace_bytes(64, 96, 2, k(16), 1) == -1 and b"channel" in err()
    assert l.gencomm_umgm_bwd_workspace_bytes(64, 64, 2, k(16), 1) > 0

    def bwd(params=16, x=16, keep=None, u=None, noise=0, sampled=16, dr=None, dl=None, dx=16, dp=16, dx_only=0, n=4, HW=0, C=64, m=2, ws=None, wsb=0):
        return l.gencomm_umgm_bwd(params, x, keep, u, 0, noise, sampled, dr, dl, dx, dp, dx_only, n, HW, C, m, k(16), 1, ws, wsb, None)

    assert bwd(params=None) == 1 and b"params" in err()
    assert bwd(sampled=None) == 1 and b"sampled" in err()
    assert bwd(dx=None) == 1 and b"dx" in err()
    assert bwd(dp=None) == 1 and b"dparams" in err()
    assert bwd(dx_only=2) == 1 and b"dx_only" in err()
    assert bwd(noise=3) == 1 and b"noise must" in err()
    assert bwd(noise=1) == 1 and b"uniforms" in err()
    assert bwd(keep=16) == 1 and b"keep" in err()
    assert bwd(n=0) == 1 and b"n must" in err()
    assert bwd(x=20) == 1 and b"aligned" in err()
    assert bwd(m=3) == 1 and b"m must" in err()
    assert bwd() == 2 and b"workspace" in err()
    assert bwd(dp=None, dx_only=1) == 2 and b"workspace" in err()
    assert l.gencomm_rows_wgrad_fixed_scratch_floats(0, 64, 64) == -1 and b"rows" in err()
    assert l.gencomm_rows_wgrad_fixed_scratch_floats(100, 64, 128) == 4 * 64 * 128            # one workgroup of 4 row ranges
    assert l.gencomm_rows_wgrad_fixed_scratch_floats(100000, 64, 64) == 64 * 64 * 64          # 16 workgroups at the most
    assert l.gencomm_rows_wgrad_fixed(None, 16, 16, 4, 64, 64, 16, 1 << 20, None) == 1 and b"null pointer" in err()
    assert l.gencomm_rows_wgrad_fixed(16, 16, 16, 0, 64, 64, 16, 1 << 20, None) == 1 and b"rows" in err()
    assert l.gencomm_rows_wgrad_fixed(16, 16, 16, 4, 96, 64, 16, 1 << 20, None) == 1 and b"Co" in err()
    assert l.gencomm_rows_wgrad_fixed(16, 16, 16, 4, 64, 32, 16, 1 << 20, None) == 1 and b"Ci" in err()
    assert l.gencomm_rows_wgrad_fixed(16, 16, 16, 4, 64, 64, 16, 10, None) == 2 and b"scratch" in err()
