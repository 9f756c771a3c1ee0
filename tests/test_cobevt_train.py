"""Training of the CoBEVT fusion, the parts that need no GPU: the float64 training restatement (tests/cobevt_train_restatement.py) against
the reference's stored float64 gradients (tests/golden/cobevt_train*.npz, made by tools/make_golden_cobevt_train.py), the opt-in
constructor, and the new entries of the C ABI. The HIP path is tested in test_gpu_cobevt_train.py."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import cobevt_restatement as R
import cobevt_train_restatement as TR
from helpers import GOLDEN, load_case
from gencomm_amd import CoBEVT, _lib, synth
from test_cobevt import load_cobevt_case

DOT_SEED = 4178     # tools/make_golden_cobevt_train.py
FULL = ("a", "b", "c", "e")


@functools.lru_cache(maxsize=None)
def load_golden():
    """The arrays of cobevt_train.npz and the files it lists, as one dictionary; arrays that were cut are joined again."""
    first = load_case("cobevt_train")
    rec = {}
    for name in json.loads(str(first["files"])):
        part = first if name == "cobevt_train.npz" else load_case(name[:-4])
        rec.update(part)
    cut = sorted({k.split(".part")[0] for k in rec if ".part" in k})
    for k in cut:
        n = len([1 for j in rec if j.startswith(k + ".part")])
        rec[k] = np.concatenate([rec.pop(f"{k}.part{j}") for j in range(n)]).reshape(tuple(rec[f"shape_{k}"]))
    return rec


def stored(rec, key, tag):
    """A stored float64 gradient: hi + lo."""
    return rec[f"{key}_hi_{tag}"].astype(np.float64) + rec[f"{key}_lo_{tag}"].astype(np.float64)


@functools.lru_cache(maxsize=None)
def restated_grads(tag):
    """(args, x, record_len, affine, g, seed, y64, dx64, {name: grad64}) of a fixture case, from the float64 restatement; computed once,
    shared (read only) by the tests of this file and of test_gpu_cobevt_train.py."""
    args, x, rl, aff, _, _, seed = load_cobevt_case(tag)
    g = load_golden()[f"g_{tag}"].astype(np.float32)
    m = CoBEVT(args).eval()
    synth.fill_params_(m, seed)
    y, dx, grads = TR.cobevt_grads(m.state_dict(), args, torch.from_numpy(x), rl, torch.from_numpy(aff), torch.from_numpy(g))
    return args, x, rl, aff, g, seed, y, dx, grads


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("tag", FULL)
def test_restatement_gradients_equal_the_reference(tag):
    rec = load_golden()
    args, x, rl, aff, g, seed, y, dx, grads = restated_grads(tag)
    names = json.loads(str(rec[f"names_{tag}"]))
    assert names == TR.param_names(CoBEVT(args).state_dict()) == list(grads)
    assert len(rec[f"yard_{tag}"]) == 1 + len(names)
    worst = rel(dx.numpy(), stored(rec, "dx", tag))
    assert worst <= 1e-10, (tag, "dx", worst)
    for i, k in enumerate(names):
        ref = stored(rec, f"p{i}", tag)
        assert ref.shape == tuple(grads[k].shape) and np.any(ref != 0), (tag, k)
        e = rel(grads[k].numpy(), ref)
        worst = max(worst, e)
        assert e <= 1e-10, (tag, k, e)
    print(f"case {tag}: float64 restatement against the reference's float64 gradients, worst relative rms {worst:.2e}")


def test_restatement_gradients_equal_the_reference_at_the_shipped_block():
    """Case d (C 256, depth 3): dx in full, the parameter gradients through their stored norms and dot products."""
    rec = load_golden()
    args, x, rl, aff, g, seed, y, dx, grads = restated_grads("d")
    names = json.loads(str(rec["names_d"]))
    assert names == list(grads) and len(names) == 70
    assert rel(dx.numpy(), stored(rec, "dx", "d")) <= 1e-10
    for i, k in enumerate(names):
        v = grads[k].numpy()
        norm, dot = float(rec["norm_d"][i]), float(rec["dot_d"][i])
        assert norm > 0
        assert abs(np.linalg.norm(v) - norm) <= 1e-10 * norm, (k, np.linalg.norm(v), norm)
        d = float((v * synth.noise_stream(DOT_SEED, i, v.shape).astype(np.float64)).sum())
        assert abs(d - dot) <= 1e-10 * abs(dot), (k, d, dot)


def test_fixture_files_are_small_and_yardsticks_are_sane():
    rec = load_golden()
    for name in json.loads(str(rec["files"])):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < (1 << 20), name
    for tag in R.CASES:
        yard = rec[f"yard_{tag}"]
        assert np.isfinite(yard).all() and yard.max() < 1e-5, (tag, yard.max())   # float32 against float64: a few 1e-7
        g = rec[f"g_{tag}"].astype(np.float32)
        c = R.CASES[tag]
        assert g.shape == (len(c["record_len"]), c["C"], c["H"], c["W"]) and np.abs(g).max() > 2.0


def test_trainable_constructor_keeps_the_state_dict_and_the_default_still_refuses():
    with open(os.path.join(GOLDEN, "cobevt_keys.json")) as f:
        spec = json.load(f)
    m = CoBEVT(spec["args"], trainable=True)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(got) == 76 and got == spec["state_dict"]
    assert m.trainable is True and CoBEVT(spec["args"]).trainable is False
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in CoBEVT(spec["args"]).named_parameters()]
    args = {"input_dim": 32, "mlp_dim": 32, "agent_size": 3, "window_size": 4, "dim_head": 16, "drop_out": 0.1, "depth": 1}
    x, aff = torch.zeros(2, 32, 8, 12), torch.from_numpy(R.make_affine([2], 3, 8, 12, 0))
    with pytest.raises(NotImplementedError, match="cobevt training"):
        CoBEVT(args).eval()(x, [2], aff)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="cobevt training"):
        CoBEVT(args).train()(x, [2], aff)
    with pytest.raises(_lib.GenCommHipError):          # trainable: no refusal, and no CPU fallback either
        CoBEVT(args, trainable=True).eval()(x, [2], aff)


def test_shell_constructs_a_trainable_cobevt():
    from test_cobevt import _shell_args
    from gencomm_amd.heter_model_baseline_w_gencomm_stage1 import HeterModelBaselineWGenCommStage1 as Shell
    m = Shell(_shell_args())
    assert isinstance(m.fusion_net, CoBEVT) and m.fusion_net.trainable


def test_new_entries_are_in_the_header_and_the_binding():
    with open(os.path.join(_lib.REPO_DIR, "include", "gencomm_hip.h")) as f:
        header = f.read()
    assert _lib.ABI_VERSION == 12 and re.search(r"#define GENCOMM_ABI_VERSION 12\b", header)
    for name in ("gencomm_swap_attn_train_fwd", "gencomm_swap_attn_bwd"):
        assert name in _lib._SIGNATURES, name
        assert re.search(r"\bint " + name + r"\(", header), name
    assert len(_lib._SIGNATURES["gencomm_swap_attn_train_fwd"][1]) == 14 and len(_lib._SIGNATURES["gencomm_swap_attn_bwd"][1]) == 17
    assert "ACCUMULATED" in header[header.index("gencomm_swap_attn_bwd "):header.index("int gencomm_swap_attn_fwd(")]


def test_library_rejects_unsupported_shapes_in_the_backward():
    _lib.build()
    l = _lib.lib()
    assert l.gencomm_swap_attn_bwd(*[None] * 8, 1, 2, 1, 16, 4, 8, 8, 0, None) == 1 and b"null pointer" in l.gencomm_last_error()
    assert l.gencomm_swap_attn_train_fwd(*[None] * 5, 1, 2, 1, 16, 4, 8, 8, 0, None) == 1 and b"null pointer" in l.gencomm_last_error()
    for dims, msg in (((1, 2, 1, 16, 16, 16, 16, 0), b"window_size must be 4 or 8"), ((1, 2, 1, 8, 4, 8, 8, 0), b"dim_head must be 16, 32 or 64"),
                      ((1, 9, 1, 16, 4, 8, 8, 0), b"must be 1..8"), ((1, 2, 1, 16, 4, 10, 8, 0), b"multiples of window_size"),
                      ((1, 2, 1, 16, 4, 8, 8, 2), b"grid_mode")):
        assert l.gencomm_swap_attn_bwd(*[1] * 8, *dims, None) == 1, dims
        assert msg in l.gencomm_last_error(), (dims, l.gencomm_last_error())
        assert l.gencomm_swap_attn_train_fwd(*[1] * 5, *dims, None) == 1, dims
