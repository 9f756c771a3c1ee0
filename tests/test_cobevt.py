"""CoBEVT fusion (`fusion_method: cobevt`), the parts that need no GPU: checkpoint keys against the reference's
(tests/golden/cobevt_keys.json), the plain-torch restatement against the reference's own outputs (tests/golden/cobevt.npz, made by
tools/make_golden_cobevt.py), the shells, and the refusals. The HIP path is tested in test_gpu_cobevt.py."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import cobevt_restatement as R
from helpers import GOLDEN, assert_close, load_case
from gencomm_amd import CoBEVT, synth


def _keys():
    with open(os.path.join(GOLDEN, "cobevt_keys.json")) as f:
        return json.load(f)


def load_cobevt_case(tag):
    """(args, x float32, record_len, affine float64, y32, y64) of a fixture case; y64 = y32 - d64 (tools/make_golden_cobevt.py)."""
    g, g64 = load_case("cobevt"), load_case("cobevt_f64")
    y32 = g[f"y32_{tag}"]
    return (json.loads(str(g[f"args_{tag}"])), g[f"x_{tag}"].astype(np.float32), [int(v) for v in g[f"record_len_{tag}"]], g[f"affine_{tag}"],
            y32, y32.astype(np.float64) - g64[f"d64_{tag}"].astype(np.float64), int(g[f"seed_{tag}"]))


def test_state_dict_keys_order_and_shapes_match_the_reference():
    spec = _keys()
    m = CoBEVT(spec["args"])
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(got) == 76
    assert got == spec["state_dict"]
    # a reference-shaped checkpoint loads strictly, and the index buffer it carries is the one the kernel's arithmetic restates
    ckpt = {k: torch.zeros(shape, dtype=m.state_dict()[k].dtype) for k, shape in spec["state_dict"]}
    m.load_state_dict(ckpt, strict=True)
    att = CoBEVT(spec["args"]).layers[0].window_attention.fn
    assert att.relative_position_index.dtype == torch.int64
    assert torch.equal(att.relative_position_index, R.relative_position_index(5, 4))


@pytest.mark.parametrize("tag", list(R.CASES))
def test_restatement_reproduces_the_reference(tag):
    args, x, rl, aff, y32, y64, seed = load_cobevt_case(tag)
    assert args == R.case_args(R.CASES[tag]) and rl == R.CASES[tag]["record_len"]
    m = CoBEVT(args).eval()
    synth.fill_params_(m, seed)
    with torch.no_grad():
        got = R.cobevt_forward(m.state_dict(), args, torch.from_numpy(x), rl, torch.from_numpy(aff))
        got64 = R.cobevt_forward(m.state_dict(), args, torch.from_numpy(x).double(), rl, torch.from_numpy(aff))
    assert_close(got.numpy(), y32, 1e-5, 1e-6, f"restatement vs reference, case {tag}")
    assert_close(got64.numpy(), y64, 1e-9, 1e-9, f"float64 restatement vs the reference's float64 run, case {tag}")


def test_fixture_exercises_what_it_claims():
    for tag, c in R.CASES.items():
        _, x, rl, aff, y32, y64, _ = load_cobevt_case(tag)
        assert np.isfinite(y32).all() and x.min() == 0.0 and x.max() > 2.0
        assert y32.shape == (len(rl), c["C"], c["H"], c["W"]) and aff.shape == (len(rl), c["L"], c["L"], 2, 3)
        far = [abs(aff[b, 0, j, 0, 2]) > 0.8 for b, n in enumerate(rl) for j in range(1, n)]
        assert any(far), f"case {tag}: no agent is warped partly out of the map"
    assert min(R.CASES["b"]["record_len"]) == 1 and R.CASES["c"]["L"] * R.CASES["c"]["ws"] ** 2 == 320


def _shell_args():
    with open(os.path.join(GOLDEN, "shell_state_dict_keys.json")) as f:
        args = copy.deepcopy(json.load(f)["args"])
    args["fusion_method"] = "cobevt"
    args["cobevt"] = {"input_dim": 128, "mlp_dim": 128, "agent_size": 5, "window_size": 4, "dim_head": 32, "drop_out": 0.1, "depth": 1}
    return args


@pytest.mark.parametrize("core", ["heter_model_baseline_w_gencomm_stage1", "heter_model_baseline_w_gencomm_stage2"])
def test_shells_construct_with_cobevt(core):
    import importlib
    mod = importlib.import_module("gencomm_amd." + core)
    cls = [v for k, v in mod.__dict__.items() if k.lower() == core.replace("_", "")][-1]
    m = cls(_shell_args())
    assert isinstance(m.fusion_net, CoBEVT)
    keys = [k for k in m.state_dict() if k.startswith("fusion_net.")]
    assert len(keys) == 28 and "fusion_net.layers.0.grid_attention.fn.relative_position_bias_table.weight" in keys
    assert "fusion_net.mlp_head.3.bias" in keys


def test_refusals_name_their_cause():
    args = {"input_dim": 32, "mlp_dim": 32, "agent_size": 3, "window_size": 4, "dim_head": 16, "drop_out": 0.1, "depth": 1}
    with pytest.raises(ValueError, match="window_size 7"):
        CoBEVT(dict(args, window_size=7))
    with pytest.raises(ValueError, match="dim_head 8"):
        CoBEVT(dict(args, dim_head=8))
    m = CoBEVT(args).eval()
    x, aff = torch.zeros(2, 32, 8, 12), torch.from_numpy(R.make_affine([2], 3, 8, 12, 0))
    with pytest.raises(NotImplementedError, match="cobevt training"):       # parameters require grad, gradients are enabled
        m(x, [2], aff)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="cobevt training"):       # ... or the input does
        m(x.clone().requires_grad_(), [2], aff)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="drop_out"):
            m.train()(x, [2], aff)
        m.eval()
        with pytest.raises(ValueError, match="multiples of window_size"):
            m(torch.zeros(2, 32, 10, 12), [2], aff)
        with pytest.raises(ValueError, match="agent_size"):
            m(x, [2], torch.from_numpy(R.make_affine([2], 5, 8, 12, 0)))
        with pytest.raises(ValueError, match="record_len"):
            m(x, [3], aff)
        from gencomm_amd import _lib
        with pytest.raises(_lib.GenCommHipError):                             # everything in order, but a CPU tensor: no fallback
            m(x, [2], aff)


def test_library_rejects_unsupported_shapes_with_a_message():
    from gencomm_amd import _lib
    _lib.build()
    l = _lib.lib()
    ok = dict(B=1, L=2, heads=1, dh=16, ws=4, H=8, W=8, grid=0)

    def call(**kw):
        a = dict(ok, **kw)
        return l.gencomm_swap_attn_fwd(1, 1, 1, 1, a["B"], a["L"], a["heads"], a["dh"], a["ws"], a["H"], a["W"], a["grid"], None)
    assert l.gencomm_swap_attn_fwd(None, None, None, None, 1, 2, 1, 16, 4, 8, 8, 0, None) == 1 and b"null pointer" in l.gencomm_last_error()
    for kw, msg in (({"ws": 16}, b"window_size must be 4 or 8"), ({"dh": 8}, b"dim_head must be 16, 32 or 64"), ({"L": 9}, b"must be 1..8"),
                    ({"H": 10}, b"multiples of window_size"), ({"grid": 2}, b"grid_mode")):
        assert call(**kw) == 1, kw
        assert msg in l.gencomm_last_error(), (kw, l.gencomm_last_error())
