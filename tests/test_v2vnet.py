"""V2VNet fusion (`gencomm_amd.V2VNetFusion`), the parts that need no GPU: checkpoint keys against the reference's
(tests/golden/v2vnet_keys.json), the decomposed restatement against the reference's own float64 outputs (tests/golden/v2vnet.npz, made by
tools/make_golden_v2vnet.py) -- which pins the three equivalences the HIP path is built on --, the refusals, and the three new entries of
the C ABI. The HIP path is tested in test_gpu_v2vnet.py."""
import json
import os

import numpy as np
import pytest
import torch

import v2vnet_restatement as R
from helpers import GOLDEN, load_case


def _keys():
    with open(os.path.join(GOLDEN, "v2vnet_keys.json")) as f:
        return json.load(f)


_FIXTURE = {}


def load_v2vnet_case(tag):
    """(args, state dict, x float32, record_len, affine float64, out32, out64, reference rel rms, reference max abs) of a fixture case."""
    if not _FIXTURE:
        _FIXTURE.update(load_case("v2vnet"))
    g, c = _FIXTURE, R.CASES[tag]
    sd = {k.split("/", 1)[1]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"w_{tag}/")}
    return (R.case_args(c), sd, g[f"x_{c['data']}"], [int(v) for v in g["record_len"]], g[f"affine_{c['data']}"], g[f"out32_{tag}"], g[f"out64_{tag}"],
            float(g[f"ref_rel_rms_{tag}"]), float(g[f"ref_max_abs_{tag}"]))


def test_state_dict_keys_order_and_shapes_match_the_reference():
    from gencomm_amd import V2VNetFusion
    spec = _keys()
    m = V2VNetFusion(spec["args"])
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == spec["state_dict"]
    assert [k for k, _ in got] == ["msg_cnn.weight", "msg_cnn.bias", "conv_gru.cell_list.0.conv_gates.weight", "conv_gru.cell_list.0.conv_gates.bias",
                                   "conv_gru.cell_list.0.conv_can.weight", "conv_gru.cell_list.0.conv_can.bias", "mlp.weight", "mlp.bias"]
    # full shapes: the hidden-state columns and the reset-gate rows are there although the forward never reads them
    assert dict(map(tuple, ((k, tuple(s)) for k, s in got)))["conv_gru.cell_list.0.conv_gates.weight"] == (512, 768, 3, 3)


def test_reference_shaped_checkpoint_loads_strictly():
    from gencomm_amd import V2VNetFusion
    spec = _keys()
    m = V2VNetFusion(spec["args"])
    m.load_state_dict({k: torch.zeros(shape) for k, shape in spec["state_dict"]}, strict=True)
    for tag in R.CASES:     # ... and so do the fixture's own weights, two GRU layers included
        args, sd = load_v2vnet_case(tag)[:2]
        V2VNetFusion(args).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_restatement_reproduces_the_reference_in_float64(tag):
    """The decomposed algorithm (split msg_cnn, zero-state GRU cell, ego-only last round) against the reference's float64 run: 1e-12
    relative rms (measured: 5.6e-17 absolute on values of 0.2). The undecomposed loop agrees too."""
    args, sd, x, rl, aff, _, out64, _, _ = load_v2vnet_case(tag)
    with torch.no_grad():
        got = R.v2vnet_forward(sd, args, torch.from_numpy(x).double(), rl, torch.from_numpy(aff)).numpy()
        loop = R.v2vnet_loop_forward(sd, args, torch.from_numpy(x).double(), rl, torch.from_numpy(aff)).numpy()
    assert got.shape == out64.shape == (len(rl), args["in_channels"], args["conv_gru"]["H"], args["conv_gru"]["W"])
    print(f"case {tag}: decomposed vs reference float64: rel rms {R.rel_rms(got, out64):.2e}, max abs {np.abs(got - out64).max():.2e}")
    assert R.rel_rms(got, out64) <= 1e-12
    assert R.rel_rms(loop, out64) <= 1e-12


def test_fixture_exercises_what_it_claims():
    g = load_case("v2vnet")
    rl = [int(v) for v in g["record_len"]]
    assert rl == R.RECORD_LEN
    for data in ("a", "d"):
        aff = torch.from_numpy(g[f"affine_{data}"])
        H, W = g[f"x_{data}"].shape[2:]
        assert tuple(aff.shape) == (4, R.L, R.L, 2, 3)
        eye = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], dtype=torch.float64)
        for b, n in enumerate(rl):       # every row of the pairwise matrix is filled: off the diagonal nothing is the identity
            for i in range(n):
                for j in range(n):
                    assert torch.equal(aff[b, i, j], eye) == (i == j), (b, i, j)
        ones = torch.ones(4, 1, H, W, dtype=torch.float64)
        to_off, from_off = R.warp(ones, aff[3, :4, 3]), R.warp(ones, aff[3, 3, :4])
        assert float(to_off[:3].abs().max()) == 0.0 and float(from_off[:3].abs().max()) == 0.0   # agent 3 of the last scene is off the map
        mask = R.warp(ones[:3], aff[1, 0, :3])
        assert 0.01 < float(((mask > 0) & (mask < 1 - 1e-9)).double().mean()) < 0.3       # the mask is fractional along the border


def _args(**kw):
    a = R.case_args(R.CASES["a"])
    a.update({k: v for k, v in kw.items() if k != "conv_gru"})
    a["conv_gru"] = dict(a["conv_gru"], **kw.get("conv_gru", {}))
    return a


def test_refusals_name_their_cause():
    from gencomm_amd import V2VNetFusion, _lib
    with pytest.raises(ValueError, match="agg_operator 'sum'"):
        V2VNetFusion(_args(agg_operator="sum"))
    with pytest.raises(NotImplementedError, match=r"kernel_size entry \[5, 5\]"):
        V2VNetFusion(_args(conv_gru={"kernel_size": [[5, 5]]}))
    with pytest.raises(ValueError, match="kernel_size has 1 entries for conv_gru.num_layers 2"):
        V2VNetFusion(_args(conv_gru={"num_layers": 2}))
    assert V2VNetFusion(_args(conv_gru={"num_layers": 2, "kernel_size": [[3, 3], [1, 1]]})).kernel_sizes == [(3, 3), (1, 1)]
    m = V2VNetFusion(_args()).eval()
    x, aff = torch.zeros(2, 8, 12, 20), torch.from_numpy(R.make_affine([2], 5, 12, 20, 0))
    with pytest.raises(NotImplementedError, match="v2vnet training"):       # parameters require grad, gradients are enabled
        m(x, [2], aff)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="v2vnet training"):       # ... or the input does
        m(x.clone().requires_grad_(), [2], aff)
    with torch.no_grad():
        with pytest.raises(ValueError, match="conv_gru.H, conv_gru.W = 12x20"):
            m(torch.zeros(2, 8, 10, 20), [2], aff)
        with pytest.raises(ValueError, match="in_channels 8"):
            m(torch.zeros(2, 6, 12, 20), [2], aff)
        with pytest.raises(ValueError, match="record_len"):
            m(x, [3], aff)
        with pytest.raises(ValueError, match="record_len"):
            m(x, [1, 1], aff)
        with pytest.raises(ValueError, match="1..8 agents"):
            m(torch.zeros(9, 8, 12, 20), [9], torch.zeros(1, 9, 9, 2, 3, dtype=torch.float64))
        with pytest.raises(_lib.GenCommHipError):                             # everything in order, but a CPU tensor: no fallback
            m(x, [2], aff)


def test_the_three_entries_are_declared_and_reject_bad_arguments():
    from gencomm_amd import _lib
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gencomm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("gencomm_v2v_warp_pairs_fwd", "gencomm_v2v_aggregate_fwd", "gencomm_gru_gate_fwd"):
        assert name in _lib.EXPORTED_SYMBOLS
        decl = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 12
    _lib.build()
    l = _lib.lib()
    assert l.gencomm_v2v_warp_pairs_fwd(None, None, None, None, 1, 8, 4, 4, None) == 1 and b"null pointer" in l.gencomm_last_error()
    assert l.gencomm_v2v_warp_pairs_fwd(1, 1, 1, 1, 0, 8, 4, 4, None) == 1 and b"warp pairs" in l.gencomm_last_error()
    assert l.gencomm_v2v_aggregate_fwd(None, None, None, None, None, None, None, 1, 8, 4, 4, 0, 0, None) == 1 and b"null pointer" in l.gencomm_last_error()
    assert l.gencomm_v2v_aggregate_fwd(1, 1, 1, 1, 1, 1, 1, 1, 8, 4, 4, 2, 0, None) == 1 and b"op must be" in l.gencomm_last_error()
    assert l.gencomm_v2v_aggregate_fwd(1, 1, 1, 1, 1, 1, 1, 1, 8, 4, 4, 0, 2, None) == 1 and b"out_mode must be" in l.gencomm_last_error()
    assert l.gencomm_v2v_aggregate_fwd(1, 1, 1, 1, 1, 1, 1, 0, 8, 4, 4, 0, 0, None) == 1 and b"v2v aggregate" in l.gencomm_last_error()
    assert l.gencomm_gru_gate_fwd(None, None, 1, 8, 16, None) == 1 and b"null pointer" in l.gencomm_last_error()
    assert l.gencomm_gru_gate_fwd(1, 1, 1, 0, 16, None) == 1 and b"gru gate" in l.gencomm_last_error()
