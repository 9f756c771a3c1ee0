"""Training of the V2VNet fusion (`V2VNetFusion(args, trainable=True)`), the parts that need no GPU: the five new entries of the C ABI,
the constructor switch and the refusals, the decomposed restatement UNDER AUTOGRAD against the reference's own float64 gradients
(tests/golden/v2vnet_train.npz, v2vnet_train_d.npz, made by tools/make_golden_v2vnet_train.py) -- which pins that the three rewrites the
HIP path is built on, the ego-only last round included, have the reference's gradient --, the fixture's own claims, and the host helper
that lists the pairs by source row. The HIP path is tested in test_gpu_v2vnet_train.py."""
import os
import re

import numpy as np
import pytest
import torch

import v2vnet_restatement as R
import v2vnet_train_restatement as TR

NEW_ENTRIES = ("gencomm_gru_gate_bwd", "gencomm_v2v_aggregate_train_fwd", "gencomm_v2v_aggregate_bwd",
               "gencomm_v2v_warp_pairs_bwd_scratch_floats", "gencomm_v2v_warp_pairs_bwd")


def test_the_five_entries_are_declared_and_reject_bad_arguments():
    from gencomm_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gencomm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTED_SYMBOLS, name
        decl = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert _lib.ABI_VERSION == 12
    _lib.build()
    l = _lib.lib()
    err = l.gencomm_last_error
    assert l.gencomm_gru_gate_bwd(None, None, None, 1, 8, 16, None) == 1 and b"null pointer" in err()
    assert l.gencomm_gru_gate_bwd(1, 1, 1, 1, 0, 16, None) == 1 and b"gru gate backward" in err()
    assert l.gencomm_v2v_aggregate_train_fwd(None, None, None, None, None, None, None, None, 1, 8, 4, 4, 0, 0, None) == 1 and b"null pointer" in err()
    assert l.gencomm_v2v_aggregate_train_fwd(1, 1, 1, 1, 1, 1, 1, None, 1, 8, 4, 4, 1, 0, None) == 1 and b"winner" in err()   # max needs the map
    assert l.gencomm_v2v_aggregate_train_fwd(1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 4, 4, 2, 0, None) == 1 and b"op must be" in err()
    assert l.gencomm_v2v_aggregate_train_fwd(1, 1, 1, 1, 1, 1, 1, 1, 0, 8, 4, 4, 0, 0, None) == 1 and b"v2v aggregate" in err()
    assert l.gencomm_v2v_aggregate_bwd(None, None, None, None, None, None, None, 1, 8, 4, 4, 0, 0, None) == 1 and b"null pointer" in err()
    assert l.gencomm_v2v_aggregate_bwd(1, 1, 1, 1, None, 1, 1, 1, 8, 4, 4, 1, 0, None) == 1 and b"winner" in err()
    assert l.gencomm_v2v_aggregate_bwd(1, 1, 1, 1, 1, 1, 1, 1, 8, 4, 4, 0, 2, None) == 1 and b"out_mode must be" in err()
    assert l.gencomm_v2v_aggregate_bwd(1, 1, 1, 1, 1, 1, 1, 70000, 8, 4, 4, 0, 0, None) == 1 and b"v2v aggregate backward" in err()
    assert l.gencomm_v2v_warp_pairs_bwd_scratch_floats(0) == -1 and b"warp pairs backward" in err()
    assert l.gencomm_v2v_warp_pairs_bwd_scratch_floats(25) >= 25
    assert l.gencomm_v2v_warp_pairs_bwd(None, None, None, None, None, None, None, 1, 1, 8, 4, 4, 0, None) == 1 and b"null pointer" in err()
    assert l.gencomm_v2v_warp_pairs_bwd(1, 1, 1, 1, 1, 1, 1, 1, 0, 8, 4, 4, 0, None) == 1 and b"warp pairs backward" in err()
    assert l.gencomm_v2v_warp_pairs_bwd(1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 4, 4, 2, None) == 1 and b"accumulate must be" in err()
    # the weight gradient with a fixed order of additions, which the training path uses
    for name in ("gencomm_conv2d_wgrad_fixed_scratch_floats", "gencomm_conv2d_wgrad_fixed"):
        assert name in _lib.EXPORTED_SYMBOLS
        decl = re.search(name + r"\s*\(([^)]*)\)", hdr).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert l.gencomm_conv2d_wgrad_fixed_scratch_floats(2, 8, 6, 10, 8, 5) == -1 and b"bad dims" in err()
    assert l.gencomm_conv2d_wgrad_fixed_scratch_floats(2, 8, 6, 10, 8, 3) > 0 and l.gencomm_conv2d_wgrad_fixed_scratch_floats(2, 64, 6, 10, 64, 3) > 0
    assert l.gencomm_conv2d_wgrad_fixed(None, None, None, None, 2, 8, 6, 10, 8, 3, None, 0, None) == 1 and b"null pointer" in err()
    assert l.gencomm_conv2d_wgrad_fixed(1, 1, 1, 1, 2, 8, 6, 10, 8, 3, 1, 16, None) == 1 and b"scratch smaller" in err()


def test_trainable_switch_constructs_and_refuses_cpu_tensors():
    from gencomm_amd import V2VNetFusion, _lib
    args = TR.case_args("a")
    m = V2VNetFusion(args, trainable=True).eval()
    assert m.trainable and not V2VNetFusion(args).trainable
    assert [k for k, _ in m.state_dict().items()] == [k for k, _ in V2VNetFusion(args).state_dict().items()]
    x, aff = torch.zeros(2, 8, 12, 20), torch.from_numpy(R.make_affine([2], 5, 12, 20, 0))
    with pytest.raises(_lib.GenCommHipError):                     # gradients enabled, CPU tensors: no fallback to torch
        m(x, [2], aff)
    with pytest.raises(_lib.GenCommHipError):
        m(x.clone().requires_grad_(), [2], aff)
    with pytest.raises(NotImplementedError, match="v2vnet training"):       # the default is what it was
        V2VNetFusion(args).eval()(x, [2], aff)


@pytest.mark.parametrize("tag", TR.TRAIN_CASES)
def test_restatement_autograd_reproduces_the_reference_gradients_in_float64(tag):
    """torch autograd of the decomposed forward in float64 against the reference's float64 gradients: 1e-12 relative rms, the bound of
    test_restatement_reproduces_the_reference_in_float64 (measured: at most 6.6e-16)."""
    c = TR.load_train_case(tag)
    _, gx, g = TR.restatement_grads(c["sd"], c["args"], c["x"], c["record_len"], c["affine"], c["grad_out"], torch.float64)
    print(f"case {tag}: d x rel rms {R.rel_rms(gx, c['gx64']):.2e}")
    assert gx.shape == c["gx64"].shape and R.rel_rms(gx, c["gx64"]) <= 1e-12
    assert set(c["g64"]) <= set(c["sd"])
    for name in c["sd"]:
        if name not in c["g64"]:
            assert g[name] is None, name
            continue
        print(f"  {name}: rel rms {R.rel_rms(g[name], c['g64'][name]):.2e}")
        assert g[name].shape == c["g64"][name].shape and R.rel_rms(g[name], c["g64"][name]) <= 1e-12, name


def test_fixture_exercises_what_it_claims():
    from helpers import load_case
    g = load_case("v2vnet_train")
    # bt: the margin condition, recomputed from the stored inputs
    c = TR.load_train_case("bt")
    rep = TR.margin_report(c["sd"], c["args"], c["x"], c["record_len"], c["affine"])
    print(f"bt (seed {int(g['bt_seed'])}): {rep}")
    assert rep["same_winners"] and rep["live"] == int(g["bt_live"]) and rep["live"] > 3000
    assert rep["ratio"] >= TR.MARGIN_FACTOR
    assert abs(rep["margin"] - float(g["bt_margin"])) <= 1e-12
    sd, x, aff = TR.bt_inputs(int(g["bt_seed"]))                  # ... and the stored inputs are the seeded ones
    assert np.array_equal(x, c["x"]) and np.array_equal(aff, c["affine"]) and all(torch.equal(sd[k], c["sd"][k]) for k in sd)
    # the off-map agent (the last of scene 2) gets an exactly zero input gradient, the others do not
    row = sum(TR.BT["record_len"][:2]) + 3
    assert float(np.abs(c["gx64"][row]).max()) == 0.0 and all(np.abs(c["gx64"][r]).max() > 0 for r in range(row))
    for tag in TR.TRAIN_CASES:
        c = TR.load_train_case(tag)
        C = c["args"]["in_channels"]
        gru = [k for k in c["sd"] if k.startswith("conv_gru.")]
        if not c["args"]["gru_flag"]:
            assert tag == "c" and gru and not any(k in c["g64"] for k in gru)      # no gradient at all
            continue
        for k in gru:                                             # the blocks that multiply the zero hidden state: exact zeros
            blocks = TR.reset_and_hidden_blocks(k, c["g64"][k], C)
            assert all(float(np.abs(b).max()) == 0.0 for b in blocks), k
            assert float(np.abs(c["g64"][k]).max()) > 0.0
        assert set(c["ref"]) == set(c["g64"]) | {"x"} and all(0 < v < 1e-6 for v in c["ref"].values())


@pytest.mark.parametrize("record_len", [[2, 3, 1, 4], [8]])
def test_pairs_by_source_row_against_brute_force(record_len):
    from gencomm_amd.v2vnet import pairs_by_source_row
    off = np.concatenate([[0], np.cumsum(record_len)]).tolist()
    full = [off[b] + j for b, k in enumerate(record_len) for _ in range(k) for j in range(k)]      # every (target, source) pair
    for src, rows in ((full, off[-1]), (list(range(off[-1])), off[-1]), ([2, 0, 2, 2], 4)):
        rpo, rp = pairs_by_source_row(src, rows)
        assert len(rpo) == rows + 1 and rpo[0] == 0 and rpo[-1] == len(src) and sorted(rp) == list(range(len(src)))
        for r in range(rows):
            assert rp[rpo[r]:rpo[r + 1]] == [p for p, s in enumerate(src) if s == r]              # ascending within a row
    if record_len == [8]:
        rpo, _ = pairs_by_source_row(full, 8)
        assert [rpo[r + 1] - rpo[r] for r in range(8)] == [8] * 8                                  # a row read by eight targets
