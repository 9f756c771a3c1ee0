"""Training the max fusion and the who2com fusion, CPU side: the torch restatements of both modules (tests/fusion_train_restatement.py)
against the fixtures the reference's OWN modules produced (tests/golden/maxfuse_train.npz, who2com.npz; tools/make_golden_fusion_train.py),
values and gradients; Who2comFusion's checkpoint keys; the stage-1 and stage-2 shells with `fusion_method: who2com`."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import fusion_train_restatement as R
from helpers import GOLDEN, assert_close, load_case


def test_max_restatement_matches_the_reference_fixture():
    g = load_case("maxfuse_train")
    rl = [int(v) for v in g["record_len"]]
    near = R.near_tie_mask(g["x"], rl, g["affine"]).numpy()
    assert float(near.mean()) == float(g["near_tie_share"]) <= R.NEAR_TIE_CAP      # a condition of the fixture, not a measurement
    assert np.all(g["G"][near] == 0) and np.count_nonzero(g["G"]) == g["G"].size - int(near.sum())
    assert int(g["exact_ties"]) > 0.05 * near.size                                   # exact ties are NOT excluded
    res = R.reference_grads(g["x"], rl, g["affine"], g["G"])
    assert np.array_equal(res[torch.float32][0], g["out32"])                         # the same ATen operators in the same order
    assert np.array_equal(res[torch.float32][1], g["dx32"])
    assert_close(res[torch.float64][0], g["out64"], 1e-12, 1e-12, "max float64 out")
    assert_close(res[torch.float64][1], g["dx64"], 1e-12, 1e-12, "max float64 dx")
    # the winner of an exact tie is the lowest agent index: scene 1's third agent lies outside the map (an exact-zero row), so it may
    # never receive a gradient even where it ties at 0 with the second agent
    assert np.count_nonzero(g["dx32"][4]) == 0 and np.count_nonzero(g["dx64"][4]) == 0


def test_who2com_restatement_matches_the_reference_fixture():
    g = load_case("who2com")
    rl = [int(v) for v in g["record_len"]]
    for dtype, tag, rtol, atol in ((torch.float32, "32", 1e-4, 1e-5), (torch.float64, "64", 1e-10, 1e-11)):
        x = torch.from_numpy(g["x"]).to(dtype).requires_grad_(True)
        w, b = (torch.from_numpy(g[k]).to(dtype).requires_grad_(True) for k in ("weight", "bias"))
        out = R.who2com_forward(w, b, x, rl, torch.from_numpy(g["affine"]))
        assert list(out.shape) == [len(rl), x.shape[1], x.shape[2], x.shape[3]]
        assert_close(out.detach().numpy(), g["out" + tag], rtol, atol, "who2com out " + tag)
        (out * torch.from_numpy(g["G"]).to(dtype)).sum().backward()
        for name, got in (("dx", x.grad), ("gw", w.grad), ("gb", b.grad)):
            assert_close(got.numpy(), g[name + tag], 2 * rtol, 2 * atol, f"who2com {name}{tag}")


def test_who2com_checkpoint_keys_match_the_reference():
    from gencomm_amd import Who2comFusion
    with open(os.path.join(GOLDEN, "who2com_keys.json")) as f:
        spec = json.load(f)
    net = Who2comFusion(spec["args"])
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == spec["state_dict"]       # keys, order and shapes
    assert [k for k, _ in net.named_parameters()] == ["decode_layer.weight", "decode_layer.bias"]  # `att` has no parameters
    assert list(Who2comFusion({"feat_dim": 128}).state_dict()) == [k for k, _ in spec["state_dict"]]
    with pytest.raises(KeyError):
        Who2comFusion({"feature_dims": 128})
    with pytest.raises(TypeError):
        Who2comFusion("128")


def _shell_args(stage):
    if stage == 1:
        with open(os.path.join(GOLDEN, "shell_state_dict_keys.json")) as f:
            return copy.deepcopy(json.load(f)["args"])
    return json.loads(str(load_case("shell2")["args"]))


@pytest.mark.parametrize("stage", [1, 2])
def test_shells_construct_who2com_and_still_refuse_the_rest(stage):
    from gencomm_amd.heter_model import HeterModelBaselineWDiffCommStage2, HeterModelBaselineWGenComm, _OTHER_FUSIONS
    from gencomm_amd.who2com import Who2comFusion
    cls = HeterModelBaselineWGenComm if stage == 1 else HeterModelBaselineWDiffCommStage2
    args = _shell_args(stage)
    base = cls(copy.deepcopy(args))
    args["fusion_method"], args["who2com"] = "who2com", 128
    model = cls(copy.deepcopy(args))
    assert isinstance(model.fusion_net, Who2comFusion)
    strip = lambda m: {k: list(v.shape) for k, v in m.state_dict().items() if not k.startswith("fusion_net.")}
    assert strip(model) == strip(base)
    assert {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith("fusion_net.")} == \
        {"fusion_net.decode_layer.weight": [128, 256, 3, 3], "fusion_net.decode_layer.bias": [128]}
    if stage == 2:   # fusion_net is one of stage 2's fixed modules (stage2.py:180-185)
        assert not any(p.requires_grad for p in model.fusion_net.parameters())
    assert _OTHER_FUSIONS == ("disconet", "v2vnet")
    for method in _OTHER_FUSIONS:
        bad = copy.deepcopy(args)
        bad["fusion_method"] = method
        with pytest.raises(NotImplementedError, match="who2com"):
            cls(bad)
