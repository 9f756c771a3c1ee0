"""The HEAL and MPDA training criteria, the part that needs no GPU: the float64 restatement reproduces every loss, ``loss_dict`` entry
and gradient the reference's own modules produced (tests/golden/baseline_criteria.npz) to 1e-10, the fixture holds the situations its
cases are there for, the two ABI entries are declared, the new header obeys the contraction rule and has no atomics, the reference's
module names stay free for the shells, and the refusals hold."""
import ctypes
import importlib
import json
import os
import pkgutil
import re

import numpy as np
import pytest
import torch

import baseline_criteria_restatement as R
from test_abi import _contract_violations

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"gencomm_pyramid_occ_loss": 16, "gencomm_domain_bce_loss": 10}
HEADER = os.path.join(REPO, "gencomm_amd", "csrc", "criteria_kernels.h")


@pytest.fixture(scope="module")
def store():
    return np.load(R.GOLDEN)


def case_of(store, name):
    kind, args, extra = str(store[f"{name}/kind"]), json.loads(str(store[f"{name}/args"])), json.loads(str(store[f"{name}/extra"]))
    inp = {k.split("/in/")[1]: store[k] for k in store.files if k.startswith(f"{name}/in/")}
    return kind, args, inp, extra


CASES = list(R.all_cases())


def test_fixture_holds_the_cases_and_their_inputs(store):
    assert os.path.getsize(R.GOLDEN) < 1 << 20
    assert sorted({k.split("/")[0] for k in store.files}) == sorted(CASES)
    for name, (kind, args, inp, extra) in R.all_cases().items():
        k2, a2, i2, e2 = case_of(store, name)
        assert (k2, a2, e2) == (kind, args, extra) and sorted(i2) == sorted(inp)
        for k in inp:
            assert np.array_equal(i2[k], inp[k]) and i2[k].dtype == inp[k].dtype, (name, k)
            if k in R.LOGITS:
                assert (i2[k] != 0).all()   # the focal term has a kink at 0


def test_fixture_cases_contain_what_they_are_for(store):
    t = lambda name: {k: torch.from_numpy(v) for k, v in case_of(store, name)[2].items()}
    even = t("occ_even")
    pos, neg = even["pos_equal_one"], even["neg_equal_one"]
    assert pos[1].sum() == 0 and pos[2, ..., 0].sum() == 0 and pos[2, ..., 1].sum() == 1 and pos[0].sum() > 1
    assert tuple(neg[0, 3, 4]) == (1, 0) and pos[0, 3, 4].sum() == 0
    for k in (1, 2, 4):
        pos_l, neg_l = R.occ_level_labels(pos, neg, k)
        assert neg_l[0, 3 // k, 4 // k] == 0
        assert pos_l[2].sum() == 1 and pos_l[1].sum() == 0 and neg_l.sum() > 0
    floor = t("occ_floor")
    pos = floor["pos_equal_one"]
    assert pos.sum() == 3 and pos[:, :8].sum() == 0 and pos[:, :, :12].sum() == 0
    assert [tuple(floor[f"occ{i}"].shape[2:]) for i in range(3)] == [(10, 14), (5, 7), (2, 3)]
    assert R.occ_level_labels(pos, floor["neg_equal_one"], 4)[0].sum() == 0 and R.occ_level_labels(pos, floor["neg_equal_one"], 2)[0].sum() == 2
    kind, args, inp, _ = case_of(store, "occ_k3")
    assert args["pyramid"]["relative_downsample"] == [1, 3] and args["cls"]["gamma"] == 1.5 and inp["occ1"].shape[2:] == (3, 5)
    wide = case_of(store, "occ_wide")[2]
    assert wide["pos_equal_one"].shape == (2, 40, 72, 2) and 40 * 72 > 256 and (40 * 72) % 256 != 0   # several workgroups, a level boundary inside one
    da = case_of(store, "mpda_b")[2]["da_feature"]
    assert da.shape == (3, 2, 7, 9) and da.size % 4 != 0 and da[0].size % 4 != 0                       # no four-wide access fits it
    assert float(store["mpda_val/dict64/da_loss"]) == 0 and float(store["mpda/dict64/da_loss"]) > 0
    # the reference adds the domain term twice and logs it once
    heads = sum(float(store[f"mpda/dict64/{k}"]) for k in ("cls_loss", "reg_loss", "dir_loss"))
    assert abs(float(store["mpda/loss64"]) - heads - 2 * float(store["mpda/dict64/da_loss"])) < 1e-12
    assert abs(float(store["mpda_val/loss64"]) - heads) < 1e-12
    # 'collab' with suffix "" is PointPillarDepthLoss: the same head and depth inputs without the occupancy term
    assert abs(float(store["pyr_single/loss64"]) - float(store["pyr_collab/loss64"]) - float(store["pyr_single/dict64/pyramid_loss"])) < 1e-12
    for name in CASES:
        assert abs(float(store[f"{name}/loss64"]) - float(store[f"{name}/loss32"])) <= 1e-6 * abs(float(store[f"{name}/loss64"]))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name, store):
    kind, args, inp, extra = case_of(store, name)
    t = R.tensors(inp, torch.float64)
    total, d = R.run_restatement(kind, args, t, extra)
    total.backward()
    worst = {"loss": R.rel(total.detach(), store[f"{name}/loss64"])}
    stored = {k.split("/dict64/")[1] for k in store.files if k.startswith(f"{name}/dict64/")}
    assert stored == set(d), (stored, set(d))
    for k in d:
        worst["dict/" + k] = R.rel(d[k], store[f"{name}/dict64/{k}"])
    grads = {k.split("/grad64/")[1] for k in store.files if k.startswith(f"{name}/grad64/")}
    assert grads == {k for k, v in t.items() if v.grad is not None}
    for k in grads:
        worst["grad/" + k] = R.rms_rel(t[k].grad.numpy(), store[f"{name}/grad64/{k}"])
    if kind == "occ":
        p = args["pyramid"]
        occ = [t[f"occ{i}"] for i in range(len(p["relative_downsample"]))]
        levels = R.occ_loss(occ, t["pos_equal_one"], t["neg_equal_one"], p["relative_downsample"], p["weight"], args["pos_cls_weight"],
                            args["cls"]["gamma"], args["cls"]["alpha"])[1]
        for i, v in enumerate(levels):
            worst[f"level/{i}"] = R.rel(v, store[f"{name}/level64/{i}"])
    key = max(worst, key=worst.get)
    print(f"{name}: {len(worst)} numbers and tensors, worst {key}: {worst[key]:.2e}")
    assert worst[key] <= 1e-10, (key, worst[key])


@pytest.mark.parametrize("name", ["mpda", "mpda_b"])
def test_stable_domain_form_agrees_with_the_reference_call(name, store):
    """max(x, 0) - x t + log1p(exp(-|x|)), the form the kernel computes, in float64 against the stored value, which torch computed in
    float32 (float32 targets): within float32 rounding of a mean, and the gradient (sigmoid(x) - t) / numel to 1e-10."""
    kind, args, inp, extra = case_of(store, name)
    x = torch.from_numpy(inp["da_feature"]).double().requires_grad_(True)
    v = R.domain_bce_stable(x, extra["record_len"])
    v.backward()
    assert R.rel(v.detach(), store[f"{name}/dict64/da_loss"]) <= 2e-7
    t = R.domain_targets(x, extra["record_len"]).double()
    assert R.rms_rel((2 * (torch.sigmoid(x.detach()) - t) / x.numel()).numpy(), store[f"{name}/grad64/da_feature"]) <= 1e-10
    assert R.rms_rel(2 * x.grad.numpy(), store[f"{name}/grad64/da_feature"]) <= 1e-10


def test_entries_are_declared_in_header_binding_and_library():
    from gencomm_amd import _lib
    assert _lib.ABI_VERSION == 12
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gencomm_hip.h")).read(), flags=re.S)
    assert "#define GENCOMM_ABI_VERSION 12" in txt
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES[name][1]) == nargs
    _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in ENTRIES)
    l, p, err = _lib.lib(), 1 << 20, lambda: _lib.lib().gencomm_last_error()
    ptrs, ks, ws = (ctypes.c_void_p * 3)(p, p, p), (ctypes.c_int * 3)(1, 2, 4), (ctypes.c_float * 3)(0.4, 0.2, 0.1)
    occ = lambda *a: l.gencomm_pyramid_occ_loss(*a)
    assert occ(None, p, ptrs, ptrs, ks, ws, 3, 2, 12, 20, 2, 2.0, 2.0, 0.25, p, None) == 1 and b"null pointer" in err()
    assert occ(p, p, ptrs, ptrs, ks, ws, 5, 2, 12, 20, 2, 2.0, 2.0, 0.25, p, None) == 1 and b"levels" in err()
    assert occ(p, p, ptrs, ptrs, ks, ws, 3, 2, 12, 20, 1, 2.0, 2.0, 0.25, p, None) == 1 and b"A >= 2" in err()
    assert occ(p, p, ptrs, ptrs, ks, ws, 3, 2, 3, 20, 2, 2.0, 2.0, 0.25, p, None) == 1 and b"relative_downsample" in err()
    assert occ(p, p, (ctypes.c_void_p * 3)(p, None, p), ptrs, ks, ws, 3, 2, 12, 20, 2, 2.0, 2.0, 0.25, p, None) == 1 and b"level pointer" in err()
    src = (ctypes.c_int * 2)(0, 5)
    assert l.gencomm_domain_bce_loss(p, src, 2, p, None, 5, 1, 6, 10, None) == 1 and b"null pointer" in err()
    assert l.gencomm_domain_bce_loss(p, src, 2, p, p, 5, 1, 6, 10, None) == 1 and b"source index" in err()
    assert l.gencomm_domain_bce_loss(p, src, 2, p, p, 2000, 1, 6, 10, None) == 1 and b"bad dims" in err()


def test_header_states_its_contraction_mode_and_has_no_atomics():
    from gencomm_amd import _lib
    txt = open(HEADER).read()
    assert _contract_violations(txt) == []
    assert len(re.findall(r"^#pragma clang fp contract\((off|fast)\)", txt, flags=re.M)) == 2   # states a mode, and hands `fast` back
    assert "atomicAdd" not in txt and not re.search(r"\batomic\w*\s*\(|__hip_atomic|__atomic_", txt)
    own = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(_lib.CSRC_DIR, "gencomm_abi_aux.hip")).read(), flags=re.M)
    assert "criteria_kernels.h" in own and own[1:] == sorted(own[1:])


def test_reference_module_names_stay_free_for_the_shells():
    import gencomm_amd
    names = {m.name for m in pkgutil.iter_modules(gencomm_amd.__path__)}
    assert "baseline_criteria" in names and not names & {"point_pillar_pyramid_loss", "point_pillar_mpda_loss"}
    m = importlib.import_module("gencomm_amd.baseline_criteria")
    assert gencomm_amd.PointPillarPyramidLoss is m.PointPillarPyramidLoss and gencomm_amd.PointPillarMPDALoss is m.PointPillarMPDALoss
    assert {"PointPillarPyramidLoss", "PointPillarMPDALoss"} <= set(gencomm_amd.__all__)
    assert issubclass(m.PointPillarPyramidLoss, gencomm_amd.PointPillarDepthLoss)


def test_refusals(store):
    from gencomm_amd import _lib
    from gencomm_amd import baseline_criteria as BC
    kind, args, inp, extra = case_of(store, "occ_even")
    t = R.tensors(inp, torch.float32, grad=False)
    crit = BC.PointPillarPyramidLoss(args)
    out, tgt = R.dicts(kind, t)
    with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):          # CPU tensors
        crit(out, tgt, "_single")
    with pytest.raises(_lib.GenCommHipError, match="no CPU fallback"):
        BC.domain_bce_loss(torch.zeros(3, 1, 4, 4), [1, 2])
    with pytest.raises(ValueError, match="'neither'"):                         # an unknown pyramid value, an unknown suffix
        crit(dict(out, pyramid="neither"), tgt)
    with pytest.raises(ValueError, match="'_ego'"):
        crit(out, tgt, "_ego")
    with pytest.raises(KeyError):
        BC.PointPillarPyramidLoss({k: v for k, v in args.items() if k != "pyramid"})
    for key in (BC.PointPillarMPDALoss, BC.PointPillarPyramidLoss):            # iou
        with pytest.raises(NotImplementedError, match="iou"):
            key(dict(args, iou={"sigma": 3.0, "weight": 1.0}))
    BC.PointPillarMPDALoss(dict(R.MPDA_ARGS, depth={"weight": 1.0}))           # accepted and ignored
    assert BC.source_index([2, 3]) == [0, 2] and BC.source_index(torch.tensor([1, 2, 1])) == [0, 1, 3]


def test_shape_refusals_name_the_level(store, monkeypatch):
    """The shape checks come before anything touches the device: run them on CPU tensors with the device check switched off."""
    from gencomm_amd import baseline_criteria as BC
    monkeypatch.setattr(BC, "require_gpu", lambda t, what: None)
    kind, args, inp, extra = case_of(store, "occ_floor")
    t = R.tensors(inp, torch.float32, grad=False)
    crit = BC.PointPillarPyramidLoss(args)
    out, tgt = R.dicts(kind, t)
    ceil = dict(out, occ_single_list=[t["occ0"], t["occ1"], torch.zeros(2, 1, 3, 4)])      # a ceil-pooled level
    with pytest.raises(ValueError, match=r"level 2: occupancy map must be \(2, 1, 2, 3\)"):
        crit(ceil, tgt, "_single")
    with pytest.raises(ValueError, match=r"level 1: .*batch of 2"):                         # a batch mismatch
        crit(dict(out, occ_single_list=[t["occ0"], t["occ1"][:1], t["occ2"]]), tgt, "_single")
    with pytest.raises(ValueError, match="4 occupancy maps"):
        crit(dict(out, occ_single_list=[t["occ0"]] * 4), tgt, "_single")
    with pytest.raises(ValueError, match="A >= 2"):
        crit(out, {k: v[..., :1] for k, v in tgt.items()}, "_single")
    with pytest.raises(ValueError, match="record_len"):
        BC.domain_bce_loss(torch.zeros(3, 1, 4, 4), [2, 2])
