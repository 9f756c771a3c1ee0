"""MPDA's feature aligner, CPU side: the torch restatement (tests/mpda_restatement.py) against the fixture the reference's OWN modules
produced (tests/golden/mpda.npz; tools/make_golden_mpda.py), the checkpoint keys, the refusals, the C-ABI entries and the absence of
a baseline shell."""
import ctypes
import json
import os
import pkgutil
import re

import numpy as np
import pytest
import torch

import mpda_restatement as R
from helpers import GOLDEN, assert_close, load_case
from gencomm_amd import synth

REPO = os.path.dirname(os.path.dirname(GOLDEN))


@pytest.fixture(scope="module")
def g():
    return load_case("mpda")


def golden_pair(g, name, tag):
    """(y32, y64, e_ref) of one stored output: the float64 output is y32 - d64 in float64."""
    y32 = g[f"{name}_y32_{tag}"]
    return y32, y32.astype(np.float64) - g[f"{name}_d64_{tag}"].astype(np.float64), float(g[f"{name}_eref_{tag}"])


def filled(module, seed):
    module = module.eval()
    synth.fill_params_(module, seed)
    synth.fill_bn_stats_(module, seed + 50)
    return module


def package_modules(tag):
    """The package's four modules of a case, filled as tools/make_golden_mpda.py fills the reference's."""
    from gencomm_amd import CrossDomainFusionEncoder, DAImgHead, LearnableResizer, MPDAAlign
    c = R.CASES[tag]
    args = R.case_args(c)
    s_res, s_cdt, s_da, s_al = R.case_seeds(tag)
    return (filled(LearnableResizer(args["resizer"]), s_res), filled(CrossDomainFusionEncoder(args["cdt"]), s_cdt),
            filled(DAImgHead(c["C"]), s_da), filled(MPDAAlign(args), s_al))


@pytest.mark.parametrize("tag", list(R.CASES))
def test_restatement_reproduces_the_reference(g, tag):
    """The float64 restatement on the package modules' parameters against the reference's float64 outputs: the restatement is the
    reference's arithmetic, and the package's constructors draw the parameters the reference's drew."""
    assert int(g["seed"]) == R.SEED
    c = R.CASES[tag]
    res, cdt, da, al = package_modules(tag)
    ego, cav, cdt_cav, x = (None if a is None else torch.from_numpy(a).double() for a in R.case_inputs(tag))
    with torch.no_grad():
        out = R.resizer(R.double_sd(res), "", ego, cav, c["dim_head"])
        assert_close(out.numpy(), golden_pair(g, "resizer", tag)[1], 1e-9, 1e-10, f"{tag} resizer")
        out = R.cdt(R.double_sd(cdt), "", ego, cdt_cav, c["heads"], c["dim_head"])
        assert_close(out.numpy(), golden_pair(g, "cdt", tag)[1], 1e-9, 1e-10, f"{tag} cdt")
        out = R.da_head(R.double_sd(da), "", cdt_cav)
        assert_close(out.numpy(), golden_pair(g, "da", tag)[1], 1e-9, 1e-10, f"{tag} da")
        if c["record_len"]:
            feats, logits = R.mpda_align(R.double_sd(al), R.case_args(c), x, c["record_len"])
            assert_close(feats.numpy(), golden_pair(g, "align", tag)[1], 1e-9, 1e-10, f"{tag} align")
            assert_close(logits.numpy(), golden_pair(g, "logits", tag)[1], 1e-9, 1e-10, f"{tag} logits")
            if c["rebuttal"]:
                assert np.array_equal(golden_pair(g, "align", tag)[0], R.case_inputs(tag)[3])
    for name in ("resizer", "cdt", "da"):
        assert 0 < golden_pair(g, name, tag)[2] < 1e-6, (name, tag)


def test_kernel_restatement_partitions():
    """The two partitions are inverses of their own un-partition and differ from each other; the bias index is the module's buffer."""
    from gencomm_amd.mpda import Attention
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float64).reshape(2, 3, 4, 6)
    for grid in (False, True):
        assert torch.equal(R.from_groups(R.to_groups(x, grid), grid, 4, 6), x)
    w, gr = R.to_groups(x, False), R.to_groups(x, True)
    assert not torch.equal(w, gr)
    # group (x 1, y 2) of map 0, channel 0: window pixels (2, 4) (2, 5) (3, 4) (3, 5); grid pixels (1, 2) (1, 5) (3, 2) (3, 5)
    assert w[0, 1 * 3 + 2, :, 0].tolist() == [16.0, 17.0, 22.0, 23.0]
    assert gr[0, 1 * 3 + 2, :, 0].tolist() == [8.0, 11.0, 20.0, 23.0]
    index = Attention(64, 32, 0.0, 2).rel_pos_indices
    assert torch.equal(index, R.rel_pos_indices(2))
    tok = [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert index.tolist() == [[(hi - hj + 1) * 3 + (wi - wj + 1) for hj, wj in tok] for hi, wi in tok]


def test_state_dict_keys_are_the_references():
    from gencomm_amd import MPDAAlign
    with open(os.path.join(GOLDEN, "mpda_keys.json")) as f:
        want = json.load(f)
    assert want["args"] == R.shipped_args() and want["classifier_in_channels"] == 128
    m = MPDAAlign(R.shipped_args())
    assert m.rebuttal is False and m.classifier.conv1_da.in_channels == 128
    for name in ("resizer", "cdt", "classifier"):
        assert [[k, list(v.shape)] for k, v in getattr(m, name).state_dict().items()] == want["state_dict"][name], name
    keys = list(m.state_dict())
    assert "resizer.wg_att_1.layers.0.block.5.fn.rel_pos_bias.weight" in keys and "cdt.layers.0.cross_win_2.to_v.1.bias" in keys
    assert not any("rel_pos_indices" in k for k in keys)          # registered with persistent=False, as in the reference
    assert m.cdt.layers[0].win_size == 2                          # hard-coded, whatever window_size says
    from gencomm_amd import CrossDomainFusionEncoder
    assert CrossDomainFusionEncoder(dict(R.shipped_args()["cdt"], window_size=8)).layers[0].win_size == 2


def test_refusals_name_what_they_refuse():
    from gencomm_amd import CrossDomainFusionEncoder, DAImgHead, LearnableResizer, MPDAAlign, SwapFusionEncoder
    args = R.case_args(R.CASES["c32"])
    with pytest.raises(ValueError, match="window_size"):
        SwapFusionEncoder(dict(args["resizer"]["wg_att"], window_size=4))
    with pytest.raises(ValueError, match="window_size"):
        MPDAAlign(dict(args, resizer=dict(args["resizer"], wg_att=dict(args["resizer"]["wg_att"], window_size=8))))
    with pytest.raises(ValueError, match="dim_head"):
        CrossDomainFusionEncoder(dict(args["cdt"], dim_head=24))
    x = torch.zeros(3, 32, 4, 6)
    m = MPDAAlign(args)
    assert m.training
    calls = {"MPDAAlign": lambda x: m(x, [1, 2]), "LearnableResizer": lambda x: m.resizer(x[:1], x[1:]),
             "CrossDomainFusionEncoder": lambda x: m.cdt(x[:1], x[1:]), "SwapFusionEncoder": lambda x: m.resizer.wg_att_1(x),
             "DAImgHead": lambda x: m.classifier(x)}
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match=r"train\(\).*mpda training"):
            call(x)
    m.eval()
    for name, call in calls.items():                              # trainable parameters, gradients enabled
        with pytest.raises(NotImplementedError, match="mpda training"):
            call(x)
    for p in m.parameters():
        p.requires_grad_(False)
    for name, call in calls.items():                              # a trainable input
        with pytest.raises(NotImplementedError, match="mpda training"):
            call(x.clone().requires_grad_(True))
    # odd maps, named by their dimension (checked before the device is)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"H must be even.*H = 5"):
            m(torch.zeros(3, 32, 5, 6), [1, 2])
        with pytest.raises(ValueError, match=r"W must be even.*W = 7"):
            m.resizer.wg_att_1(torch.zeros(1, 32, 4, 7))
        with pytest.raises(ValueError, match=r"W must be even.*W = 3"):
            m.cdt(torch.zeros(1, 32, 4, 3), torch.zeros(2, 32, 4, 3))
        with pytest.raises(ValueError, match=r"collaborator.*H must be even.*H = 3"):
            m.resizer(torch.zeros(1, 32, 4, 6), torch.zeros(1, 32, 3, 6))
        with pytest.raises(ValueError, match="record_len"):
            m(x, [2, 2])
        from gencomm_amd._lib import GenCommHipError
        with pytest.raises(GenCommHipError, match="no CPU fallback"):     # no eager fall-back
            m(x, [1, 2])


def test_entries_are_declared_and_exported():
    from gencomm_amd import _lib
    with open(os.path.join(REPO, "include", "gencomm_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in {"gencomm_quad_attn_fwd": 15, "gencomm_resize_bilinear_fwd": 9}.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert len(_lib._SIGNATURES["gencomm_conv2d_act_res_fwd"][1]) == 17       # LeakyReLU is a value of `act`, not a new entry
    assert _lib.ABI_VERSION == 12                        # additive entries: the ABI version stays
    assert os.path.exists(os.path.join(_lib.CSRC_DIR, "mpda_kernels.h"))


def test_entries_refuse_what_is_outside_their_domain():
    """Status codes with a message, before any launch: no device is needed to see them."""
    from gencomm_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = dict(N=1, Nkv=1, heads=1, dim_head=32, H=2, W=2, q_ct=32, kv_ct=32, grid_mode=0)

    def quad(q=p, k=p, v=p, out=p, **kw):
        a = dict(good, **kw)
        return l.gencomm_quad_attn_fwd(q, k, v, None, out, a["N"], a["Nkv"], a["heads"], a["dim_head"], a["H"], a["W"], a["q_ct"], a["kv_ct"],
                                       a["grid_mode"], None)

    for kw, word in ((dict(q=None), "null pointer"), (dict(out=None), "null pointer"), (dict(dim_head=24), "dim_head 24"), (dict(H=3), "even"),
                     (dict(W=0), "even"), (dict(heads=0), "heads"), (dict(N=3, Nkv=2), "Nkv"), (dict(grid_mode=2), "grid_mode"),
                     (dict(q_ct=16), "q_ct"), (dict(q=p + 4), "8-byte aligned")):
        assert quad(**kw) != 0, kw
        assert word in l.gencomm_last_error().decode(), (kw, l.gencomm_last_error())
    for args, word in (((None, p, 1, 1, 2, 2, 2, 2), "null pointer"), ((p, None, 1, 1, 2, 2, 2, 2), "null pointer"), ((p, p, 1, 1, 0, 2, 2, 2), "bad"),
                       ((p, p, 1, 1, 2, 2, 2, 0), "bad")):
        assert l.gencomm_resize_bilinear_fwd(*args, None) != 0, args
        assert word in l.gencomm_last_error().decode(), args
    assert l.gencomm_conv2d_act_res_fwd(p, p, p, p, None, p, 1, 1, 2, 2, 1, 3, 3, 1, 1, 5, None) != 0      # act 5 does not exist


def test_no_baseline_shell_module():
    import gencomm_amd
    names = {m.name for m in pkgutil.iter_modules(gencomm_amd.__path__)}
    assert "mpda" in names
    assert not names & {"heter_model_baseline_w_mpda", "point_pillar_mpda_loss"}
