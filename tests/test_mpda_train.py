"""Training MPDA's feature aligner, CPU side: the trainable restatement (tests/mpda_train_restatement.py) against the gradients the
reference's OWN modules produced (tests/golden/mpda_train_*.npz; tools/make_golden_mpda_train.py), the new C-ABI entries and their
refusals, the ``trainable`` constructors, the gather-range arithmetic of the resize adjoint and the keep-mask packing."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mpda_restatement as R
import mpda_train_restatement as TR
from helpers import GOLDEN, assert_close
from gencomm_amd import synth

REPO = os.path.dirname(os.path.dirname(GOLDEN))

NEW_ENTRIES = {"gencomm_quad_attn_train_fwd": 17, "gencomm_quad_attn_bwd_workspace_bytes": 7, "gencomm_quad_attn_bwd": 23,
               "gencomm_resize_bilinear_bwd": 9, "gencomm_leaky_relu_fwd": 5, "gencomm_leaky_relu_bwd": 6}


def package_module(tag, trainable=True):
    """The package's module of a golden case, filled as the generator fills the reference's."""
    from gencomm_amd import CrossDomainFusionEncoder, DAImgHead, LearnableResizer, MPDAAlign
    c, args = TR.TRAIN_CASES[tag], TR.case_args(tag)
    m = {"resizer": lambda: LearnableResizer(args["resizer"], trainable=trainable), "cdt": lambda: CrossDomainFusionEncoder(args["cdt"], trainable=trainable),
         "da": lambda: DAImgHead(TR.C, trainable=trainable), "align": lambda: MPDAAlign(args, trainable=trainable)}[c["kind"]]()
    synth.fill_params_(m, TR.case_seed(tag))
    synth.fill_bn_stats_(m, TR.case_seed(tag) + 50)
    return m.train() if c["mode"] == "train" else m.eval()


@pytest.mark.parametrize("tag", list(TR.TRAIN_CASES))
def test_restatement_reproduces_the_reference_gradients(tag):
    """float64 restatement on the package module's parameters against the reference's float64 step: outputs, input gradients, every
    parameter gradient and (train() case) the BatchNorm running statistics after the step, to 1e-10."""
    rec = TR.load_golden(tag)
    names = TR.stored_names(rec)
    got = TR.run_case(tag, package_module(tag), torch.float64)
    assert sorted(got) == names, set(got) ^ set(names)
    assert any(k.startswith("g:") for k in names) and any(k.startswith("d_") for k in names)
    for k in names:
        assert_close(got[k], TR.stored(rec, k)[1], 1e-9, 1e-10, f"{tag} {k}")
    c = TR.TRAIN_CASES[tag]
    if c["mode"] == "train":
        assert sum(k.startswith("rs:") for k in names) == 8          # two blocks x two BatchNorms x (mean, var)
    if tag == "rebuttal":                                            # the maps pass straight through; so does the functional's gradient
        x = TR.case_inputs(tag)[0]
        assert np.array_equal(rec["y32/aligned"], x)
        assert not any(np.abs(rec["y32/" + k]).max() > 0 for k in names if k.startswith(("g:resizer", "g:cdt")))
    if tag == "da":                                                  # the reversal factor is in the stored input gradient
        m = package_module(tag)
        sd = TR.leaf_sd(m, torch.float64)
        x = torch.from_numpy(TR.case_inputs(tag)[0]).double().requires_grad_(True)
        g = torch.from_numpy(TR.functional(tag, (x.shape[0], 1, TR.H, TR.W))).double()
        plain, = torch.autograd.grad((TR.da_head(sd, "", x, None) * g).sum(), x)
        assert_close(-9.1 * plain.numpy(), TR.stored(rec, "d_x")[1], 1e-9, 1e-10, "da d_x = -9.1 x the head's plain gradient")


def test_new_entries_are_declared_exported_and_signature_matched():
    from gencomm_amd import _lib
    with open(os.path.join(REPO, "include", "gencomm_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW_ENTRIES.items():
        decl = re.search(r"\b(?:int|long long)\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert _lib.ABI_VERSION == 12 and _lib.lib().gencomm_abi_version() == 12          # additive entries: the ABI version stays
    assert len(_lib._SIGNATURES["gencomm_quad_attn_fwd"][1]) == 15 and len(_lib._SIGNATURES["gencomm_resize_bilinear_fwd"][1]) == 9
    assert os.path.exists(os.path.join(_lib.CSRC_DIR, "mpda_bwd_kernels.h"))
    with open(os.path.join(_lib.CSRC_DIR, "mpda_bwd_kernels.h")) as f:
        src = f.read()
    assert "atomicAdd" not in src and "fp contract(off)" in src


def test_new_entries_refuse_what_is_outside_their_domain():
    """Status codes with a message, before any launch: host pointers, no device."""
    from gencomm_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = dict(N=1, Nkv=1, heads=1, dim_head=32, H=2, W=2, q_ct=32, kv_ct=32, grid_mode=0)

    def train_fwd(q=p, k=p, v=p, out=p, keep=None, **kw):
        a = dict(good, **kw)
        return l.gencomm_quad_attn_train_fwd(q, k, v, None, keep, 1.0, out, a["N"], a["Nkv"], a["heads"], a["dim_head"], a["H"], a["W"], a["q_ct"],
                                             a["kv_ct"], a["grid_mode"], None)

    def bwd(q=p, k=p, v=p, dout=p, dq=p, dk=p, dv=p, bias=None, dbias=None, keep=None, ws=None, ws_bytes=0, **kw):
        a = dict(good, **kw)
        return l.gencomm_quad_attn_bwd(q, k, v, bias, keep, 1.0, dout, dq, dk, dv, dbias, a["N"], a["Nkv"], a["heads"], a["dim_head"], a["H"], a["W"],
                                       a["q_ct"], a["kv_ct"], a["grid_mode"], ws, ws_bytes, None)

    domain = ((dict(dim_head=24), "dim_head 24"), (dict(H=3), "even"), (dict(W=0), "even"), (dict(heads=0), "heads"), (dict(N=3, Nkv=2), "Nkv"),
              (dict(grid_mode=2), "grid_mode"), (dict(q_ct=16), "q_ct"), (dict(kv_ct=31), "kv_ct"), (dict(q=p + 4), "8-byte aligned"))
    for kw, word in ((dict(q=None), "null pointer"), (dict(out=None), "null pointer"), (dict(keep=p + 1), "2-byte aligned")) + domain:
        assert train_fwd(**kw) != 0, kw
        assert word in l.gencomm_last_error().decode(), (kw, l.gencomm_last_error())
    for kw, word in ((dict(dout=None), "null pointer"), (dict(dk=None), "null pointer"), (dict(bias=p), "null pointer"), (dict(dv=p + 4), "8-byte aligned"),
                     (dict(bias=p, dbias=p), "workspace"), (dict(N=2, Nkv=1), "workspace"), (dict(keep=p + 1), "2-byte aligned")) + domain:
        assert bwd(**kw) != 0, kw
        assert word in l.gencomm_last_error().decode(), (kw, l.gencomm_last_error())
    assert bwd(bias=p, dbias=p) == 2 and bwd(N=2, Nkv=1, ws=p, ws_bytes=8) == 2          # GC_ERR_WORKSPACE
    # the workspace query: nothing without a table and with one map per query map; the slabs and the partials otherwise
    assert l.gencomm_quad_attn_bwd_workspace_bytes(3, 3, 2, 32, 4, 6, 0) == 0
    assert l.gencomm_quad_attn_bwd_workspace_bytes(1, 1, 2, 32, 4, 6, 0) == 0
    assert l.gencomm_quad_attn_bwd_workspace_bytes(3, 3, 2, 32, 4, 6, 1) == 256              # 3 workgroups x 2 heads x 9 floats, rounded up
    assert l.gencomm_quad_attn_bwd_workspace_bytes(3, 1, 2, 32, 4, 6, 0) == 2 * 3 * 64 * 24 * 4
    assert l.gencomm_quad_attn_bwd_workspace_bytes(3, 1, 2, 24, 4, 6, 0) == -1 and "dim_head 24" in l.gencomm_last_error().decode()
    for args, word in (((None, p, 1, 1, 2, 2, 2, 2), "null pointer"), ((p, None, 1, 1, 2, 2, 2, 2), "null pointer"), ((p, p, 1, 1, 0, 2, 2, 2), "bad"),
                       ((p, p, 1, 1, 2, 2, 2, 0), "bad")):
        assert l.gencomm_resize_bilinear_bwd(*args, None) != 0, args
        assert word in l.gencomm_last_error().decode(), args
    assert l.gencomm_leaky_relu_fwd(None, p, 4, 0.01, None) != 0 and "null pointer" in l.gencomm_last_error().decode()
    assert l.gencomm_leaky_relu_fwd(p, p, 0, 0.01, None) != 0 and "n must be" in l.gencomm_last_error().decode()
    assert l.gencomm_leaky_relu_bwd(p, None, p, 4, 0.01, None) != 0 and "null pointer" in l.gencomm_last_error().decode()
    assert l.gencomm_leaky_relu_bwd(p, p, p, -1, 0.01, None) != 0 and "n must be" in l.gencomm_last_error().decode()


def test_trainable_constructors_keep_the_state_dict():
    from gencomm_amd import CrossDomainFusionEncoder, DAImgHead, LearnableResizer, MPDAAlign, SwapFusionEncoder
    args = R.shipped_args()
    m, d = MPDAAlign(args, trainable=True), MPDAAlign(args)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in d.state_dict().items()]
    assert [k for k, _ in m.named_buffers()] == [k for k, _ in d.named_buffers()]
    flagged = [n for n, s in m.named_modules() if getattr(s, "trainable", False)]
    assert {"", "resizer", "resizer.wg_att_1", "resizer.wg_att_2", "resizer.res_blocks.0", "resizer.res_blocks.1", "cdt", "classifier"} == set(flagged)
    assert not any(getattr(s, "trainable", False) for s in d.modules())
    for make in (lambda t: LearnableResizer(args["resizer"], trainable=t), lambda t: SwapFusionEncoder(args["resizer"]["wg_att"], trainable=t),
                 lambda t: CrossDomainFusionEncoder(args["cdt"], trainable=t), lambda t: DAImgHead(128, trainable=t)):
        assert list(make(True).state_dict()) == list(make(False).state_dict()) and make(True).trainable and not make(False).trainable


def test_default_constructor_still_refuses_and_trainable_refuses_what_is_not_built():
    from gencomm_amd import CrossDomainFusionEncoder, MPDAAlign, SwapFusionEncoder
    from gencomm_amd._lib import GenCommHipError
    args = R.case_args(R.CASES["c32"])
    x = torch.zeros(3, 32, 4, 6)
    d = MPDAAlign(args)
    with pytest.raises(NotImplementedError, match=r"MPDAAlign: train\(\) mode is not built \(mpda training -- dropout, BatchNorm batch statistics and every "
                                                  r"backward kernel -- is a later change\): call \.eval\(\)"):
        d(x, [1, 2])
    with pytest.raises(NotImplementedError, match=r"DAImgHead: mpda training is not built \(no backward kernels\): call it under torch.no_grad\(\), or with "
                                                  "nothing that requires a gradient"):
        d.eval().classifier(x)
    m = MPDAAlign(args, trainable=True)
    with pytest.raises(ValueError, match="window_size"):
        SwapFusionEncoder(dict(args["resizer"]["wg_att"], window_size=4), trainable=True)
    with pytest.raises(ValueError, match="dim_head"):
        CrossDomainFusionEncoder(dict(args["cdt"], dim_head=24), trainable=True)
    with pytest.raises(NotImplementedError, match="mask"):
        m.resizer.wg_att_1(x, mask=torch.ones(1))
    with pytest.raises(ValueError, match=r"H must be even.*H = 5"):
        m(torch.zeros(3, 32, 5, 6), [1, 2])
    with pytest.raises(ValueError, match=r"W must be even.*W = 7"):
        m.resizer.wg_att_1(torch.zeros(1, 32, 4, 7))
    for call in (lambda: m(x, [1, 2]), lambda: m.eval()(x.clone().requires_grad_(True), [1, 2]), lambda: m.classifier(x)):
        with pytest.raises(GenCommHipError, match="no CPU fallback"):      # the training path has no eager fall-back either
            call()


@pytest.mark.parametrize("n_in,n_out", [(3, 7), (7, 3), (5, 5), (6, 4), (2, 9), (1, 4)])
def test_resize_adjoint_gather_ranges(n_in, n_out):
    """The kernel's range arithmetic, restated in numpy (TR.first_output / resize_adjoint_matrix), against F.interpolate's autograd per
    axis: the gather matrix is the transpose of the forward's matrix; the ranges are contiguous, ordered, and cover every output that
    reads the source index -- nothing outside a range has a weight."""
    scale = np.float32(n_in) / np.float32(n_out)
    lo = [TR.first_output(i, scale, n_in, n_out) for i in range(-1, n_in + 2)]
    assert lo[0] == 0 and lo[1] == 0 and lo[-1] == n_out and lo[-2] == n_out and all(a <= b for a, b in zip(lo, lo[1:]))
    for i in range(n_in + 1):                                         # lo(i) really is the first output whose lower index is >= i
        first = next((o for o in range(n_out) if TR.resize_source(o, scale, n_in)[0] >= i), n_out)
        assert TR.first_output(i, scale, n_in, n_out) == first, i
    A = TR.resize_adjoint_matrix(n_in, n_out)
    for axis in (2, 3):
        shape = [1, 1, 4, 4]
        shape[axis] = n_in
        x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        size = [4, 4]
        size[axis - 2] = n_out
        y = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
        for o in range(n_out):                                        # column o of the forward's matrix along this axis
            g = torch.zeros_like(y)
            g.select(axis, o)[0, 0, 0] = 1.0                           # output (o, 0) along axis 2, (0, o) along axis 3
            col, = torch.autograd.grad(y, x, g, retain_graph=True)
            assert_close(A[:, o], (col[0, 0, :, 0] if axis == 2 else col[0, 0, 0, :]).numpy(), 1e-6, 1e-6, f"axis {axis} column {o}")
    if n_in == n_out:
        assert np.array_equal(A, np.eye(n_in))                        # a same-size call copies dy
    assert_close(A.sum(0), np.ones(n_out), 1e-6, 1e-6, "every output's weights sum to 1")


def test_keep_mask_packing_round_trips():
    from gencomm_amd.mpda import pack_keep, unpack_keep
    g = torch.Generator().manual_seed(3)
    keep = torch.rand(2, 3, 5, 16, generator=g) >= 0.5
    words = pack_keep(keep)
    assert words.dtype == torch.int16 and tuple(words.shape) == (2, 3, 5) and words.is_contiguous()
    assert torch.equal(unpack_keep(words), keep)
    one = torch.zeros(1, 1, 1, 16, dtype=torch.bool)
    one[..., 4 * 2 + 3] = True                                        # query token 2, key token 3 -> bit 11
    assert int(pack_keep(one)) == 1 << 11
    one[..., 15] = True                                               # bit 15 is the int16's sign: the uint16 pattern survives
    assert int(pack_keep(one)) & 0xFFFF == (1 << 11) | (1 << 15)
    assert int(pack_keep(torch.ones(1, 1, 1, 16, dtype=torch.bool))) & 0xFFFF == 0xFFFF
    assert int(pack_keep(torch.zeros(1, 1, 1, 16, dtype=torch.bool))) == 0
