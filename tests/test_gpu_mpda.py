"""MPDA's feature aligner on the GPU: the quad-attention and bilinear-resize kernels and the LeakyReLU layer alone against float64, the
four modules against the reference's stored outputs (tests/golden/mpda.npz), and determinism. Outputs start as NaN and the allocator
is poisoned, so an element a kernel leaves out, or a workspace it reads without writing, shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mpda_restatement as R
from helpers import assert_close, load_case
from gencomm_amd import _lib
from gencomm_amd.mpda import Attention, _conv_bn_act
from gencomm_amd.runtime import ptr, stream_ptr
from test_mpda import golden_pair, package_modules

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def poison_allocator():
    """Leave NaNs in the memory torch's caching allocator hands out next: a kernel that reads a workspace it did not write shows."""
    junk = torch.full((32 << 20,), float("nan"), device=DEV)
    del junk


def quad_attn_hip(q, k, v, table, heads, dh, grid, q_coff=0, k_coff=0, v_coff=0):
    """gencomm_quad_attn_fwd on device tensors, each read from its channel offset on; the output starts as NaN."""
    N, q_ct, H, W = q.shape
    Nkv, kv_ct = k.shape[:2]
    out = torch.full((N, heads * dh, H, W), float("nan"), device=DEV)
    at = lambda t, c: ptr(t) + 4 * c * H * W
    _lib.check(_lib.lib().gencomm_quad_attn_fwd(at(q, q_coff), at(k, k_coff), at(v, v_coff), ptr(table), ptr(out), N, Nkv, heads, dh, H, W, q_ct, kv_ct,
                                                int(grid), stream_ptr(q.device)), "gencomm_quad_attn_fwd")
    return out


@pytest.mark.parametrize("heads", R.QUAD_HEADS)
def test_quad_attention_kernel_vs_float64(heads):
    """dim_head 32, both partitions, every map of the table (one group; 4 x 6; 15 groups; more groups than one workgroup holds; X != Y
    everywhere, so a swapped partition shows). Cross form: three tensors, no bias, Nkv = N = 2 and Nkv = 1 with N = 3. Self form: q | k | v
    blocks of one tensor and a bias table, read in the restatement through the ``rel_pos_indices`` buffer the module registers, so the
    kernel's index arithmetic is checked against the buffer. Queries are scaled by 3: scores of a few units, a softmax far from uniform."""
    dh, inner = 32, heads * 32
    rng = np.random.RandomState(700 + heads)
    index = Attention(inner, dh, 0.0, 2).rel_pos_indices
    assert tuple(index.shape) == (4, 4)
    draw = lambda *s: rng.standard_normal(s).astype(np.float32)
    poison_allocator()
    for H, W in R.QUAD_MAPS:
        for grid in (0, 1):
            for N, Nkv in ((2, 2), (3, 1)):                                     # cross attention
                q, k, v = 3.0 * draw(N, inner, H, W), draw(Nkv, inner, H, W), draw(Nkv, inner, H, W)
                got = quad_attn_hip(*(torch.from_numpy(t).to(DEV) for t in (q, k, v)), None, heads, dh, grid).cpu().numpy()
                ref = R.quad_attention(*(torch.from_numpy(t).double() for t in (q, k, v)), None, None, heads, dh, bool(grid)).numpy()
                what = f"quad attention, cross, heads {heads} {H}x{W} grid {grid} N {N} Nkv {Nkv}"
                assert np.isfinite(got).all(), what + ": output elements left unwritten"
                assert_close(got, ref, 1e-4, 1e-5, what)
            qkv = draw(2, 3 * inner, H, W)                                      # self attention from one to_qkv output
            qkv[:, :inner] *= 3.0
            table = rng.uniform(-1.0, 1.0, (9, heads)).astype(np.float32)
            t_dev = torch.from_numpy(qkv).to(DEV)
            got = quad_attn_hip(t_dev, t_dev, t_dev, torch.from_numpy(table).to(DEV), heads, dh, grid, 0, inner, 2 * inner).cpu().numpy()
            q64, k64, v64 = torch.from_numpy(qkv).double().chunk(3, dim=1)
            ref = R.quad_attention(q64, k64, v64, torch.from_numpy(table).double(), index, heads, dh, bool(grid)).numpy()
            what = f"quad attention, self + bias, heads {heads} {H}x{W} grid {grid}"
            assert np.isfinite(got).all(), what + ": output elements left unwritten"
            assert_close(got, ref, 1e-4, 1e-5, what)


@pytest.mark.parametrize("dh", [16, 64])
def test_quad_attention_other_head_widths(dh):
    """dim_head 16 and 64 are the same kernel at another channel count: one map, both partitions, cross form with a broadcast ego."""
    rng = np.random.RandomState(800 + dh)
    heads, H, W = 2, 6, 10
    q, k, v = (rng.standard_normal((n, heads * dh, H, W)).astype(np.float32) for n in (3, 1, 1))
    q *= 3.0
    for grid in (0, 1):
        got = quad_attn_hip(*(torch.from_numpy(t).to(DEV) for t in (q, k, v)), None, heads, dh, grid).cpu().numpy()
        ref = R.quad_attention(*(torch.from_numpy(t).double() for t in (q, k, v)), None, None, heads, dh, bool(grid)).numpy()
        assert np.isfinite(got).all()
        assert_close(got, ref, 1e-4, 1e-5, f"quad attention dim_head {dh} grid {grid}")


@pytest.mark.parametrize("src,dst", R.RESIZE_CASES)
def test_resize_kernel_vs_torch_float64(src, dst):
    """Against torch's CPU F.interpolate(mode='bilinear', align_corners=False) in float64; a resize to the input's own size returns
    the input's bits."""
    rng = np.random.RandomState(900 + 10 * src[0] + dst[0])
    x = rng.standard_normal((2, 3, *src)).astype(np.float32)
    y = torch.full((2, 3, *dst), float("nan"), device=DEV)
    xd = torch.from_numpy(x).to(DEV)
    _lib.check(_lib.lib().gencomm_resize_bilinear_fwd(ptr(xd), ptr(y), 2, 3, *src, *dst, stream_ptr(xd.device)), "gencomm_resize_bilinear_fwd")
    got = y.cpu().numpy()
    ref = R.resize(torch.from_numpy(x).double(), dst).numpy()
    assert np.isfinite(got).all(), "output elements left unwritten"
    assert_close(got, ref, 1e-4, 1e-5, f"bilinear resize {src} -> {dst}")
    if src == dst:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32)), "a resize to the same size must return the input's bits"


def test_leaky_relu_layer_vs_torch_float64():
    """Conv2d(16, 16, 3, padding 1) + eval-mode BatchNorm + LeakyReLU(0.01) as one launch (act 4), against torch in float64; the
    pre-activations are negative for about half of the elements."""
    torch.manual_seed(0)
    conv, bn = torch.nn.Conv2d(16, 16, 3, padding=1), torch.nn.BatchNorm2d(16).eval()
    rng = np.random.RandomState(41)
    with torch.no_grad():
        for t, v in ((conv.weight, 0.1 * rng.standard_normal((16, 16, 3, 3))), (conv.bias, 0.1 * rng.standard_normal(16)),
                     (bn.weight, rng.uniform(0.5, 1.5, 16)), (bn.bias, 0.1 * rng.standard_normal(16)),
                     (bn.running_mean, 0.1 * rng.standard_normal(16)), (bn.running_var, rng.uniform(0.5, 2.0, 16))):
            t.copy_(torch.from_numpy(np.asarray(v, np.float32)))
    x = rng.standard_normal((2, 16, 6, 10)).astype(np.float32)
    c64, b64 = torch.nn.Conv2d(16, 16, 3, padding=1).double(), torch.nn.BatchNorm2d(16).double().eval()
    c64.load_state_dict(conv.state_dict()), b64.load_state_dict(bn.state_dict())
    with torch.no_grad():
        pre = b64(c64(torch.from_numpy(x).double()))
        ref = F.leaky_relu(pre, 0.01).numpy()
        assert 0.3 < float((pre < 0).double().mean()) < 0.7
        poison_allocator()
        got = _conv_bn_act(torch.from_numpy(x).to(DEV), conv.to(DEV), bn.to(DEV), 4).cpu().numpy()
    assert_close(got, ref, 1e-4, 1e-5, "conv3x3 + BatchNorm + LeakyReLU(0.01)")


def _two_bars(out, g, name, tag):
    """Every element against the reference's float32 output, and the rms-relative error against the reference's float64 output within
    twice the reference float32 run's own (floored at 1e-6): the bars of test_gpu_cobevt.py::test_module_vs_reference_golden."""
    y32, y64, e_ref = golden_pair(g, name, tag)
    e_hip = R.rel_rms(out, y64)
    print(f"mpda case {tag} {name}: rms-relative error against float64: HIP {e_hip:.3e}, reference float32 {e_ref:.3e}; "
          f"max abs against the float32 output {np.abs(out - y32).max():.3e}")
    assert abs(R.rel_rms(y32, y64) - e_ref) <= 1e-3 * e_ref + 1e-12          # the stored yardstick is the float32 run's own error
    assert_close(out, y32, 1e-4, 1e-5, f"MPDA HIP vs reference golden, case {tag}, {name}")
    assert e_hip <= max(2.0 * e_ref, 1e-6), (tag, name, e_hip, e_ref)


@pytest.fixture(scope="module")
def g():
    return load_case("mpda")


@pytest.mark.parametrize("tag", list(R.CASES))
def test_modules_vs_reference_golden(g, tag):
    """LearnableResizer, CrossDomainFusionEncoder (one ego map broadcast by the kernel; the reference's repeated ego gives the same
    result), DAImgHead and MPDAAlign against the reference's own outputs."""
    c = R.CASES[tag]
    res, cdt, da, al = (m.to(DEV) for m in package_modules(tag))
    ego, cav, cdt_cav, x = (None if a is None else torch.from_numpy(a).to(DEV) for a in R.case_inputs(tag))
    with torch.no_grad():
        poison_allocator()
        _two_bars(res(ego, cav).cpu().numpy(), g, "resizer", tag)
        poison_allocator()
        one = cdt(ego, cdt_cav)
        _two_bars(one.cpu().numpy(), g, "cdt", tag)
        rep = cdt(ego.repeat(cdt_cav.shape[0], 1, 1, 1), cdt_cav)          # the ego projected per collaborator: other launch shapes
        assert_close(one.cpu().numpy(), rep.cpu().numpy(), 1e-5, 1e-6, f"case {tag}: broadcast ego vs repeated ego")
        _two_bars(da(cdt_cav).cpu().numpy(), g, "da", tag)
        if c["record_len"]:
            poison_allocator()
            feats, logits = al(x, torch.tensor(c["record_len"]))
            _two_bars(feats.cpu().numpy(), g, "align", tag)
            _two_bars(logits.cpu().numpy(), g, "logits", tag)
            if c["rebuttal"]:
                assert torch.equal(feats, x)


def test_aligner_is_deterministic_and_skips_nothing_it_returns():
    """Two runs of MPDAAlign give the same bits with NaNs planted in the allocator's free memory before each; the ego rows are the
    input's bits; a batch of ego-only scenes returns its input and the classifier's logits."""
    tag = "c32"
    c = R.CASES[tag]
    al = package_modules(tag)[3].to(DEV)
    x = torch.from_numpy(R.case_inputs(tag)[3]).to(DEV)
    with torch.no_grad():
        poison_allocator()
        a = [t.clone() for t in al(x, c["record_len"])]
        poison_allocator()
        b = [t.clone() for t in al(x, c["record_len"])]
        assert all(torch.isfinite(t).all() for t in a)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0][[0, 1, 4]], x[[0, 1, 4]]) and not torch.equal(a[0][2], x[2])
        feats, logits = al(x[:2], [1, 1])
        assert torch.equal(feats, x[:2])
        assert_close(logits.cpu().numpy(), a[1][:2].cpu().numpy(), 1e-5, 1e-6, "logits of the two egos alone")
