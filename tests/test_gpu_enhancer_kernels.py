"""The Enhancer's kernels (csrc/enhancer_kernels.h) one stage at a time through gencomm_enhancer_fwd_stages, each against the same stage in
float64 (tests/enhancer_reference.py, pinned on the CPU by test_enhancer_reference.py).

A case fills the whole workspace with NaN bit patterns, writes ONE stage's input into it (offsets from gencomm_enhancer_workspace_layout),
runs that stage alone and reads its output: a stage that reads scratch nothing wrote, or leaves an element out, shows as NaN. The truth is
the float64 stage applied to the input the kernel actually read, so every bound is per stage.

Criterion (the project's, as test_gpu_msgext_kernels.py::_check): relative rms error of the kernel against the truth <= max(2 x that of
the same stage in float32 on the CPU, 1e-6) -- on the whole output AND separately on the image's border ring, on the pixels of the last
partial tile in x and in y, and on each agent, so that a wrong edge is not averaged away. Matrix stages run under arith = split and
arith = f32 and additionally meet the bar of test_gpu_conv_h3.py::_check between the two (relative to max |truth|: e_split <=
max(2 e_f32, 4e-7) and e_split <= 3e-6).

Every case asserts the exact launch log (GC_KLOG names in enhancer_host.h); the selection condition of enhancer_enqueue that the shape was
chosen by is quoted in the docstring."""
import os

import numpy as np
import pytest
import torch

import enhancer_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F16_0, F16_1, F32_0, F32_1 = "gemm_f16s_mfma_kernel<0>", "gemm_f16s_mfma_kernel<1>", "gemm_f32_mfma_kernel<0>", "gemm_f32_mfma_kernel<1>"
WSCALE, DWGATE = "enh_wscale_kernel", "enh_dwgate_kernel<8>"
PC_H, PC_F = "enh_prep_pconv_h_kernel", "enh_prep_pconv_kernel"


def _lib():
    from gencomm_amd import _lib as l
    return l


class Stages:
    """One (n, C, H, W) geometry: packed parameters, a NaN-filled workspace, named views into it, and run(first, last)."""

    def __init__(self, sd, n, C, H, W):
        from gencomm_amd.runtime import PackedParams
        l = _lib()
        self.n, self.C, self.H, self.W = n, C, H, W
        packed = PackedParams(l.enhancer_param_table(C), l.check_size(l.lib().gencomm_enhancer_raw_floats(C), "gencomm_enhancer_raw_floats"))
        packed.update({k: v.to(DEV) for k, v in sd.items()})
        self.raw = packed.flat
        self.ws = torch.empty(l.check_size(l.lib().gencomm_enhancer_workspace_bytes(n, C, H, W), "gencomm_enhancer_workspace_bytes"), dtype=torch.uint8, device=DEV)
        self.ws.fill_(0xFF)                               # every float of the workspace a NaN
        self.off = l.enhancer_workspace_layout(n, C, H, W)
        ch = {"Y": C, "Z": C, "Zc": C // 4, "Hd": 4 * C, "G": 2 * C, "O": C}
        self.shape = {k: (n, H, W, c) for k, c in ch.items()}
        self.shape["colsum"] = self.shape["gate"] = (n, C)

    def view(self, name):
        numel = int(np.prod(self.shape[name]))
        return self.ws[self.off[name]:self.off[name] + 4 * numel].view(torch.float32).view(self.shape[name])

    def put(self, name, t):
        self.view(name).copy_(t.to(torch.float32))

    def get(self, name):
        return self.view(name).cpu()

    def run(self, first, last, x=None, out=None):
        from gencomm_amd.runtime import stream_ptr
        l = _lib()
        with l.kernel_log() as kl:
            l.check(l.lib().gencomm_enhancer_fwd_stages(self.raw.data_ptr(), x.data_ptr() if x is not None else None, out.data_ptr() if out is not None else None,
                                                        self.n, self.C, self.H, self.W, self.ws.data_ptr(), self.ws.numel(), first, last,
                                                        stream_ptr(torch.device(DEV))), "gencomm_enhancer_fwd_stages")
        torch.cuda.synchronize()
        return dict(kl.counts)


def _crit(what, got, truth, yard, subsets=None):
    """The criterion on the whole tensor and on every subset (name -> index into the leading axes)."""
    assert torch.isfinite(got).all(), f"{what}: output elements left unwritten, or computed from workspace nothing wrote"
    worst = 0.0
    for name, idx in [("whole", None)] + list((subsets or {}).items()):
        g, t, y = (got, truth, yard) if idx is None else (got[idx], truth[idx], yard[idx])
        e_k, e_y = R.rel_rms(g.numpy(), t.numpy()), R.rel_rms(y.numpy(), t.numpy())
        print(f"{what} [{name}]: relative rms error against float64: kernel {e_k:.3e}, float32 ATen {e_y:.3e}")
        assert e_k <= max(2.0 * e_y, 1e-6), (what, name, e_k, e_y)
        worst = max(worst, e_k)
    return worst


def _bar(what, y_split, y_f32, truth):
    """test_gpu_conv_h3.py::_check: the f16-pipe kernel beside the exact-fp32 kernel, relative to max |truth|."""
    scale = max(float(truth.abs().max()), 1e-300)
    e3, e32 = float((y_split.double() - truth).abs().max()) / scale, float((y_f32.double() - truth).abs().max()) / scale
    print(f"{what}: max error / max |truth|: split {e3:.3e}, f32 kernel {e32:.3e}")
    assert e3 <= max(2.0 * e32, 4e-7) and e3 <= 3e-6, (what, e3, e32)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _gemm_subsets(n, H, W, N):
    """GEMM tiles are 128 flattened pixels x 64 columns: the last partial M tile, the last partial N tile (as a column slice), each agent."""
    s = R.subsets(n, H, W, 1, 1)
    s.pop("border ring")
    HW = H * W
    if HW % 128:
        m = torch.zeros(n, HW, dtype=torch.bool)
        m[:, HW - HW % 128:] = True
        s["last partial M tile"] = m.view(n, H, W)
    if N % 64:
        s["last partial N tile"] = (Ellipsis, slice(N - N % 64, N))
    return s


# ---- K1: the two LayerNorms ------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(64, 5, 7), (64, 7, 10), (64, 21, 37)] + [(C, H, W) for C in (16, 24, 40, 128, 256) for H, W in ((5, 7), (21, 37))]


def _ln_input(kind, n, C, H, W):
    x = _randn(C + H, n, C, H, W)
    if kind == "mean1000":
        x = x + 1000.0
    elif kind == "constant_pixel":
        x[:, :, 0, 0] = 3.0                               # variance 0: LayerNorm1 gives its bias there (the eps path)
        x[:, :, H - 1, W - 1] = 0.0
    elif kind == "1e5":
        x = x * 1e5
    elif kind == "1e-6":
        x = x * 1e-6
    return x


# enh_ln64_kernel at mean 1000, std 1 misses the criterion on Z (measured on an MI355X, relative rms against float64, kernel / float32
# ATen): 5 x 7: 5.11e-5 / 2.07e-5, 7 x 10: 5.55e-5 / 2.01e-5, 21 x 37: 5.86e-5 / 1.99e-5 -- 2.5 to 2.9 times the yardstick where 2 is
# allowed (Y: 1.1e-7 / 4.1e-8, inside the 1e-6 floor). The lane adds its 64 channels one after the other in fp32: at |x| ~ 1000 the mean
# of LayerNorm1 is off by ~1e-4, every channel of Y moves by that times gamma / std, and LayerNorm2 (std ~ 2) turns it into ~5e-5 of Z.
# enh_ln_kernel (four partial sums per pixel) meets the bar on the same inputs (C = 128: 2.54e-5 / 1.97e-5). The kernel is on the benchmark
# path and is not changed with these tests: strict xfail, so that a kernel that starts to pass is noticed.
_LN64_MEAN1000 = pytest.mark.xfail(strict=True, reason="enh_ln64_kernel: sequential fp32 channel sum, Z error 2.5-2.9 x the float32 yardstick at mean 1000")
LN_CASES = [pytest.param(C, H, W, kind, marks=[_LN64_MEAN1000] if (C == 64 and kind == "mean1000") else [])
            for C, H, W in LN_SHAPES for kind in ("normal", "mean1000", "constant_pixel", "1e5", "1e-6")]


@pytest.mark.parametrize("C,H,W,kind", LN_CASES)
def test_k1_layernorms_vs_float64(C, H, W, kind):
    """`if (C == 64) enh_ln64_kernel<<<(HW + 255) / 256, n>>> else enh_ln_kernel<<<(HW + 63) / 64, n>>>`. enh_ln64_kernel: a wave owns 64
    pixels, HW = 35: one partial wave and three wholly out of range; 70: a full wave, a partial one (6 lanes), two out of range; 777 = 3
    workgroups + 9 pixels. enh_ln_kernel: 64 pixels per workgroup, channels dealt to four quarter-workgroups (C = 24, 40: off the power-of-two
    grid; C = 256: 68 KB of LDS, the hipFuncSetAttribute branch). Y = x + LN1(x), Z = LN2(Y); Zc is the compact copy of Z's first C / 4
    channels and must be bit-equal to them. At |x| ~ 1e-6 the variance is far below eps = 1e-5: LN1(x) ~ x / sqrt(eps)."""
    n = 2
    sd = R.random_sd(C, 11 + C)
    x = _ln_input(kind, n, C, H, W)
    st = Stages(sd, n, C, H, W)
    log = st.run(1, 1, x=x.to(DEV).contiguous())
    assert log == {"enh_ln64_kernel" if C == 64 else "enh_ln_kernel": 1}, log
    Y64, Z64 = R.ln(R.cast(sd, torch.float64), x.double())
    Y32, Z32 = R.ln(R.cast(sd, torch.float32), x)
    Y, Z, Zc = st.get("Y"), st.get("Z"), st.get("Zc")
    sub = R.subsets(n, H, W, 64, 64)
    sub.pop("border ring")
    HW = H * W
    if HW % 64:
        m = torch.zeros(n, HW, dtype=torch.bool)
        m[:, HW - HW % 64:] = True
        sub["last partial group of 64 pixels"] = m.view(n, H, W)
    if kind == "constant_pixel":
        m = torch.zeros(n, H, W, dtype=torch.bool)
        m[:, 0, 0] = True
        sub["the constant pixel"] = m
    _crit(f"K1 Y C {C} {H}x{W} {kind}", Y, Y64, Y32, sub)
    _crit(f"K1 Z C {C} {H}x{W} {kind}", Z, Z64, Z32, sub)
    assert torch.equal(Zc, Z[..., :C // 4])


# ---- K2: the partial convolution ---------------------------------------------------------------------------------------------------------
def _pconv_weights(sd, kind, dc):
    w = sd[R.PM + "partial_conv3.weight"]
    if kind == "rows":                                    # output rows spread over 2^-12 .. 1
        w = w * (2.0 ** (-12.0 * torch.arange(dc).float() / max(dc - 1, 1))).view(dc, 1, 1, 1)
    elif kind == "zero":
        w = torch.zeros_like(w)
    sd[R.PM + "partial_conv3.weight"] = w.contiguous()
    return sd


def _run_pconv(modes, arith, sd, Zln, kernels):
    n, H, W, C = Zln.shape
    dc = C // 4
    modes(arith=arith)
    st = Stages(sd, n, C, H, W)
    Zd = Zln.to(DEV)
    st.put("Z", Zd)
    st.put("Zc", Zd[..., :dc])
    log = st.run(2, 2)
    assert log == {k: 1 for k in kernels}, (arith, log)
    assert torch.equal(st.view("Z")[..., dc:], Zd[..., dc:]), "channels >= dc must pass the partial convolution untouched"
    return st.view("Z")[..., :dc].cpu()


def _check_pconv(what, got, Zln, sd, tw, th, kind):
    n, H, W, C = Zln.shape
    dc = C // 4
    t64 = R.pconv(R.cast(sd, torch.float64), Zln.double())[..., :dc]
    t32 = R.pconv(R.cast(sd, torch.float32), Zln)[..., :dc]
    if kind == "zero":
        assert torch.equal(got, torch.zeros_like(got)), what
    elif kind == "rows":                                  # judged per output channel: each row has its own magnitude
        for c in sorted({0, dc // 2, dc - 1}):
            _crit(f"{what} channel {c}", got[..., c], t64[..., c], t32[..., c], R.subsets(n, H, W, tw, th))
    else:
        _crit(what, got, t64, t32, R.subsets(n, H, W, tw, th))
    return t64


PCONV_MAPS = [(2, 21, 37), (1, 1, 5)]


@pytest.mark.parametrize("kind", ["random", "rows", "zero"])
@pytest.mark.parametrize("n,H,W", PCONV_MAPS)
@pytest.mark.parametrize("C", [64, 128, 256])
def test_k2_pconv_f16_pipe_narrow_tiles_vs_float64(modes, C, n, H, W, kind):
    """`m.split() && dc in {16, 32, 64}` -> the f16 pipe; `wide = dc <= 32 && cdiv(W, 32) cdiv(H, 16) n >= 256`: 2 * 2 * 2 = 8 and 1
    workgroups, so enh_pconv_h_kernel<16> (C = 256: dc = 64 is never wide; 104 KB of LDS). Under arith = f32 the same maps run
    enh_pconv_kernel<16,16> (dc <= 32) and enh_pconv_kernel<16,8> (dc = 64). 21 x 37: partial 16 x 16 tiles in x and y (and partial
    16 x 8 ones); 1 x 5: one row, every pixel on the border."""
    sd = _pconv_weights(R.random_sd(C, 21 + C), kind, C // 4)
    Zln = _randn(C + H, n, H, W, C)
    f32_kernel = "enh_pconv_kernel<16,16>" if C // 4 <= 32 else "enh_pconv_kernel<16,8>"
    ys = _run_pconv(modes, "split", sd, Zln, (PC_H, "enh_pconv_h_kernel<16>"))
    yf = _run_pconv(modes, "f32", sd, Zln, (PC_F, f32_kernel))
    t64 = _check_pconv(f"K2 enh_pconv_h_kernel<16> C {C} n {n} {H}x{W} {kind}", ys, Zln, sd, 16, 16, kind)
    _check_pconv(f"K2 {f32_kernel} C {C} n {n} {H}x{W} {kind}", yf, Zln, sd, 16, 16 if C // 4 <= 32 else 8, kind)
    if kind == "random":
        _bar(f"K2 C {C} n {n} {H}x{W}", ys, yf, t64)


@pytest.mark.parametrize("C", [64, 128])
def test_k2_pconv_f16_pipe_wide_tiles_ragged_edges_vs_float64(modes, C):
    """enh_pconv_h_kernel<32> needs dc <= 32 and cdiv(W, 32) cdiv(H, 16) n >= 256: n = 8, H = 50, W = 250 gives 8 * 4 * 8 = 256 exactly,
    with a ragged right edge (250 = 7 * 32 + 26: the last tile's second 16-pixel column group holds 10 pixels) and a ragged bottom
    (50 = 3 * 16 + 2). Only stage 2 runs, so the (NaN-filled) hidden tensors of this large map are never touched."""
    n, H, W = 8, 50, 250
    sd = R.random_sd(C, 31 + C)
    Zln = _randn(C, n, H, W, C)
    ys = _run_pconv(modes, "split", sd, Zln, (PC_H, "enh_pconv_h_kernel<32>"))
    yf = _run_pconv(modes, "f32", sd, Zln, (PC_F, "enh_pconv_kernel<16,16>"))
    t64 = _check_pconv(f"K2 enh_pconv_h_kernel<32> C {C} n {n} {H}x{W}", ys, Zln, sd, 32, 16, "random")
    _bar(f"K2 wide C {C}", ys, yf, t64)


@pytest.mark.parametrize("kind", ["random", "rows", "zero"])
@pytest.mark.parametrize("n,H,W", PCONV_MAPS)
@pytest.mark.parametrize("C", [16, 32, 40, 192, 320])
def test_k2_pconv_fp32_kernels_vs_float64(modes, C, n, H, W, kind):
    """dc = C / 4 = 4, 8, 10, 48, 80 is none of {16, 32, 64}: the fp32 kernels in BOTH arithmetic modes. `dc <= 32` ->
    enh_pconv_kernel<16,16> (dc = 10: the `ob + o < dc` tail of the 16-channel output block; dc = 4, 8: a block mostly tail), else
    enh_pconv_kernel<16,8> (dc = 48; dc = 80: 10 * 18 * 81 * 4 = 58320 B of LDS > 48 KB, the hipFuncSetAttribute branch)."""
    dc = C // 4
    sd = _pconv_weights(R.random_sd(C, 41 + C), kind, dc)
    Zln = _randn(C + W, n, H, W, C)
    kernel, th = ("enh_pconv_kernel<16,16>", 16) if dc <= 32 else ("enh_pconv_kernel<16,8>", 8)
    for arith in ("split", "f32"):
        y = _run_pconv(modes, arith, sd, Zln, (PC_F, kernel))
        _check_pconv(f"K2 {kernel} C {C} n {n} {H}x{W} {kind} arith {arith}", y, Zln, sd, 16, th, kind)


# ---- K3 / K5: the two GEMMs ----------------------------------------------------------------------------------------------------------------
GEMM_C = [16, 24, 40, 72, 128]
GEMM_MAPS = [(21, 37), (5, 7)]


@pytest.mark.parametrize("H,W", GEMM_MAPS)
@pytest.mark.parametrize("C", GEMM_C)
def test_k3_linear1_gelu_both_gemms_vs_float64(modes, C, H, W):
    """K3 off C = 64: `m.split() && (C & 3) == 0` -> gemm_f16s_mfma_kernel<0>, else gemm_f32_mfma_kernel<0>; M = HW per agent in tiles of
    128 (777 = 6 * 128 + 9, 35: one partial tile), N = 4C in tiles of 64 (C = 24, 40, 72: 96, 160, 288 -- a partial N tile; C = 16: N = 64),
    K = C in chunks of 32 (24, 40, 72: a partial last chunk; 16: less than one chunk). The split structure first runs enh_wscale_kernel."""
    n = 2
    sd = R.random_sd(C, 51 + C)
    Z = _randn(C * H, n, H, W, C)
    t64, t32 = R.linear1(R.cast(sd, torch.float64), Z.double()), R.linear1(R.cast(sd, torch.float32), Z)
    got = {}
    for arith, want in (("split", {WSCALE: 1, F16_0: 1}), ("f32", {F32_0: 1})):
        modes(arith=arith, enh_fuse=0)
        st = Stages(sd, n, C, H, W)
        st.put("Z", Z)
        log = st.run(3, 3)
        assert log == want, (arith, log)
        got[arith] = st.get("Hd")
        _crit(f"K3 {list(want)[-1]} C {C} {H}x{W}", got[arith], t64, t32, _gemm_subsets(n, H, W, 4 * C))
    _bar(f"K3 C {C} {H}x{W}", got["split"], got["f32"], t64)


def _check_colsum(what, colsum, O, HW):
    """The pool sums against the float64 sum of the kernel's OWN O: |colsum - sum| <= HW 2^-24 sum |O| per channel holds for any order of
    fp32 additions (and of the atomics); at HW <= 1000 it is more than ten times below one average pixel's share sum |O| / HW, so a
    dropped or doubled pixel fails."""
    assert torch.isfinite(colsum).all(), what
    exact, mag = O.double().sum((1, 2)), O.double().abs().sum((1, 2))
    err = (colsum.double() - exact).abs()
    print(f"{what}: colsum error / (HW 2^-24 sum |O|): worst {float((err / (HW * 2.0 ** -24 * mag)).max()):.3f}")
    assert HW * HW * 2.0 ** -24 * 10 < 1.0 and (err <= HW * 2.0 ** -24 * mag).all(), what


@pytest.mark.parametrize("H,W", GEMM_MAPS)
@pytest.mark.parametrize("C", GEMM_C)
def test_k5_linear2_residual_poolsums_both_gemms_vs_float64(modes, C, H, W):
    """K5 off the fully fused structure: `m.split() && (hid & 3) == 0` -> gemm_f16s_mfma_kernel<1>, else gemm_f32_mfma_kernel<1>;
    N = C (16, 24, 40: N < 64; 72: a partial second N tile; 128), K = 2C (48, 80, 144: a partial last chunk of 32). The epilogue adds the
    residual Y and accumulates the column sums (cleared by the stage itself: the workspace holds NaN)."""
    n = 2
    sd = R.random_sd(C, 61 + C)
    G, Y = _randn(C + H, n, H, W, 2 * C), _randn(C + W, n, H, W, C) * 2.0
    t64, t32 = R.linear2(R.cast(sd, torch.float64), G.double(), Y.double()), R.linear2(R.cast(sd, torch.float32), G, Y)
    got = {}
    for arith, want in (("split", {WSCALE: 1, F16_1: 1}), ("f32", {F32_1: 1})):
        modes(arith=arith, enh_fuse=0)
        st = Stages(sd, n, C, H, W)
        st.put("G", G)
        st.put("Y", Y)
        log = st.run(5, 5)
        assert log == want, (arith, log)
        got[arith] = st.get("O")
        _crit(f"K5 {list(want)[-1]} C {C} {H}x{W}", got[arith], t64, t32, _gemm_subsets(n, H, W, C))
        _check_colsum(f"K5 {list(want)[-1]} C {C} {H}x{W}", st.get("colsum"), got[arith], H * W)
    _bar(f"K5 C {C} {H}x{W}", got["split"], got["f32"], t64)


# ---- K3 + K4 (+ K5): the fused front kernel and the separate structure on the same inputs --------------------------------------------------
FRONT_LOG = {0: {WSCALE: 1, F16_0: 1, DWGATE: 1, F16_1: 1},
             1: {WSCALE: 1, "enh_prep_front_kernel": 1, "enh_front_h_kernel<false>": 1, F16_1: 1},
             2: {WSCALE: 1, "enh_prep_front_kernel": 1, "enh_prep_back_kernel": 1, "enh_front_h_kernel<true>": 1}}


def _front_truth(sd, Z, Y, dt):
    s = R.cast(sd, dt)
    G = R.dwgate(s, R.linear1(s, Z.to(dt)))
    return G, R.linear2(s, G, Y.to(dt))


@pytest.mark.parametrize("fuse", [0, 1, 2])
@pytest.mark.parametrize("H,W", [(1, 1), (8, 8), (9, 9), (1, 70), (21, 37)])
def test_front_structures_vs_float64(modes, H, W, fuse):
    """C = 64, split arithmetic: `enh_fuse_level = MODE_ENH_FUSE` -> 0: K3, enh_dwgate_kernel, K5; 1: enh_front_h_kernel<false> (K3 + K4 on
    8 x 8 tiles with the Linear1 outputs of the 10 x 10 halo region recomputed), K5; 2: enh_front_h_kernel<true> (+ Linear2, residual, pool
    sums). The Linear1 bias is of order 1, so GELU(bias) -- what a zero token gives on a halo pixel outside the image -- is far from the
    zero the depthwise convolution must see there (test_enhancer_reference.py pins that the two differ by > 1e-3 at a corner). 1 x 1: all
    halo; 8 x 8: one full tile; 9 x 9: one-pixel partial tiles in x and y; 1 x 70: a single row over nine tiles; 21 x 37: partial tiles
    with agents n = 3. All structures answer to the same truth: G (where it reaches memory), O, and the pool sums."""
    n, C = 3, 64
    sd = R.random_sd(C, 71, bias1=1.0)
    Z, Y = _randn(H * 100 + W, n, H, W, C), _randn(H * 100 + W + 1, n, H, W, C) * 2.0
    G64, O64 = _front_truth(sd, Z, Y, torch.float64)
    G32, O32 = _front_truth(sd, Z, Y, torch.float32)
    modes(arith="split", enh_fuse=fuse)
    st = Stages(sd, n, C, H, W)
    st.put("Z", Z)
    st.put("Y", Y)
    log = st.run(3, 5)
    assert log == FRONT_LOG[fuse], log
    sub = R.subsets(n, H, W, 8, 8)
    name = {0: "K3, enh_dwgate_kernel, K5", 1: "enh_front_h_kernel<false>, K5", 2: "enh_front_h_kernel<true>"}[fuse]
    if fuse < 2:
        _crit(f"{name} G {H}x{W}", st.get("G"), G64, G32, sub)
    O = st.get("O")
    _crit(f"{name} O {H}x{W}", O, O64, O32, sub)
    _check_colsum(f"{name} {H}x{W}", st.get("colsum"), O, H * W)


@pytest.mark.parametrize("C,H,W", [(24, 3, 5), (24, 4, 13), (64, 21, 37), (16, 9, 9)])
def test_k4_dwgate_kernel_alone_vs_float64(modes, C, H, W):
    """enh_dwgate_kernel<8> (every structure but the fused ones): a thread slides a 3 x 3 window along a strip of 8 pixels of one hidden
    channel: W = 5: one strip cut short by `if (x >= W) break`, W = 13 = 8 + 5: a full strip and a tail, W = 37 = 4 * 8 + 5. The hidden
    tensor is written by the test (x1 of order 1 everywhere, so zero padding matters on the ring)."""
    n = 2
    sd = R.random_sd(C, 81 + C)
    Hd = _randn(C + W, n, H, W, 4 * C) + 0.5
    modes(arith="split", enh_fuse=0)
    st = Stages(sd, n, C, H, W)
    st.put("Hd", Hd)
    log = st.run(4, 4)
    assert log == {DWGATE: 1}, log
    _crit(f"K4 enh_dwgate_kernel<8> C {C} {H}x{W}", st.get("G"), R.dwgate(R.cast(sd, torch.float64), Hd.double()), R.dwgate(R.cast(sd, torch.float32), Hd),
          R.subsets(n, H, W, 8, 1))


# ---- K6, K7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "constant", "large"])
@pytest.mark.parametrize("C", [16, 24, 64, 256])
def test_k6_gate_kernel_vs_float64(C, kind):
    """enh_gate_kernel: one workgroup of 256 per agent, channels strided over the threads (C = 16, 24: most threads idle, a partial wave
    in the block sums; C = 256: one channel each). colsum is written by the test: random pool sums; constant vectors (all zero for agent
    0: fc1 gives zeros, the LayerNorm sees variance 0 and returns its bias; all 5 HW for agent 1); large sums with fc2 x 30, so that the
    sigmoid saturates to both ends."""
    n, HW = 3, 777
    sd = R.random_sd(C, 91 + C)
    cs = _randn(C, n, C) * HW
    if kind == "constant":
        cs[0], cs[1] = 0.0, 5.0 * HW
    elif kind == "large":
        cs = cs * 1e3
        sd[R.PS + "fc2.weight"] = sd[R.PS + "fc2.weight"] * 30.0
    st = Stages(sd, n, C, 21, 37)
    st.put("colsum", cs)
    log = st.run(6, 6)
    assert log == {"enh_gate_kernel": 1}, log
    t64, t32 = R.gate(R.cast(sd, torch.float64), cs.double(), HW), R.gate(R.cast(sd, torch.float32), cs, HW)
    if kind == "large":
        assert float(t64.max()) > 1 - 1e-6 and float(t64.min()) < 1e-6
    _crit(f"K6 enh_gate_kernel C {C} {kind}", st.get("gate"), t64, t32, {f"agent {a}": a for a in range(n)})


@pytest.mark.parametrize("H,W", [(5, 7), (21, 37)])
@pytest.mark.parametrize("C", [24, 64])
def test_k7_scale_transpose_is_exact(C, H, W):
    """enh_scale_transpose_kernel: 32 pixels x all channels per workgroup through LDS (35 = 32 + 3, 777 = 24 * 32 + 9: partial last
    groups). out[n][c][p] = O[n][p][c] * gate[n][c] is ONE float32 rounding: bit-equal to the float32 product, transposed."""
    n = 2
    st = Stages(R.random_sd(C, 5), n, C, H, W)
    O, gt = _randn(C + H, n, H, W, C), torch.rand(n, C, generator=torch.Generator().manual_seed(C))
    st.put("O", O)
    st.put("gate", gt)
    out = torch.full((n, C, H, W), NAN, device=DEV)
    log = st.run(7, 7, out=out)
    assert log == {"enh_scale_transpose_kernel": 1}, log
    assert torch.equal(out.cpu(), R.scale_out(O, gt))


# ---- the whole module through the stage entry, and its argument checks ----------------------------------------------------------------------
@pytest.mark.parametrize("C,fuse", [(64, 2), (64, 0), (40, 2)])
def test_all_stages_in_one_call_equal_the_module_entry(modes, C, fuse):
    """first_stage = 1, last_stage = 7 is gencomm_enhancer_fwd: the same launches, the full launch log."""
    from gencomm_amd.runtime import stream_ptr
    n, H, W = 2, 9, 13
    sd = R.random_sd(C, 3)
    x = _randn(C, n, C, H, W).to(DEV)
    modes(arith="split", enh_fuse=fuse)
    st = Stages(sd, n, C, H, W)
    out = torch.full((n, C, H, W), NAN, device=DEV)
    log = st.run(1, 7, x=x, out=out)
    front = dict(FRONT_LOG[fuse if C == 64 else 0])
    pc = {PC_H: 1, "enh_pconv_h_kernel<16>": 1} if C == 64 else {PC_F: 1, "enh_pconv_kernel<16,16>": 1}
    assert log == {"enh_ln64_kernel" if C == 64 else "enh_ln_kernel": 1, **pc, **front, "enh_gate_kernel": 1, "enh_scale_transpose_kernel": 1}, log
    l = _lib()
    ws2, out2 = torch.empty_like(st.ws).fill_(0xFF), torch.full_like(out, NAN)
    l.check(l.lib().gencomm_enhancer_fwd(st.raw.data_ptr(), x.data_ptr(), out2.data_ptr(), n, C, H, W, ws2.data_ptr(), ws2.numel(),
                                         stream_ptr(torch.device(DEV))), "gencomm_enhancer_fwd")
    torch.cuda.synchronize()
    # the token-major result is the same launches' bit for bit; the pool sums meet in atomics of no fixed order, so the gate, and with it
    # the output, may differ in the last place
    assert torch.isfinite(out).all() and torch.isfinite(out2).all()
    o2 = ws2[st.off["O"]:st.off["O"] + 4 * n * H * W * C].view(torch.float32).view(n, H, W, C)
    assert torch.equal(st.view("O"), o2)
    assert float((out - out2).abs().max()) <= 1e-6 * float(out2.abs().max())


def test_a_stage_range_that_cuts_a_fused_launch_is_refused(modes):
    n, C, H, W = 1, 64, 8, 8
    st = Stages(R.random_sd(C, 3), n, C, H, W)
    l = _lib()
    for fuse, first, last, ok in ((2, 3, 4, False), (2, 4, 5, False), (2, 5, 5, False), (1, 4, 4, False), (1, 3, 3, False), (1, 5, 5, True), (0, 4, 4, True)):
        modes(arith="split", enh_fuse=fuse)
        st.ws.fill_(0)
        if ok:
            st.run(first, last)
        else:
            with pytest.raises(l.GenCommHipError, match="fused launch"):
                st.run(first, last)
    modes(arith="f32", enh_fuse=2)                       # the exact-fp32 arithmetic has no fused launch
    st.run(4, 4)
    with pytest.raises(l.GenCommHipError):
        st.run(0, 3)
    with pytest.raises(l.GenCommHipError):
        st.run(1, 1)                                      # stage 1 without x


# ---- range ------------------------------------------------------------------------------------------------------------------------------------
RANGE_STRUCTS = [(64, 0), (64, 1), (64, 2), (128, 0)]


def _range_log(C, fuse):
    return FRONT_LOG[fuse if C == 64 else 0]


@pytest.mark.parametrize("big", [20.0, 300.0])
@pytest.mark.parametrize("C,fuse", RANGE_STRUCTS)
def test_range_large_linear_weights_every_structure(modes, C, fuse, big):
    """A few entries of Linear1 / Linear2 set to +-big (test_gpu_enhancer_fuse.py's case for the fully fused structure, here for every
    structure). The f16-pipe kernels multiply a weight by a power of two before the fp16 split; with the static 2^12 a weight of magnitude
    >= 16 became inf as its first term and its residual NaN. gemm_f16s_mfma_kernel -- Linear1 and Linear2 for every C != 64, both under
    enh_fuse = 0, Linear2 under enh_fuse = 1 -- takes the tensor's scale from enh_wscale_kernel like the fused tables. The result must be
    finite and meet the criterion."""
    n, H, W = 2, 9, 13
    sd = R.random_sd(C, 101 + C)
    w1, w2 = sd[R.PM + "linear1.0.weight"], sd[R.PM + "linear2.0.weight"]
    w1[3, 5], w1[3 * C + 8, C - 4], w2[7, 11], w2[C - 24, 2 * C - 28] = big, -big, big, -big
    Z, Y = _randn(C, n, H, W, C), _randn(C + 1, n, H, W, C)
    G64, O64 = _front_truth(sd, Z, Y, torch.float64)
    G32, O32 = _front_truth(sd, Z, Y, torch.float32)
    modes(arith="split", enh_fuse=fuse)
    st = Stages(sd, n, C, H, W)
    st.put("Z", Z)
    st.put("Y", Y)
    log = st.run(3, 5)
    G, O = st.get("G"), st.get("O")
    print(f"range weights +-{big} C {C} enh_fuse {fuse}: G finite {bool(torch.isfinite(G).all()) if fuse < 2 or C != 64 else None}, O finite {bool(torch.isfinite(O).all())}; launched {log}")
    assert log == _range_log(C, fuse), log
    sub = R.subsets(n, H, W, 8, 8)
    if fuse < 2 or C != 64:
        _crit(f"range weights +-{big} C {C} enh_fuse {fuse} G", G, G64, G32, sub)
    _crit(f"range weights +-{big} C {C} enh_fuse {fuse} O", O, O64, O32, sub)


@pytest.mark.parametrize("C,fuse", [(64, 0), (64, 1), (128, 0)])
def test_range_gated_tensor_up_to_1e4_into_linear2(modes, C, fuse):
    """Linear2's A operand G = GELU(dw(x1)) x2 is a product of two hidden activations, bounded by no LayerNorm, and is split UNSCALED.
    Up to 1e4 (< 65504, the end of fp16) the three-term split is still exact: the criterion holds as for ordinary sizes."""
    n, H, W = 2, 9, 13
    sd = R.random_sd(C, 111 + C)
    G = (_randn(C, n, H, W, 2 * C) * 3e3).clamp(-1e4, 1e4)
    G[0, 0, 0, :4] = torch.tensor([1e4, -1e4, 9999.5, 1e-3])
    Y = _randn(C + 1, n, H, W, C)
    modes(arith="split", enh_fuse=fuse)
    st = Stages(sd, n, C, H, W)
    st.put("G", G)
    st.put("Y", Y)
    log = st.run(5, 5)
    assert log == {WSCALE: 1, F16_1: 1}, log
    O = st.get("O")
    _crit(f"range |G| <= 1e4 C {C} enh_fuse {fuse}", O, R.linear2(R.cast(sd, torch.float64), G.double(), Y.double()), R.linear2(R.cast(sd, torch.float32), G, Y),
          _gemm_subsets(n, H, W, C))
    _check_colsum(f"range |G| <= 1e4 C {C}", st.get("colsum"), O, H * W)


@pytest.mark.parametrize("C,fuse", RANGE_STRUCTS)
def test_range_gated_tensor_of_1e5_stays_finite(modes, C, fuse):
    """|G| >= 65520 is beyond fp16. Every f16-pipe kernel of the Enhancer runs with MODE.FP16_OVFL = 1 (fp16_ovfl_clamp), so the first
    term saturates to +-65504 instead of becoming inf (the second term still picks up part of the rest): the result is FINITE in every
    structure, but no longer accurate to fp32 -- saturation is accepted here, and only finiteness asserted, because a running activation
    scale for G belongs in the fused kernel's hot loop and is not part of this change. G is written by the test for the structures that
    keep it in memory; for all of them, parameters that make x1 ~ x2 ~ 400 (Linear1 bias 400, an identity depthwise tap) produce G ~ 1.6e5
    inside the launch."""
    n, H, W = 2, 9, 13
    sd = R.random_sd(C, 121 + C)
    modes(arith="split", enh_fuse=fuse)
    if fuse < 2 or C != 64:
        G = _randn(C, n, H, W, 2 * C) * 1e3
        G[:, ::2, ::3, ::5] = 1e5
        G[:, 1::2, ::3, 1::5] = -3e5
        st = Stages(sd, n, C, H, W)
        st.put("G", G)
        st.put("Y", _randn(C + 1, n, H, W, C))
        log = st.run(5, 5)
        assert log == {WSCALE: 1, F16_1: 1}, log
        assert torch.isfinite(st.get("O")).all() and torch.isfinite(st.get("colsum")).all()
    sd[R.PM + "linear1.0.bias"] = torch.full((4 * C,), 400.0)
    dw = torch.zeros(2 * C, 1, 3, 3)
    dw[:, 0, 1, 1] = 1.0
    sd[R.PM + "dwconv.0.weight"], sd[R.PM + "dwconv.0.bias"] = dw, torch.zeros(2 * C)
    Z, Y = _randn(C, n, H, W, C), _randn(C + 1, n, H, W, C)
    G64, _ = _front_truth(sd, Z, Y, torch.float64)
    assert float(G64.abs().min()) > 1e5
    st = Stages(sd, n, C, H, W)
    st.put("Z", Z)
    st.put("Y", Y)
    log = st.run(3, 5)
    assert log == _range_log(C, fuse), log
    assert torch.isfinite(st.get("O")).all() and torch.isfinite(st.get("colsum")).all()


GEMM_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enhancer_gemm_f16s_scale4096.npz")
GEMM_RECORD_KEYS = (R.PM + "linear1.0.weight", R.PM + "linear1.0.bias", R.PM + "linear2.0.weight", R.PM + "linear2.0.bias")


def gemm_record_inputs(C):
    """Inputs of the recorded runs (stored in the fixture beside the results, so that the test does not depend on a generator's stream)."""
    n, H, W = 2, 5, 7
    sd = R.random_sd(C, 131 + C)
    d = {k: sd[k].numpy() for k in GEMM_RECORD_KEYS}
    d.update(Z=_randn(C, n, H, W, C).numpy(), G=_randn(C + 1, n, H, W, 2 * C).numpy(), Y=_randn(C + 2, n, H, W, C).numpy())
    return d


def gemm_record_run(C, d):
    """gemm_f16s_mfma_kernel<0> and <1> on stored inputs -> (Hd, O) as numpy."""
    n, H, W = d["Z"].shape[:3]
    sd = R.random_sd(C, 1)
    sd.update({k: torch.from_numpy(d[k]) for k in GEMM_RECORD_KEYS})
    st = Stages(sd, n, C, H, W)
    st.put("Z", torch.from_numpy(d["Z"]))
    log = st.run(3, 3)
    assert log.get(F16_0) == 1, log
    Hd = st.get("Hd").numpy()
    st.put("G", torch.from_numpy(d["G"]))
    st.put("Y", torch.from_numpy(d["Y"]))
    log = st.run(5, 5)
    assert log.get(F16_1) == 1, log
    return Hd, st.get("O").numpy()


@pytest.mark.parametrize("C", [24, 40])
def test_f16_gemm_with_ordinary_weights_is_bit_identical_to_the_static_scale(modes, C):
    """max |w| < 4 keeps the scale of enh_wscale_kernel at 2^12, the former constant, so every scaled weight, product and result of
    gemm_f16s_mfma_kernel is what it was: both epilogues against results recorded from the library before the per-tensor scale (static
    2^12, the same stage entry), bit for bit. (The pool sums are accumulated by atomics in no fixed order and are not recorded.)"""
    z = np.load(GEMM_RECORD)
    d = {k[len(f"C{C}/"):]: z[k] for k in z.files if k.startswith(f"C{C}/")}
    assert max(float(np.abs(d[GEMM_RECORD_KEYS[0]]).max()), float(np.abs(d[GEMM_RECORD_KEYS[2]]).max())) < 4.0
    modes(arith="split", enh_fuse=0)
    Hd, O = gemm_record_run(C, d)
    assert np.array_equal(Hd, d["Hd"]) and np.array_equal(O, d["O"])
