"""The V2X-ViT building-block kernels (gencomm_amd/csrc/v2xvit_kernels.h) called directly through the C ABI, each against the same
operation in float64 (tests/v2xvit_kernel_reference.py):

  window attention  gencomm_win_attn_fwd / _bwd: all seven (window, dim_head) pairs -- win_attn_mfma_kernel for (8,32) (8,64) (16,32)
                    (16,64), win_attn_kernel for (4,16) (4,32) (8,16); the form that ran is read from the kernel log -- on a map whose
                    window count fills every workgroup and on one whose last workgroup is partly filled, at unit and at large logits;
                    and against gencomm_swap_attn_fwd where CoBEVT's swap attention is the same function (one agent, window partition)
  agent attention   gencomm_hgt_attn_fwd at dim_head 8 .. 64 with scenes of 1 .. 8 agents in one launch, per-query-agent and streaming
                    form; gencomm_hgt_attn_bwd at dim_head 8, 16, 64
  warp              gencomm_warp_affine_fwd / _bwd: identity, whole-pixel shift, rotation, sampling positions within a pixel of each
                    border, maps sent far outside; the same thetas through gencomm_warp_maxfuse_fwd / gencomm_warp_attfuse_fwd with one
                    agent per scene, bit for bit the warp's output (one bilinear cell for every kernel, csrc/fuse_cell.h)
  split attention   gencomm_split3_attn_fwd at C 64 / 96 / 128 / 256, with and without the residual
  contract          argument errors, and the 8-agents-per-scene limit of the module

Three results per quantity: truth (float64, CPU), yardstick (the same torch code in float32 on the CPU) and the kernel's; the pass rule is
bn_reference.Report.check with C_OUT for outputs and C_GRAD for gradients.  Outputs are pre-filled with NaN and sit between guard
bands, so an element the kernel leaves out or a write past the end fails the test."""
import pytest
import torch

import v2xvit_kernel_reference as R
from bn_reference import C_GRAD, C_OUT, Report

pytestmark = pytest.mark.gpu

GUARD = 256          # floats on either side of every buffer a kernel writes
SENTINEL = 7.25


def _dev():
    return torch.device("cuda:0")


def _call(name, *args):
    from gencomm_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _st():
    from gencomm_amd.runtime import stream_ptr
    return stream_ptr(_dev())


def _p(t):
    from gencomm_amd.runtime import ptr
    return ptr(t)


class Guarded:
    """A float32 device buffer of exactly `shape` elements between two guard bands; intact(): the bands are as they were."""

    def __init__(self, shape, fill=float("nan")):
        numel = 1
        for v in shape:
            numel *= int(v)
        self.buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=_dev())
        self.t = self.buf[GUARD:GUARD + numel].view(*shape)
        self.t.fill_(fill)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


def _bound(ref, f32, c):
    """The max-error bound of Report.check for (ref, f32, c)."""
    ref, f32 = ref.detach().double(), f32.detach().double()
    return max(4.0 * float((f32 - ref).abs().max()), c * float(ref.abs().max()))


def _grads(fn, inputs, w, dtype):
    """fn on `inputs` in `dtype`: the output and the gradients of (out * w).sum() for every input."""
    xs = [t.to(dtype).clone().requires_grad_(True) for t in inputs]
    out = fn(*xs)
    return out.detach(), torch.autograd.grad((out * w.to(dtype)).sum(), xs)


# ---- window attention -------------------------------------------------------------------------------------------------------------
WIN_PAIRS = [(4, 16), (4, 32), (8, 16), (8, 32), (8, 64), (16, 32), (16, 64)]       # (window, dim_head): every pair the ABI dispatches
# per window: a map whose window count is a multiple of 256 / window^2 and one whose last workgroup is partly filled (H != W).  Window
# 16 has one window per workgroup: H != W with several windows
WIN_MAPS = {4: {"full": (16, 16), "partial": (20, 28)}, 8: {"full": (16, 32), "partial": (24, 40)}, 16: {"full": (32, 32), "partial": (32, 48)}}
WIN_N, WIN_HEADS = 2, 3
# q scale of the "hot" case: q . k / sqrt(dim_head) of N(0,1) entries is N(0,1), so the logits are N(0, 10^2) and their extremes over a
# map lie around 40-60; the gap between the two largest of T such logits is about 10 / sqrt(2 ln T), i.e. 3-5, against ln 99 = 4.6 for a
# 1 % runner-up: a large part of the rows keeps more than 1 % of its mass off the arg-max (asserted below)
HOT_Q = 10.0


def _win_kernel_name(ws, dh):
    return ("win_attn_mfma_kernel" if ws * ws >= 64 and dh % 32 == 0 else "win_attn_kernel") + f"<{dh},{ws}>"


def _win_case(ws, dh, which, scale):
    H, W = WIN_MAPS[ws][which]
    nwin, wpb = (H // ws) * (W // ws), 256 // (ws * ws)
    assert (nwin % wpb == 0) == (which == "full") or wpb == 1, (nwin, wpb)
    if which == "partial":
        assert H != W and nwin > 1
    g = torch.Generator().manual_seed(1000 * ws + dh + (7 if which == "partial" else 0) + (13 if scale == "hot" else 0))
    inner = WIN_HEADS * dh
    qkv = torch.randn(WIN_N, 3 * inner, H, W, generator=g)
    if scale == "hot":
        qkv[:, :inner] *= HOT_Q
    pos = torch.randn(2 * ws - 1, 2 * ws - 1, generator=g)
    off_centre = torch.ones_like(pos, dtype=torch.bool)
    off_centre[ws - 1, ws - 1] = False
    off_diag = ~torch.eye(2 * ws - 1, dtype=torch.bool)
    assert bool((pos != pos.t())[off_diag].all()) and bool((pos != pos.flip(0, 1))[off_centre].all())   # pos[dy][dx], [dx][dy], [-dy][-dx] all differ
    dout = torch.randn(WIN_N, inner, H, W, generator=g)
    logits = R.window_logits(qkv.double(), pos.double(), WIN_HEADS, dh, ws)
    off_max = 1.0 - logits.softmax(-1).amax(-1)
    share = float((off_max >= 0.01).double().mean())
    peak = float(logits.abs().max())
    if scale == "hot":
        assert peak >= 30.0, peak
        assert share >= 0.2, share         # not a degenerate one-hot softmax
    title = f"{_win_kernel_name(ws, dh)} {H}x{W} ({nwin} windows, {wpb} per workgroup) {scale} (max |logit| {peak:.0f}, {100 * share:.0f}% soft rows)"
    return H, W, qkv, pos, dout, title


def _win_fwd(qkv_d, pos_d, ws, dh, H, W):
    out = Guarded((WIN_N, WIN_HEADS * dh, H, W))
    _call("gencomm_win_attn_fwd", _p(qkv_d), _p(pos_d), _p(out.t), WIN_N, WIN_HEADS, dh, ws, H, W, _st())
    assert out.intact()
    return out.t


@pytest.mark.parametrize("scale", ["unit", "hot"])
@pytest.mark.parametrize("which", ["full", "partial"])
@pytest.mark.parametrize("ws,dh", WIN_PAIRS)
def test_win_attn_fwd(ws, dh, which, scale):
    from gencomm_amd import _lib
    H, W, qkv, pos, _, title = _win_case(ws, dh, which, scale)
    with _lib.kernel_log() as kl:
        out = _win_fwd(qkv.to(_dev()), pos.to(_dev()), ws, dh, H, W)
    assert kl.counts == {_win_kernel_name(ws, dh): 1}, kl.counts
    rep = Report("fwd " + title)
    try:
        rep.check("out", out, R.win_attn(qkv.double(), pos.double(), WIN_HEADS, dh, ws), R.win_attn(qkv, pos, WIN_HEADS, dh, ws), C_OUT)
    finally:
        rep.show()


@pytest.mark.parametrize("scale", ["unit", "hot"])
@pytest.mark.parametrize("which", ["full", "partial"])
@pytest.mark.parametrize("ws,dh", WIN_PAIRS)
def test_win_attn_bwd(ws, dh, which, scale):
    """gencomm_win_attn_bwd on the forward kernel's own `out`: dqkv overwritten (NaN beforehand), dpos accumulated onto a non-zero
    table (twice: the atomic sum has no fixed order, so the two runs need only agree within the bound), scratch of exactly
    gencomm_win_attn_bwd_scratch_floats floats, NaN beforehand."""
    from gencomm_amd import _lib
    H, W, qkv, pos, dout, title = _win_case(ws, dh, which, scale)
    inner = WIN_HEADS * dh
    fn = lambda a, b: R.win_attn(a, b, WIN_HEADS, dh, ws)
    _, (dqkv64, dpos64) = _grads(fn, (qkv, pos), dout, torch.float64)
    _, (dqkv32, dpos32) = _grads(fn, (qkv, pos), dout, torch.float32)
    qkv_d, pos_d, dout_d = qkv.to(_dev()), pos.to(_dev()), dout.to(_dev())
    out_d = _win_fwd(qkv_d, pos_d, ws, dh, H, W)
    nfl = _lib.check_size(_lib.lib().gencomm_win_attn_bwd_scratch_floats(WIN_N, WIN_HEADS, ws, H, W), "gencomm_win_attn_bwd_scratch_floats")
    prefill = (torch.arange((2 * ws - 1) ** 2, dtype=torch.float32).reshape(2 * ws - 1, 2 * ws - 1) % 7 - 3.0) * 0.25 + 0.125   # never zero
    rep = Report("bwd " + title.replace("win_attn_mfma_kernel", "win_attn_bwd_{a,b}_kernel").replace("win_attn_kernel", "win_attn_bwd_{a,b}_kernel"))
    runs = []
    try:
        for run in (1, 2):
            dqkv, scratch, dpos = Guarded(qkv.shape), Guarded((nfl,)), Guarded(prefill.shape, 0.0)
            dpos.t.copy_(prefill)
            _call("gencomm_win_attn_bwd", _p(qkv_d), _p(pos_d), _p(out_d), _p(dout_d), _p(dqkv.t), _p(dpos.t), _p(scratch.t),
                  WIN_N, WIN_HEADS, dh, ws, H, W, _st())
            assert dqkv.intact() and scratch.intact() and dpos.intact()
            got = dqkv.t.cpu()
            for i, name in enumerate(("dq", "dk", "dv")):
                sl = slice(i * inner, (i + 1) * inner)
                rep.check(f"{name} (run {run})", got[:, sl], dqkv64[:, sl], dqkv32[:, sl], C_GRAD)
            runs.append(dpos.t.cpu().double() - prefill.double())
            rep.check(f"dpos after - prefill (run {run})", runs[-1], dpos64, dpos32, C_GRAD)
        diff, bound = float((runs[0] - runs[1]).abs().max()), _bound(dpos64, dpos32, C_GRAD)
        print(f"{rep.title} dpos run 1 vs run 2: max difference {diff:.2e} (bound {bound:.2e})")
        assert diff <= bound
    finally:
        rep.show()


@pytest.mark.parametrize("ws,dh", [(8, 32), (8, 64), (4, 32)])
def test_swap_and_window_attention_agree_where_they_overlap(ws, dh):
    """CoBEVT's swap attention with one agent per scene and the window partition is plain window attention, so gencomm_swap_attn_fwd
    and gencomm_win_attn_fwd must agree there: (8, 32) and (8, 64) run the matrix-core tile (csrc/attn_mfma.h) on both sides, (4, 32)
    the lane-per-query kernel on the window side.  The swap table is indexed by query - key and pos by key - query, so table[i][head] =
    pos.flatten()[(2 ws - 1)^2 - 1 - i].  Map 16 x 24 (X != Y), two heads, two scenes, qkv as in test_swap_attention_kernel_vs_float64.
    The two sides differ in their exponential (expf against __expf), so they are not compared bit for bit.  The tolerance is DERIVED, not
    measured: each side is already held to a bound against float64 -- the swap side to assert_close(rtol 1e-4, atol 1e-5)
    (test_swap_attention_kernel_vs_float64), the window side to Report.check's max-error bound with C_OUT (test_win_attn_fwd) -- and
    two results within those bounds of the truth differ by at most their sum."""
    import numpy as np
    from gencomm_amd import _lib
    heads, B, H, W = 2, 2, 16, 24
    rng = np.random.RandomState(100 * ws + dh)
    qkv = rng.standard_normal((B, 3 * heads * dh, H, W)).astype(np.float32)
    qkv[:, :heads * dh] *= 1.5
    qkv = torch.from_numpy(qkv)
    pos = torch.from_numpy(rng.uniform(-1.0, 1.0, (2 * ws - 1, 2 * ws - 1)).astype(np.float32))
    off_centre = torch.ones_like(pos, dtype=torch.bool)
    off_centre[ws - 1, ws - 1] = False
    assert bool((pos != pos.flip(0, 1))[off_centre].all())   # pos[dy][dx] != pos[-dy][-dx]: a table that is not flipped shows
    table = pos.flatten().flip(0)[:, None].repeat(1, heads).contiguous()
    q_d, nv = qkv.to(_dev()), torch.ones(B, dtype=torch.int32, device=_dev())
    swap, win = Guarded((B, heads * dh, H, W)), Guarded((B, heads * dh, H, W))
    with _lib.kernel_log() as kl:
        _call("gencomm_swap_attn_fwd", _p(q_d), _p(table.to(_dev())), _p(nv), _p(swap.t), B, 1, heads, dh, ws, H, W, 0, _st())
        _call("gencomm_win_attn_fwd", _p(q_d), _p(pos.to(_dev())), _p(win.t), B, heads, dh, ws, H, W, _st())
    assert swap.intact() and win.intact()
    assert kl.counts == {f"swap_attn_kernel<{dh},{ws}>": 1, _win_kernel_name(ws, dh): 1}, kl.counts
    truth, f32 = R.win_attn(qkv.double(), pos.double(), heads, dh, ws), R.win_attn(qkv, pos, heads, dh, ws)
    tol = _bound(truth, f32, C_OUT) + 1e-5 + 1e-4 * truth.abs()
    err = (swap.t.cpu().double() - win.t.cpu().double()).abs()
    print(f"swap vs window attention ws {ws} dh {dh}: max difference {float(err.max()):.2e}, smallest tolerance {float(tol.min()):.2e}")
    assert bool(torch.isfinite(err).all()) and bool((err <= tol).all()), (float(err.max()), float(tol.min()))


# ---- agent attention --------------------------------------------------------------------------------------------------------------
HGT_LENS = [8, 1, 7, 2, 6, 3, 5, 4]      # every scene size the kernels instantiate, in one launch
HGT_HEADS = 2
HGT_STREAM_THREADS = 131072              # gencomm_hgt_attn_fwd: HW heads B from which dim_head 16 / 32 take the streaming form


def _hgt_case(dh, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    n, inner = sum(HGT_LENS), HGT_HEADS * dh
    assert (H * W) % 256 != 0
    qkv = torch.randn(n, 3 * inner, H * W, generator=g)
    dout = torch.randn(n, inner, H * W, generator=g)
    off = [0]
    for v in HGT_LENS:
        off.append(off[-1] + v)
    return qkv, dout, torch.tensor(off, dtype=torch.int32, device=_dev())


@pytest.mark.parametrize("dh,H,W", [(8, 13, 23), (16, 13, 23), (32, 13, 23), (64, 13, 23), (8, 9, 15), (16, 90, 93), (32, 90, 93)])
def test_hgt_attn_fwd(dh, H, W):
    from gencomm_amd import _lib
    qkv, _, so = _hgt_case(dh, H, W, 50 + dh + H)
    HW, B = H * W, len(HGT_LENS)
    stream = HW * HGT_HEADS * B >= HGT_STREAM_THREADS and dh in (16, 32)
    assert stream == (H == 90)
    kernel = "hgt_attn_stream_kernel" if stream else "hgt_attn_kernel"
    out, qkv_d = Guarded((sum(HGT_LENS), HGT_HEADS * dh, HW)), qkv.to(_dev())
    with _lib.kernel_log() as kl:
        _call("gencomm_hgt_attn_fwd", _p(qkv_d), _p(so), _p(out.t), B, HGT_HEADS, dh, HW, _st())
        assert out.intact()
    assert kl.counts == {kernel: 1}, kl.counts
    rep = Report(f"fwd {kernel}<{dh}> HW {HW} scenes {HGT_LENS}")
    try:
        ref64, ref32 = R.hgt_attn(qkv.double(), HGT_LENS, HGT_HEADS, dh), R.hgt_attn(qkv, HGT_LENS, HGT_HEADS, dh)
        off = 0
        for N in HGT_LENS:      # per scene size: the streaming form has one instantiation per size
            rep.check(f"out, scene of {N}", out.t[off:off + N], ref64[off:off + N], ref32[off:off + N], C_OUT)
            off += N
    finally:
        rep.show()


@pytest.mark.parametrize("dh", [8, 16, 64])
def test_hgt_attn_bwd(dh):
    H, W = 13, 23
    qkv, dout, so = _hgt_case(dh, H, W, 90 + dh)
    HW, inner = H * W, HGT_HEADS * dh
    fn = lambda a: R.hgt_attn(a, HGT_LENS, HGT_HEADS, dh)
    _, (d64,) = _grads(fn, (qkv,), dout, torch.float64)
    _, (d32,) = _grads(fn, (qkv,), dout, torch.float32)
    dqkv, qkv_d, dout_d = Guarded(qkv.shape), qkv.to(_dev()), dout.to(_dev())
    _call("gencomm_hgt_attn_bwd", _p(qkv_d), _p(so), _p(dout_d), _p(dqkv.t), len(HGT_LENS), HGT_HEADS, dh, HW, _st())
    assert dqkv.intact()
    rep = Report(f"bwd hgt_attn_bwd_kernel<{dh}> HW {HW} scenes {HGT_LENS}")
    try:
        got, off = dqkv.t.cpu(), 0
        for N in HGT_LENS:
            for i, name in enumerate(("dq", "dk", "dv")):
                sl = slice(i * inner, (i + 1) * inner)
                rep.check(f"{name}, scene of {N}", got[off:off + N, sl], d64[off:off + N, sl], d32[off:off + N, sl], C_GRAD)
            off += N
    finally:
        rep.show()


# ---- warp -------------------------------------------------------------------------------------------------------------------------
def _thetas(H, W):
    """name -> theta [2][3] (normalised: a shift of d pixels is 2 d / W resp. 2 d / H)"""
    import math
    a = math.radians(7.0)
    c, s = math.cos(a), math.sin(a)
    px, py = 2.0 / W, 2.0 / H
    return {
        "identity": [[1, 0, 0], [0, 1, 0]],
        "shift x+1 y-1": [[1, 0, px], [0, 1, -py]],
        "rotation 7 deg + shift": [[c, -s * H / W, 2.3 * px], [s * W / H, c, -1.6 * py]],          # as normalize_pairwise_tfm builds it
        "shift +0.4 +0.7 (right / bottom band)": [[1, 0, 0.4 * px], [0, 1, 0.7 * py]],
        "shift -0.6 -0.3 (left / top band)": [[1, 0, -0.6 * px], [0, 1, -0.3 * py]],
        "zoom out (all four bands)": [[(W + 1.5) / W, 0, 0], [0, (H + 1.5) / H, 0]],
        "far 1e3": [[1, 0, 1e3], [0, 1, -1e3]],
        "far 1e9": [[1, 0, -1e9], [0, 1, 1e9]],
    }


def _border_bands(theta, H, W):
    """How many output pixels sample with exactly the left / right / top / bottom corner pair outside (float64 positions)."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xb, yb = (2 * xs + 1) / W - 1, (2 * ys + 1) / H - 1
    ix = ((theta[0, 0] * xb + theta[0, 1] * yb + theta[0, 2] + 1) * W - 1) / 2
    iy = ((theta[1, 0] * xb + theta[1, 1] * yb + theta[1, 2] + 1) * H - 1) / 2
    x0, y0 = ix.floor(), iy.floor()
    return [int(m.sum()) for m in (x0 == -1, x0 == W - 1, y0 == -1, y0 == H - 1)]


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("H,W", [(8, 16), (13, 22)])
def test_warp_affine_fwd_bwd(H, W, C):
    """On the 8 x 16 map every grid value of the identity and of the whole-pixel shift is a dyadic rational that float32 holds exactly
    ((2 w + 1) / 16 - 1 and 2 / 16), so the sampling positions are whole numbers and the output must be the input / its slice bit for
    bit.  At 13 x 22 the float32 grid is rounded (in torch's warp_affine_simple too), and those rows go through the float64 bound
    like the others."""
    names = list(_thetas(H, W))
    theta = torch.tensor([_thetas(H, W)[k] for k in names], dtype=torch.float64)
    n = len(names)
    assert H != W and (H * W) % 256 != 0
    g = torch.Generator().manual_seed(H * W + C)
    x, dout = torch.randn(n, C, H, W, generator=g), torch.randn(n, C, H, W, generator=g)
    seen = [0, 0, 0, 0]
    for i, k in enumerate(names):
        if "band" in k:
            seen = [a + b for a, b in zip(seen, _border_bands(theta[i], H, W))]
    assert min(seen) > 0, seen          # each single out-of-range side is sampled
    out64, (dx64,) = _grads(lambda t: R.warp_affine(t, theta), (x,), dout, torch.float64)
    out32, (dx32,) = _grads(lambda t: R.warp_affine(t, theta), (x,), dout, torch.float32)
    th_d, x_d, dout_d = theta.to(_dev()), x.to(_dev()), dout.to(_dev())
    out, dx = Guarded(x.shape), Guarded(x.shape)
    _call("gencomm_warp_affine_fwd", _p(x_d), _p(th_d), _p(out.t), n, C, H, W, _st())
    _call("gencomm_warp_affine_bwd", _p(th_d), _p(dout_d), _p(dx.t), n, C, H, W, _st())
    assert out.intact() and dx.intact()
    o, d = out.t.cpu(), dx.t.cpu()
    rep = Report(f"warp_affine_kernel / warp_affine_bwd_kernel {H}x{W} C {C}")
    try:
        for i, k in enumerate(names):
            rep.check(f"out [{k}]", o[i], out64[i], out32[i], C_OUT)
            rep.check(f"dx [{k}]", d[i], dx64[i], dx32[i], C_GRAD)
        for i, k in enumerate(names):
            if k.startswith("far"):
                assert float(out64[i].abs().max()) == 0.0 and float(dx64[i].abs().max()) == 0.0
                assert bool((o[i] == 0).all()) and bool((d[i] == 0).all()), k
        if (H, W) == (8, 16):
            assert torch.equal(o[0], x[0]), "identity is not bit-exact"
            shifted = torch.zeros_like(x[1])
            shifted[:, 1:, :-1] = x[1][:, :-1, 1:]         # out[h][w] = x[h - 1][w + 1]
            assert torch.equal(o[1], shifted), "whole-pixel shift is not bit-exact"
    finally:
        rep.show()


@pytest.mark.parametrize("H,W,C", [(13, 22, 5), (16, 16, 3)])
def test_warp_is_one_cell_across_kernels(H, W, C):
    """warp_affine_kernel, warp_attfuse_kernel in max mode and in attention mode sample with one bilinear cell (csrc/fuse_cell.h): with
    every agent a scene of its own the three outputs are the same bits -- the max of one map is that map, and the attention weight of a
    single agent is exp(0) / exp(0) = 1 with fmaf(1, v, 0) = v.  x has no zeros, so a tap dropped or added by one kernel shows."""
    names = list(_thetas(H, W))
    theta = torch.tensor([_thetas(H, W)[k] for k in names], dtype=torch.float64)
    n = len(names)
    assert sum(k.startswith("far") for k in names) == 2
    seen = [0, 0, 0, 0]
    for i, k in enumerate(names):
        if "band" in k:
            seen = [a + b for a, b in zip(seen, _border_bands(theta[i], H, W))]
    assert min(seen) > 0, seen          # each single out-of-range side is sampled
    g = torch.Generator().manual_seed(3 * H * W + C)
    x = torch.randn(n, C, H, W, generator=g)
    x = torch.where(x == 0, torch.ones_like(x), x)
    th_d, x_d = theta.to(_dev()), x.to(_dev())
    scene_off = torch.arange(n + 1, dtype=torch.int32, device=_dev())
    warp, mx, att = Guarded(x.shape), Guarded(x.shape), Guarded(x.shape)
    _call("gencomm_warp_affine_fwd", _p(x_d), _p(th_d), _p(warp.t), n, C, H, W, _st())
    _call("gencomm_warp_maxfuse_fwd", _p(x_d), _p(th_d), _p(scene_off), _p(mx.t), n, n, C, H, W, _st())
    _call("gencomm_warp_attfuse_fwd", _p(x_d), _p(th_d), _p(scene_off), _p(att.t), n, n, C, H, W, _st())
    assert warp.intact() and mx.intact() and att.intact()
    o = warp.t.cpu()
    assert bool(torch.isfinite(o).all()) and float(o[0].abs().max()) > 0
    for i, k in enumerate(names):
        assert torch.equal(mx.t[i].cpu(), o[i]), f"max fusion differs from warp_affine [{k}]"
        assert torch.equal(att.t[i].cpu(), o[i]), f"attention fusion differs from warp_affine [{k}]"


# ---- split attention --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("C", [64, 96, 128, 256])
def test_split3_attn_fwd(C, n):
    g = torch.Generator().manual_seed(3 * C + n)
    rnd = lambda *s: torch.randn(*s, generator=g)
    fc1, fc2 = rnd(C, C) / C ** 0.5, rnd(3 * C, C) * 2.0 / C ** 0.5
    ln_w, ln_b = 1.0 + 0.3 * rnd(C), 0.3 * rnd(C)
    rep = Report(f"split3_gap / _gate / _apply_kernel C {C} n {n}")
    try:
        for HW in (9 * 15, 13 * 23):                # below 256, and above it without being a multiple
            assert HW % 256 != 0
            a, b, c = (rnd(n, C, HW) + 2.0 * rnd(n, C, 1) for _ in range(3))       # per-channel means: the gates are not all 1/3
            res = rnd(n, C, HW)
            t64 = [t.double() for t in (a, b, c, fc1, ln_w, ln_b, fc2)]
            gates = R.split3_gates(*t64)
            assert float((gates.amax(1) - gates.amin(1)).max()) > 0.1       # a wrong branch order shows
            dev = [t.to(_dev()) for t in (a, b, c, fc1, ln_w, ln_b, fc2)]
            for r in (res, None):
                out, scratch, r_d = Guarded((n, C, HW)), Guarded((4 * n * C,)), None if r is None else r.to(_dev())
                _call("gencomm_split3_attn_fwd", *[_p(t) for t in dev], _p(r_d), _p(out.t), _p(scratch.t), n, C, HW, _st())
                assert out.intact() and scratch.intact()
                rep.check(f"out HW {HW} {'with' if r is not None else 'NULL'} residual", out.t,
                          R.split3(*t64, None if r is None else r.double()), R.split3(a, b, c, fc1, ln_w, ln_b, fc2, r), C_OUT)
                rep.check(f"gates HW {HW}", scratch.t[n * C:].view(n, 3, C), gates, R.split3_gates(a, b, c, fc1, ln_w, ln_b, fc2), C_OUT)
    finally:
        rep.show()


# ---- contract ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_do_not_launch():
    """Unsupported shapes return an error code and leave the output alone."""
    from gencomm_amd import _lib
    l = _lib.lib()
    buf = torch.zeros(1 << 16, device=_dev())
    so = torch.tensor([0, 1], dtype=torch.int32, device=_dev())

    def refused(rc, text):
        assert rc != 0
        msg = l.gencomm_last_error().decode()
        assert text in msg, msg

    pairs = "(4,16) (4,32) (8,16) (8,32) (8,64) (16,32) (16,64)"
    for ws, dh in ((4, 64), (16, 16), (2, 16), (8, 24)):
        out = Guarded((1, dh, 16, 16))
        refused(l.gencomm_win_attn_fwd(_p(buf), _p(buf), _p(out.t), 1, 1, dh, ws, 16, 16, _st()), pairs)
        refused(l.gencomm_win_attn_bwd(_p(buf), _p(buf), _p(buf), _p(buf), _p(out.t), _p(buf), _p(buf), 1, 1, dh, ws, 16, 16, _st()), pairs)
        assert out.intact() and bool(out.t.isnan().all())
    out = Guarded((1, 32, 12, 16))
    refused(l.gencomm_win_attn_fwd(_p(buf), _p(buf), _p(out.t), 1, 1, 32, 8, 12, 16, _st()), "multiples of the window size")
    refused(l.gencomm_win_attn_bwd(_p(buf), _p(buf), _p(buf), _p(buf), _p(out.t), _p(buf), _p(buf), 1, 1, 32, 8, 16, 12, _st()),
            "multiples of the window size")
    assert l.gencomm_win_attn_bwd_scratch_floats(1, 1, 8, 12, 16) == -1
    assert out.intact() and bool(out.t.isnan().all())
    out = Guarded((1, 257, 4))
    refused(l.gencomm_split3_attn_fwd(*[_p(buf)] * 7, None, _p(out.t), _p(buf), 1, 257, 4, _st()), "C <= 256")
    assert out.intact() and bool(out.t.isnan().all())
    out = Guarded((1, 3 * 24, 4))
    refused(l.gencomm_hgt_attn_fwd(_p(buf), _p(so), _p(out.t), 1, 1, 24, 4, _st()), "dim_head must be 8, 16, 32 or 64")
    refused(l.gencomm_hgt_attn_bwd(_p(buf), _p(so), _p(buf), _p(out.t), 1, 1, 24, 4, _st()), "dim_head must be 8, 16, 32 or 64")
    assert out.intact() and bool(out.t.isnan().all())


def test_v2xvit_refuses_nine_agents():
    """The attention kernels leave a scene of more than 8 agents untouched without an error (include/gencomm_hip.h): the module must refuse
    it before any launch."""
    import json

    from helpers import load_case
    from gencomm_amd.fusion import MAX_AGENTS_PER_SCENE
    from gencomm_amd.v2xvit import V2XViTFusion
    assert MAX_AGENTS_PER_SCENE == 8
    net = V2XViTFusion(json.loads(str(load_case("v2xvit")["args"]))).eval().cuda()
    aff = torch.eye(2, 3, dtype=torch.float64).expand(1, 9, 9, 2, 3).contiguous()
    with torch.no_grad():
        with pytest.raises(ValueError, match="agents per scene"):
            net(torch.zeros(9, 128, 16, 16, device=_dev()), [9], aff)
        with pytest.raises(ValueError, match="agents per scene"):
            net(torch.zeros(10, 128, 16, 16, device=_dev()), [1, 9], aff.expand(2, 9, 9, 2, 3).contiguous())
        out = net(torch.zeros(8, 128, 16, 16, device=_dev()), [8], aff[:, :8, :8].contiguous())
    assert list(out.shape) == [1, 128, 16, 16]
