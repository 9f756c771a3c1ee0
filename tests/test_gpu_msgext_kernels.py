"""The MessageExtractorv2 kernels called directly through the C ABI, each against the same operation in float64: the offset convolution
(conv3x3_cN_kernel, three tile instantiations), the fused deformable convolution (dcn_kernel, dcn_csplit_kernel), msg_gate_kernel and
msg_fuse_kernel behind gencomm_msgext_fwd, and the training path's sampling kernels (dcn_sample_kernel, dcn_scatter_bwd_kernel,
dcn_scatter_dx_tile_kernel, dcn_scatter_dx_gather_kernel) behind gencomm_dcn_sample_fwd / gencomm_dcn_scatter_bwd_ws /
gencomm_dcn_scatter_bwd.

Kernel criterion (as test_gpu_v2vnet.py::_check): three results per quantity -- truth (float64, CPU, oracle/torch_port.py), yardstick
(the same code in float32 on the CPU) and the kernel's; relative rms error of the kernel against the truth <= max(2 x the yardstick's,
1e-6). Outputs are pre-filled with NaN, so an element a kernel leaves out fails the test; the workspace is filled with NaN bit patterns
too, so a kernel that reads scratch nothing wrote shows as well.

Every forward case runs inside _lib.kernel_log() and asserts the exact launch log: the shapes are chosen by the selection arithmetic of
msgext_enqueue (quoted in each docstring), and a later change of a threshold that takes a kernel out of reach fails the case instead of
silently testing another kernel. The truth itself is pinned at the sampling edges by test_msgext_oracle.py (CPU)."""
import numpy as np
import pytest
import torch

import msgext_reference as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CONV64, CONV32x16, CONV32x8 = "conv3x3_cN_kernel<64,16,4,5>", "conv3x3_cN_kernel<32,16,4,5>", "conv3x3_cN_kernel<32,8,1,5>"


def _lib():
    from gencomm_amd import _lib as l
    return l


def _st():
    from gencomm_amd.runtime import stream_ptr
    return stream_ptr(torch.device(DEV))


def _log(conv, dcn):
    return {conv: 1, dcn: 1, "msg_gate_kernel": 1, "msg_fuse_kernel": 1}


def _workspace(n, C, H, W):
    l = _lib()
    return torch.empty(l.check_size(l.lib().gencomm_msgext_workspace_bytes(n, C, H, W), "gencomm_msgext_workspace_bytes"), dtype=torch.uint8, device=DEV)


def _run(sd, x, ws=None, poison=True):
    """gencomm_msgext_fwd on parameters packed as the module packs them -> (out [n, 2, H, W] numpy, kernel log)."""
    from gencomm_amd.runtime import PackedParams
    l = _lib()
    n, C, H, W = x.shape
    packed = PackedParams(l.msgext_param_table(C), l.check_size(l.lib().gencomm_msgext_raw_floats(C), "gencomm_msgext_raw_floats"))
    packed.update({k: v.to(DEV) for k, v in sd.items()})
    if ws is None:
        ws = _workspace(n, C, H, W)
    if poison:
        ws.fill_(0xFF)                                   # every float of the workspace a NaN
    xd = x.to(DEV).contiguous()
    out = torch.full((n, 2, H, W), NAN, device=DEV)
    with l.kernel_log() as kl:
        l.check(l.lib().gencomm_msgext_fwd(packed.flat.data_ptr(), xd.data_ptr(), out.data_ptr(), n, C, H, W, ws.data_ptr(), ws.numel(), _st()),
                "gencomm_msgext_fwd")
    torch.cuda.synchronize()
    return out.cpu().numpy(), dict(kl.counts)


def _tol(truth, yard):
    return max(2.0 * M.rel_rms(yard, truth), 1e-6)


def _check(what, got, truth, yard, log=None):
    e_k, e_y = M.rel_rms(got, truth), M.rel_rms(yard, truth)
    print(f"{what}: relative rms error against float64: kernel {e_k:.3e}, float32 ATen {e_y:.3e}, ratio {e_k / max(e_y, 1e-300):.2f}" + (f"; launched {log}" if log else ""))
    assert np.isfinite(np.asarray(got)).all(), f"{what}: output elements left unwritten"
    assert e_k <= max(2.0 * e_y, 1e-6), (what, e_k, e_y)


# ---- (a), (b): dcn_kernel and dcn_csplit_kernel on the same agents -----------------------------------------------------------------------
BIG = (4, 181, 182)     # n, H, W


@pytest.mark.parametrize("C", [8, 24])
def test_dcn_kernel_vs_float64(C):
    """msgext_enqueue takes dcn_kernel when cdiv(H W, 256) n >= 512: 181 x 182 = 32942 pixels = 129 workgroups per agent, x 4 agents = 516.
    The last workgroup of an agent has 32942 - 128 * 256 = 174 live lanes: two full waves, one partial (46 lanes) and one empty, all of
    which meet in the LDS reduction into colsum. C = 8 and 24: one and three 8-channel chunks. The offset convolution: default (split)
    arithmetic wants 160 workgroups; 64 x 16 tiles give 3 * 12 * 4 = 144, 32 x 16 tiles 6 * 12 * 4 = 288, so the 32 x 16 instantiation."""
    n, H, W = BIG
    sd, x, truth, yard = M.random_case(n, C, H, W, 50 + C)
    got, log = _run(sd, x)
    assert log == _log(CONV32x16, "dcn_kernel"), log
    _check(f"(a) dcn_kernel C {C} n {n} {H}x{W}", got, truth, yard, log)


@pytest.mark.parametrize("C", [8, 24])
def test_both_deformable_kernels_on_the_same_agents(C):
    """The first three agents of case (a) alone: 129 * 3 = 387 < 512 workgroups, so dcn_csplit_kernel (cdiv(32942, 64) = 515 workgroups
    per agent, the last with 46 live lanes); the offset convolution has 3 * 12 * 3 = 108 and 6 * 12 * 3 = 216 workgroups: 32 x 16 again.
    An agent's message depends on no other agent, so both runs answer to the same truth."""
    n, H, W = BIG
    sd, x, truth, yard = M.random_case(n, C, H, W, 50 + C)
    got4, log4 = _run(sd, x)
    got3, log3 = _run(sd, x[:3])
    assert log4 == _log(CONV32x16, "dcn_kernel"), log4
    assert log3 == _log(CONV32x16, "dcn_csplit_kernel"), log3
    _check(f"(b) dcn_kernel, agents 0-2 of n 4, C {C}", got4[:3], truth[:3], yard[:3], log4)
    _check(f"(b) dcn_csplit_kernel, the same agents alone, C {C}", got3, truth[:3], yard[:3], log3)
    e = M.rel_rms(got3, got4[:3])
    print(f"(b) C {C}: the two kernels differ by {e:.3e} relative rms")
    assert e <= 2.0 * _tol(truth[:3], yard[:3]), e


# ---- (c): dcn_csplit_kernel chunk splits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,H,W", [(1, 8, 7, 9), (2, 40, 9, 15), (3, 16, 8, 16)])
def test_dcn_csplit_chunk_splits_vs_float64(n, C, H, W):
    """dcn_csplit_kernel deals the C / 8 input chunks to its four waves (wave q: chunks q, q + 4, ...): C = 8 leaves three waves without a
    chunk (they still add zeros in LDS and finish their 16 output channels), C = 40 gives wave 0 two chunks and the others one, C = 16 two
    waves one each. 7 x 9 = 63 pixels: one workgroup, 63 live lanes; 9 x 15 = 135 = 2 * 64 + 7: seven live lanes in the last workgroup;
    8 x 16 = 128: no partial workgroup. cdiv(H W, 256) n <= 3 < 512: dcn_csplit_kernel; at most 3 workgroups of 64 x 16 or 32 x 16 tiles
    < 160: the 32 x 8 offset convolution."""
    sd, x, truth, yard = M.random_case(n, C, H, W, 60 + C)
    got, log = _run(sd, x)
    assert log == _log(CONV32x8, "dcn_csplit_kernel"), log
    _check(f"(c) dcn_csplit_kernel n {n} C {C} {H}x{W}", got, truth, yard, log)


# ---- (d): the offset convolution, every instantiation and both staging paths ---------------------------------------------------------
@pytest.mark.parametrize("W", [70, 72])
def test_offset_conv_every_tile_vs_float64(W, modes):
    """pick_tile: 64 x 16 tiles when cdiv(W, 64) cdiv(H, 16) n >= tile_want, else 32 x 16 when cdiv(W, 32) cdiv(H, 16) n >= tile_want, else
    32 x 8. n = 2, H = 20, W = 70 or 72: 2 * 2 * 2 = 8 and 3 * 2 * 2 = 12 workgroups, so tile_want = 1 -> 64 x 16, 10 -> 32 x 16,
    100 -> 32 x 8. W = 72 stages the input with 128-bit loads (W % 4 == 0), W = 70 with the scalar path; both have a partial tile in x
    (the gx + p < W store mask of the four-pixel lanes: 70 = 64 + 6 ends inside a lane's four pixels) and in y (20 = 16 + 4)."""
    n, C, H = 2, 16, 20
    sd, x, truth, yard = M.random_case(n, C, H, W, 70 + W)
    outs = {}
    for want, conv in ((1, CONV64), (10, CONV32x16), (100, CONV32x8)):
        modes(tile_want=want)
        got, log = _run(sd, x)
        assert log == _log(conv, "dcn_csplit_kernel"), (want, log)
        _check(f"(d) {conv} {H}x{W}", got, truth, yard, log)
        outs[conv] = got
    for a, b in ((CONV64, CONV32x16), (CONV64, CONV32x8), (CONV32x16, CONV32x8)):
        e = M.rel_rms(outs[a], outs[b])
        print(f"(d) {H}x{W}: {a} against {b}: {e:.3e} relative rms")
        assert e <= 2.0 * _tol(truth, yard), (a, b, e)


# ---- (e): sampling edges through the fused kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,W,plant,dcn,conv", [(2, 11, 13, 0.0, "dcn_csplit_kernel", CONV32x8), (4, 181, 182, 0.1, "dcn_kernel", CONV32x16)])
def test_sampling_edges_through_the_fused_kernels(n, H, W, plant, dcn, conv):
    """Exact offsets per pixel (msgext_reference.exact_offset_state_dict): offset1 copies input channel k < 18 into offset map k bit for
    bit, the deformable convolution reads channels 18 .. 23. The offsets put sampling positions exactly on -1, on H and W (open bounds),
    on integers (ly == 0), on H - 1 and W - 1 (no lower / right neighbour), on half and quarter pixels and far outside (+-1e6).
    2 x 24 x 11 x 13: one workgroup of 256 per agent < 512 -> dcn_csplit_kernel. 4 x 24 x 181 x 182: 516 workgroups -> dcn_kernel (case
    (a)); on a map that large the two offset sets alone reach the bounds only in the outermost rows, so a tenth of the pixels has every tap
    planted on an edge, and the test asserts that every 256-pixel workgroup holds such a position."""
    C = 24
    sd, x, truth, yard = M.exact_case(n, C, H, W, 0, plant)
    inside, bound, on_bound = M.edge_stats(x[:, :18])
    print(f"(e) {H}x{W}: {100 * inside:.1f} % of the (pixel, tap) positions inside the map, {100 * bound:.1f} % exactly on -1, H or W")
    assert 0.50 <= inside <= 0.85 and bound >= 0.02, (inside, bound)
    if plant > 0.0:
        per_pixel = on_bound.any(1).reshape(n, H * W)
        groups = -(-H * W // 256)
        padded = torch.zeros(n, groups * 256, dtype=torch.bool)
        padded[:, :H * W] = per_pixel
        assert bool(padded.view(n, groups, 256).any(2).all()), "a workgroup without a position on an open bound"
    got, log = _run(sd, x)
    assert log == _log(conv, dcn), log
    _check(f"(e) sampling edges through {dcn}, n {n} {H}x{W}", got, truth, yard, log)


# ---- (f): no stale state -------------------------------------------------------------------------------------------------------------------
def test_no_stale_state_in_a_reused_workspace():
    """One workspace tensor, a larger call (2 x 40 x 9 x 15) and then a smaller one (1 x 8 x 7 x 9) without touching it in between:
    colsum is accumulated by atomics and must be cleared by every call, and the zero-padded offset weights likewise; the second call's
    regions lie over whatever the first left there (its prepared weights and maps). Both shapes are those of case (c): one or two
    workgroups of 256 pixels < 512 -> dcn_csplit_kernel, at most 2 tiles < 160 -> the 32 x 8 offset convolution."""
    big, small = M.random_case(2, 40, 9, 15, 100), M.random_case(1, 8, 7, 9, 68)
    ws = _workspace(2, 40, 9, 15)
    got, log = _run(big[0], big[1], ws)
    assert log == _log(CONV32x8, "dcn_csplit_kernel"), log
    _check("(f) first call, 2 x 40 x 9 x 15", got, big[2], big[3], log)
    got, log = _run(small[0], small[1], ws, poison=False)
    assert log == _log(CONV32x8, "dcn_csplit_kernel"), log
    _check("(f) second call on the same workspace, 1 x 8 x 7 x 9", got, small[2], small[3], log)
    got, log = _run(big[0], big[1], ws, poison=False)
    _check("(f) third call, the larger shape again", got, big[2], big[3], log)


# ---- the training path's sampling kernels --------------------------------------------------------------------------------------------------
# maps that are no multiple of the 16 x 16 tile of dcn_scatter_dx_tile_kernel (20 x 36, 33 x 18), C = 12 and 20: a partial 8-channel chunk;
# non-square maps, so that the offsets +-H and +-W land INSIDE the map far beyond the 4-pixel LDS halo (the direct global-atomic branch)
TRAIN_SHAPES = [(2, 12, 20, 36), (1, 20, 33, 18)]


def _sample(x, off):
    n, C, H, W = x.shape
    xd, od = x.to(DEV).contiguous(), off.to(DEV).contiguous()
    col = torch.full((n, C * 9, H, W), NAN, device=DEV)
    _lib().check(_lib().lib().gencomm_dcn_sample_fwd(xd.data_ptr(), od.data_ptr(), col.data_ptr(), n, C, H, W, _st()), "gencomm_dcn_sample_fwd")
    torch.cuda.synchronize()
    return col.cpu()


def _scatter(x, off, dcol, scratch):
    """(dx, doffset) through gencomm_dcn_scatter_bwd_ws (scratch = True) or the null-scratch entry gencomm_dcn_scatter_bwd."""
    l = _lib()
    n, C, H, W = x.shape
    xd, od, dd = x.to(DEV).contiguous(), off.to(DEV).contiguous(), dcol.to(DEV).contiguous()
    dx = torch.zeros(n, C, H, W, device=DEV)                       # the ABI requires dx zeroed
    doff = torch.full((n, 18, H, W), NAN, device=DEV)
    if scratch:
        need = l.check_size(l.lib().gencomm_dcn_scatter_scratch_floats(n, C, H, W), "gencomm_dcn_scatter_scratch_floats")
        s = torch.full((need,), NAN, device=DEV)
        l.check(l.lib().gencomm_dcn_scatter_bwd_ws(xd.data_ptr(), od.data_ptr(), dd.data_ptr(), dx.data_ptr(), doff.data_ptr(), n, C, H, W,
                                                   s.data_ptr(), need, _st()), "gencomm_dcn_scatter_bwd_ws")
    else:
        l.check(l.lib().gencomm_dcn_scatter_bwd(xd.data_ptr(), od.data_ptr(), dd.data_ptr(), dx.data_ptr(), doff.data_ptr(), n, C, H, W, _st()),
                "gencomm_dcn_scatter_bwd")
    torch.cuda.synchronize()
    return dx.cpu(), doff.cpu()


@pytest.mark.parametrize("n,C,H,W", TRAIN_SHAPES)
def test_dcn_sample_edges_vs_float64(n, C, H, W):
    """gencomm_dcn_sample_fwd (dcn_sample_kernel) at the edge offsets against deform_conv2d_ref with an identity weight; positions exactly
    on an open bound give exact zeros."""
    case = M.sampling_case(n, C, H, W, H * W + C)
    inside, bound, on_bound = M.edge_stats(case["off"])
    assert 0.50 <= inside <= 0.85 and bound >= 0.02, (inside, bound)
    col = _sample(case["x"], case["off"])
    _check(f"dcn_sample n {n} C {C} {H}x{W}", col.numpy(), case["col64"].numpy(), case["col32"].numpy())
    assert float(col.view(n, C, 9, H, W)[on_bound.unsqueeze(1).expand(n, C, 9, H, W)].abs().max()) == 0.0


def test_dcn_sample_and_the_fused_kernels_make_the_same_cell_decisions():
    """Case (e)'s parameters on 2 x 24 x 11 x 13: the training path's sampler on the same input and offsets, then the rest of the module
    in float64 FROM THE KERNEL'S col (GEMM half, gate, 1x1 layers) must meet the criterion against the module's truth, and agree with
    the fused forward's output within twice it -- a sampler that decided one cell differently at an edge misses both."""
    n, C, H, W = 2, 24, 11, 13
    sd, x, truth, yard = M.exact_case(n, C, H, W, 0, 0.0)
    col = _sample(x, x[:, :18])
    via_col = M.module_from_col(sd, col).numpy()
    _check(f"module from the kernel's col, n {n} C {C} {H}x{W}", via_col, truth, yard)
    fused, log = _run(sd, x)
    assert log == _log(CONV32x8, "dcn_csplit_kernel"), log
    e = M.rel_rms(fused, via_col)
    print(f"fused forward against sampling + float64 GEMM: {e:.3e} relative rms")
    assert e <= 2.0 * _tol(truth, yard), e


@pytest.mark.parametrize("n,C,H,W", TRAIN_SHAPES)
def test_dcn_scatter_both_entries_vs_float64_autograd(n, C, H, W):
    """dx and doffset of both entries -- gencomm_dcn_scatter_bwd_ws with scratch (LDS regions stored, dcn_scatter_dx_gather_kernel sums
    them) and gencomm_dcn_scatter_bwd without (one global atomic per touched, non-zero cell of the region) -- against float64 autograd
    through deform_conv2d_ref.
    Integral positions are compared here although test_gpu_train_ops.py avoids them: at the edge offsets every sampling position is
    exactly representable in float32, so the kernel and the reference compute the SAME position, take the same floor, hence the same
    cell and the same one-sided derivative (floor is treated as constant by both); with Gaussian offsets a position within rounding of
    an integer could fall on either side in the two precisions and the derivatives would legitimately differ."""
    case = M.sampling_case(n, C, H, W, H * W + C)
    far = M.far_corner_count(case["off"])
    print(f"dcn_scatter n {n} C {C} {H}x{W}: {far} (pixel, tap) positions with corners beyond the 4-pixel halo of their tile")
    assert far > 0
    res = {}
    for scratch in (True, False):
        name = "gencomm_dcn_scatter_bwd_ws" if scratch else "gencomm_dcn_scatter_bwd (no scratch)"
        dx, doff = _scatter(case["x"], case["off"], case["dcol"], scratch)
        _check(f"{name} dx n {n} C {C} {H}x{W}", dx.numpy(), case["dx64"].numpy(), case["dx32"].numpy())
        _check(f"{name} doffset n {n} C {C} {H}x{W}", doff.numpy(), case["doff64"].numpy(), case["doff32"].numpy())
        res[scratch] = (dx, doff)
    e = float((res[True][0].double() - res[False][0].double()).pow(2).mean().sqrt() / case["dx64"].pow(2).mean().sqrt())
    print(f"the two entries' dx differ by {e:.3e} of the truth's rms")
    assert e <= 2.0 * _tol(case["dx64"].numpy(), case["dx32"].numpy()), e
    assert torch.equal(res[True][1], res[False][1])                # doffset: the same kernel, no atomics


@pytest.mark.parametrize("n,C,H,W", TRAIN_SHAPES)
def test_dcn_sample_and_scatter_are_adjoint(n, C, H, W):
    """<dcol, sample(x)> = <dx, x> (the sampling is linear in x and dx is its transpose applied to dcol), both sides in float64 from the
    kernels' float32 results, for both entries. The defect |lhs - rhs| is measured against ||dcol|| ||col|| (Cauchy-Schwarz: the natural
    scale of the bilinear form; |lhs| itself is a random sum and can be small) and judged by the project's criterion against the same
    defect of the float32 CPU results. The offsets include +-H, +-W on a non-square map: corners beyond the LDS halo, the direct
    global-atomic branch."""
    case = M.sampling_case(n, C, H, W, H * W + C)
    assert M.far_corner_count(case["off"]) > 0
    x64, d64 = case["x"].double(), case["dcol"].double()
    scale = float(d64.norm() * case["col64"].norm())
    t_l, t_r = float((d64 * case["col64"]).sum()), float((case["dx64"] * x64).sum())
    assert abs(t_l - t_r) <= 1e-12 * scale                          # the reference itself is adjoint
    e_y = abs(float((d64 * case["col32"].double()).sum()) - float((case["dx32"].double() * x64).sum())) / scale
    lhs = float((d64 * _sample(case["x"], case["off"]).double()).sum())
    for scratch in (True, False):
        dx, _ = _scatter(case["x"], case["off"], case["dcol"], scratch)
        assert torch.isfinite(dx).all()
        e_k = abs(lhs - float((dx.double() * x64).sum())) / scale
        print(f"adjoint identity n {n} C {C} {H}x{W} scratch {scratch}: <dcol, col> {lhs:.6f}; defect / (||dcol|| ||col||): kernel {e_k:.3e}, float32 ATen {e_y:.3e}")
        assert e_k <= max(2.0 * e_y, 1e-6), (scratch, e_k, e_y)
