"""V2VNet fusion on the GPU: the three message-passing kernels called directly through the C ABI, each against the same operation in
float64, then the module against the reference's stored outputs (tests/golden/v2vnet.npz) and against the restatement on a fresh shape,
determinism, record_len as a tensor, and the training refusal.

Kernel criterion (as test_gpu_v2xvit_kernels.py / test_gpu_lss_train.py): three results per quantity -- truth (float64, CPU), yardstick
(the same torch code in float32 on the CPU) and the kernel's; relative rms error of the kernel against the truth
<= max(2 x the yardstick's, 1e-6). Outputs are pre-filled with NaN, so an element a kernel leaves out fails the test."""
import math

import numpy as np
import pytest
import torch

import fusion_train_restatement as FR
import v2vnet_restatement as R
from test_v2vnet import load_v2vnet_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(6, 7, 9), (8, 12, 20)]      # H W = 63: no 128-bit path, a partly filled workgroup; H W = 240: the 128-bit path


def _lib():
    from gencomm_amd import _lib as l
    return l


def _call(name, *args):
    _lib().check(getattr(_lib().lib(), name)(*args), name)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _st():
    from gencomm_amd.runtime import stream_ptr
    return stream_ptr(torch.device(DEV))


def _ints(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _check(what, got, truth, yard):
    e_k, e_y = R.rel_rms(got, truth), R.rel_rms(yard, truth)
    print(f"{what}: relative rms error against float64: kernel {e_k:.3e}, float32 ATen {e_y:.3e}")
    assert np.isfinite(np.asarray(got)).all(), f"{what}: output elements left unwritten"
    assert e_k <= max(2.0 * e_y, 1e-6), (what, e_k, e_y)


def _thetas(H, W):
    """identity, a rotation, a half-pixel shift, a shift off the map."""
    return [FR.theta(H, W), FR.rot(H, W, 0.4, 1.37, -0.61), FR.theta(H, W, tx=0.5, ty=-0.5), FR.theta(H, W, tx=3.0 * W + 0.37)]


# ---- gencomm_v2v_warp_pairs_fwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_warp_pairs_vs_float64(C, H, W):
    rng = np.random.RandomState(H * W)
    x = torch.from_numpy(rng.standard_normal((3, C, H, W)).astype(np.float32))
    I, rot, half, off = _thetas(H, W)
    theta = torch.from_numpy(np.stack([I, rot, half, off, FR.rot(H, W, -0.9, 2.21, 1.43), I]))
    src = [0, 1, 2, 0, 1, 2]             # rows 0, 1 and 2 are each read for two targets
    out = torch.full((len(src), C, H, W), float("nan"), device=DEV)
    xd, td, sd = x.to(DEV), theta.to(DEV), _ints(src)
    _call("gencomm_v2v_warp_pairs_fwd", _p(xd), _p(td), _p(sd), _p(out), len(src), C, H, W, _st())
    got = out.cpu()
    truth, yard = R.warp(x[src].double(), theta), R.warp(x[src], theta)
    _check(f"warp_pairs C {C} {H}x{W}", got.numpy(), truth.numpy(), yard.numpy())
    assert torch.equal(got[0], x[0]) and torch.equal(got[5], x[2])          # identity pairs: bit-equal to their source
    assert float(got[3].abs().max()) == 0.0 and float(truth[3].abs().max()) == 0.0   # off the map: exact zeros
    assert float(np.abs(got.numpy() - truth.numpy()).max()) <= max(4.0 * float((yard.double() - truth).abs().max()), 1e-6 * float(truth.abs().max()))


# ---- gencomm_v2v_aggregate_fwd ------------------------------------------------------------------------------------------------------
def _aggregate_case(C, H, W):
    """Nodes of 1, 3 and 8 pairs; the first pair of a node is its own (identity); the 3-pair node's other agents are off the map."""
    rng = np.random.RandomState(C * H)
    I, _, half, off = _thetas(H, W)
    rigid = [FR.rot(H, W, rng.uniform(-math.pi, math.pi), *rng.uniform(-0.3 * W, 0.3 * W, 2)) for _ in range(7)]
    theta = np.stack([I] + [I, off, FR.theta(H, W, ty=-2.0 * H - 0.37)] + [I, half] + rigid[:6])
    pair_off, node_row = [0, 1, 4, 12], [4, 0, 2]
    y = torch.from_numpy(rng.standard_normal((12, C, H, W)).astype(np.float32))
    e = torch.from_numpy(rng.standard_normal((3, C, H, W)).astype(np.float32))
    h = torch.from_numpy(rng.standard_normal((5, C, H, W)).astype(np.float32))
    return y, e, h, torch.from_numpy(theta), node_row, pair_off


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_aggregate_vs_float64(C, H, W):
    y, e, h, theta, node_row, pair_off = _aggregate_case(C, H, W)
    dev = [t.to(DEV) for t in (y, e, h, theta)] + [_ints(node_row), _ints(pair_off)]     # kept alive for the launches
    for op in (0, 1):
        for out_mode in (0, 1):
            out = torch.full((3, C if out_mode else 2 * C, H, W), float("nan"), device=DEV)
            _call("gencomm_v2v_aggregate_fwd", *[_p(t) for t in dev], _p(out), 3, C, H, W, op, out_mode, _st())
            got = out.cpu().numpy()
            truth = R.aggregate(y.double(), e.double(), h.double(), theta, node_row, pair_off, op, out_mode).numpy()
            yard = R.aggregate(y, e, h, theta, node_row, pair_off, op, out_mode).numpy()
            _check(f"aggregate C {C} {H}x{W} op {op} out_mode {out_mode}", got, truth, yard)
            if out_mode == 0:
                assert np.array_equal(got[:, :C], h[node_row].numpy())                   # the h half of [h | agg] is a copy
            # the node whose other agents are off the map: only its own message is left, divided by 3 under the mean
            own = (y[1].double() + e[1].double()).numpy() * (1.0 / 3.0 if op == 0 else 1.0)
            agg = got[1, C:] if out_mode == 0 else got[1] - h[0].numpy()
            if op == 0:
                assert np.abs(agg - own).max() <= 1e-5 * np.abs(own).max()
            else:
                assert np.abs(agg - np.maximum(own, 0.0)).max() <= 1e-5 * np.abs(own).max()   # the masked agents contribute exact zeros


# ---- gencomm_gru_gate_fwd -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,HW", [(3, 5, 63), (2, 8, 240)])
def test_gru_gate_vs_float64(n, C, HW):
    rng = np.random.RandomState(HW)
    g = torch.from_numpy(rng.uniform(-30.0, 30.0, (n, 2 * C, HW)).astype(np.float32))
    g[0, 0, :4] = torch.tensor([-30.0, 30.0, 0.0, -0.0])
    g[0, C, :4] = torch.tensor([30.0, -30.0, 1e-4, 0.5])
    out = torch.full((n, C, HW), float("nan"), device=DEV)
    gd = g.to(DEV)
    _call("gencomm_gru_gate_fwd", _p(gd), _p(out), n, C, HW, _st())
    _check(f"gru_gate n {n} C {C} HW {HW}", out.cpu().numpy(), R.gate(g.double()).numpy(), R.gate(g).numpy())


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def _module(args, sd):
    from gencomm_amd import V2VNetFusion
    m = V2VNetFusion(args).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_module_vs_reference_golden(tag):
    """Against the reference's float64 output: relative rms <= max(2 x the reference float32 run's own, 1e-6) and max abs <= max(4 x the
    reference float32 run's own, 1e-5) (the factor 4: the split msg_cnn sums in a different order).
    Measured (HIP relative rms / max abs against float64; the reference's float32 run in brackets):
      a  5.105e-08 / 3.225e-08   (5.091e-08 / 3.304e-08)
      b  2.869e-08 / 2.089e-08   (2.838e-08 / 1.983e-08)
      c  8.922e-08 / 2.719e-07   (9.663e-08 / 2.502e-07)
      d  7.525e-08 / 3.855e-08   (7.109e-08 / 3.596e-08)     every convolution on the three-term matrix-pipe route
    """
    args, sd, x, rl, aff, out32, out64, ref_rms, ref_max = load_v2vnet_case(tag)
    m = _module(args, sd)
    with torch.no_grad():
        out = m(torch.from_numpy(x).to(DEV), rl, torch.from_numpy(aff).to(DEV)).cpu().numpy()
    e_rms, e_max = R.rel_rms(out, out64), float(np.abs(out - out64).max())
    print(f"v2vnet case {tag}: against the reference's float64 output: HIP rel rms {e_rms:.3e} max abs {e_max:.3e}; reference float32 rel rms "
          f"{ref_rms:.3e} max abs {ref_max:.3e}")
    assert out.shape == out64.shape and np.isfinite(out).all()
    assert e_rms <= max(2.0 * ref_rms, 1e-6), (tag, e_rms, ref_rms)
    assert e_max <= max(4.0 * ref_max, 1e-5), (tag, e_max, ref_max)


def test_two_runs_are_bit_identical_and_record_len_may_be_a_tensor():
    args, sd, x, rl, aff, *_ = load_v2vnet_case("b")
    m = _module(args, sd)
    xd, ad = torch.from_numpy(x).to(DEV), torch.from_numpy(aff).to(DEV)
    with torch.no_grad():
        junk = torch.full((8 << 20,), float("nan"), device=DEV)   # NaNs in the memory the allocator hands out next
        del junk
        a = m(xd, rl, ad).clone()
        b = m(xd, rl, ad).clone()
        c = m(xd, torch.tensor(rl), ad).clone()
        d = m(xd, torch.tensor(rl, device=DEV), ad).clone()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_single_scene_of_eight_agents_vs_restatement():
    """One scene, 8 agents (the most a node can receive from), C = 8, 8 x 12, max aggregation, two rounds, a [3, 3] and a [1, 1] GRU layer:
    against the float64 restatement, with the float32 restatement on the CPU as the yardstick."""
    c = dict(C=8, H=8, W=12, agg="max", gru=True, layers=2, iters=2)
    args = R.case_args(c)
    args["conv_gru"]["kernel_size"] = [[3, 3], [1, 1]]
    from gencomm_amd import V2VNetFusion, synth
    m = V2VNetFusion(args).eval()
    synth.fill_params_(m, 31)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.from_numpy(R.make_x(8, 8, 8, 12, 32))
    aff = torch.from_numpy(R.make_affine([8], 8, 8, 12, 33))
    with torch.no_grad():
        truth = R.v2vnet_forward(sd, args, x.double(), [8], aff).numpy()
        yard = R.v2vnet_forward(sd, args, x, [8], aff).numpy()
        out = m.to(DEV)(x.to(DEV), [8], aff.to(DEV)).cpu().numpy()
    assert out.shape == (1, 8, 8, 12)
    _check("v2vnet, one scene of 8 agents", out, truth, yard)


def test_training_is_refused_and_no_grad_runs():
    args, sd, x, rl, aff, *_ = load_v2vnet_case("c")
    m = _module(args, sd)
    xd, ad = torch.from_numpy(x).to(DEV), torch.from_numpy(aff).to(DEV)
    assert all(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match="v2vnet training"):
        m(xd, rl, ad)
    with torch.no_grad():
        out = m(xd, rl, ad)
    assert tuple(out.shape) == (4, 8, 12, 20) and not out.requires_grad and torch.isfinite(out).all()
