"""CoBEVT on the GPU: the swap-attention kernel alone against a float64 restatement, the module against the reference's stored
outputs (tests/golden/cobevt.npz) and against the restatement on fresh shapes, determinism, and the stage-1 shell."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import cobevt_restatement as R
from helpers import GOLDEN, assert_close, load_case, shell_noise
from gencomm_amd import CoBEVT, _lib, synth
from gencomm_amd.cobevt import Attention
from gencomm_amd.runtime import ptr, stream_ptr
from test_cobevt import load_cobevt_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_rms(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).mean()) / max(np.sqrt((ref ** 2).mean()), 1e-300))


def poison_allocator():
    """Leave NaNs in the memory torch's caching allocator hands out next: a kernel that reads a workspace it did not write shows."""
    junk = torch.full((32 << 20,), float("nan"), device=DEV)
    del junk


def swap_attn_hip(qkv, table, nvalid, L, heads, dh, ws, grid):
    """gencomm_swap_attn_fwd on qkv [B L, 3 heads dh, H, W]; the output starts as NaN, so an element the kernel leaves out shows."""
    n, _, H, W = qkv.shape
    B = n // L
    out = torch.full((n, heads * dh, H, W), float("nan"), device=DEV)
    nv = torch.tensor(nvalid, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().gencomm_swap_attn_fwd(ptr(qkv), ptr(table), ptr(nv), ptr(out), B, L, heads, dh, ws, H, W, int(grid), stream_ptr(qkv.device)),
               "gencomm_swap_attn_fwd")
    return out


@pytest.mark.parametrize("ws,dh", [(4, 16), (4, 32), (4, 64), (8, 16), (8, 32), (8, 64)])
def test_swap_attention_kernel_vs_float64(ws, dh):
    """Every supported (window_size, dim_head) pair, window and grid mode, L 2 and 5, maps 8 x 12 and 16 x 24 (those the window divides;
    X != Y, so a swapped partition shows), two heads, agent counts 1, L and one in between: against the float64 restatement built from the
    ``relative_position_index`` buffer the module registers, so the kernel's index arithmetic is checked against the buffer."""
    heads = 2
    rng = np.random.RandomState(100 * ws + dh)
    for L in (2, 5):
        att = Attention(heads * dh, dh, 0.0, L, ws)
        index = att.relative_position_index
        assert tuple(index.shape) == (L * ws * ws, L * ws * ws)
        nvalid = [1, L, max(1, L - 2)]
        for H, W in ((8, 12), (16, 24)):
            if H % ws or W % ws:
                continue
            qkv = rng.standard_normal((3 * L, 3 * heads * dh, H, W)).astype(np.float32)
            qkv[:, :heads * dh] *= 1.5                                  # scores of a few units: a softmax that is far from uniform
            table = rng.uniform(-1.0, 1.0, ((2 * L - 1) * (2 * ws - 1) ** 2, heads)).astype(np.float32)
            q_dev, t_dev = torch.from_numpy(qkv).to(DEV), torch.from_numpy(table).to(DEV)
            for grid in (0, 1):
                got = swap_attn_hip(q_dev, t_dev, nvalid, L, heads, dh, ws, grid).cpu().numpy()
                ref = R.swap_attention(torch.from_numpy(qkv).double().view(3, L, 3 * heads * dh, H, W), torch.from_numpy(table).double(),
                                       index, nvalid, L, ws, heads, bool(grid)).reshape(3 * L, heads * dh, H, W).numpy()
                assert np.isfinite(got).all(), f"ws {ws} dh {dh} L {L} {H}x{W} grid {grid}: output elements left unwritten"
                assert_close(got, ref, 1e-4, 1e-5, f"swap attention ws {ws} dh {dh} L {L} {H}x{W} grid {grid}")


def _module(args, seed):
    m = CoBEVT(args).eval()
    synth.fill_params_(m, seed)
    return m


@pytest.mark.parametrize("tag", list(R.CASES))
def test_module_vs_reference_golden(tag):
    """Every element against the reference's float32 output (the project's bar for HIP against reference goldens), and the rms-relative
    error against the reference's float64 output within twice the reference float32 run's own (floored at 1e-6)."""
    args, x, rl, aff, y32, y64, seed = load_cobevt_case(tag)
    m = _module(args, seed).to(DEV)
    with torch.no_grad():
        out = m(torch.from_numpy(x).to(DEV), torch.tensor(rl), torch.from_numpy(aff).to(DEV)).cpu().numpy()
    e_hip, e_ref = rel_rms(out, y64), rel_rms(y32, y64)
    print(f"cobevt case {tag}: rms-relative error against float64: HIP {e_hip:.3e}, reference float32 {e_ref:.3e}; "
          f"max abs against the float32 output {np.abs(out - y32).max():.3e}")
    assert_close(out, y32, 1e-4, 1e-5, f"CoBEVT HIP vs reference golden, case {tag}")
    assert e_hip <= max(2.0 * e_ref, 1e-6), (tag, e_hip, e_ref)


def test_module_vs_restatement_on_fresh_inputs():
    """Shapes that are not in the fixture: three scenes of 1, 5 and 2 agents (ego alone; a full scene), identity poses for the full one."""
    c = dict(C=64, dim_head=32, ws=4, L=5, H=12, W=8, depth=2, record_len=[1, 5, 2])
    args = R.case_args(c)
    m = _module(args, 77)
    rng = np.random.RandomState(78)
    x = np.maximum(rng.standard_normal((8, 64, 12, 8)), 0.0).astype(np.float32)
    aff = R.make_affine(c["record_len"], 5, 12, 8, 79, identity_scenes=(1,))
    with torch.no_grad():
        ref = R.cobevt_forward(m.state_dict(), args, torch.from_numpy(x).double(), c["record_len"], torch.from_numpy(aff)).numpy()
        out = m.to(DEV)(torch.from_numpy(x).to(DEV), c["record_len"], torch.from_numpy(aff).to(DEV)).cpu().numpy()
    assert_close(out, ref, 1e-4, 1e-5, "CoBEVT HIP vs float64 restatement, record_len [1, 5, 2]")


def test_calls_are_bit_identical_and_read_no_uninitialised_memory():
    """Two consecutive calls give the same bits. With every scene full (N_b = L) the padded buffer needs no zero rows; adding a scene
    that has some changes nothing in the full scenes' results, bit for bit, with NaNs planted in the allocator's free memory before
    every call."""
    c = dict(C=64, dim_head=32, ws=4, L=3, H=8, W=12, depth=1, record_len=[3, 3])
    args = R.case_args(c)
    m = _module(args, 5).to(DEV)
    rng = np.random.RandomState(6)
    x = torch.from_numpy(np.maximum(rng.standard_normal((7, 64, 8, 12)), 0.0).astype(np.float32)).to(DEV)
    aff = torch.from_numpy(R.make_affine([3, 3, 1], 3, 8, 12, 7)).to(DEV)
    with torch.no_grad():
        poison_allocator()
        a = m(x[:6], [3, 3], aff[:2]).clone()
        poison_allocator()
        b = m(x[:6], [3, 3], aff[:2]).clone()
        poison_allocator()
        c3 = m(x, [3, 3, 1], aff).clone()
    assert torch.isfinite(a).all() and torch.isfinite(c3).all()
    assert torch.equal(a, b)
    assert torch.equal(a, c3[:2])


def test_stage1_shell_with_cobevt_matches_the_restated_fusion():
    """Stage-1 shell with `fusion_method: cobevt` end to end on the small shell spec of test_shell.py: its cls_preds / reg_preds equal the
    same shell with the fusion net replaced by the restatement (run in float64 on the CPU), at the shell test's own tolerance."""
    from test_cobevt import _shell_args
    from gencomm_amd.heter_model_baseline_w_gencomm_stage1 import HeterModelBaselineWGenCommStage1 as Shell
    g = load_case("shell")
    args = _shell_args()
    model = Shell(copy.deepcopy(args)).eval()
    synth.fill_params_(model, int(g["weight_seed"]))
    synth.fill_bn_stats_(model, int(g["bn_seed"]))
    model = model.to(DEV)
    rl = [int(v) for v in g["record_len"]]
    pil = synth.make_pillars(int(g["M"]), sum(rl), int(g["nx"]), int(g["ny"]), int(g["data_seed"]), voxel_size=[0.4, 0.4, 4.0],
                             pc_range=args["lidar_range"])
    ptm = synth.make_pairwise_t_matrix(rl, 5, int(g["pose_seed"]), max_shift=float(g["max_shift"]))
    data = {"agent_modality_list": ["m1"] * sum(rl), "record_len": torch.tensor(rl), "pairwise_t_matrix": torch.from_numpy(ptm).to(DEV),
            "inputs_m1": {k: torch.from_numpy(pil[k]).to(DEV) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}}

    def run():
        with torch.no_grad(), shell_noise(model.gencomm, int(g["noise_seed"]), sum(rl), 128, 16, 32, DEV):
            return {k: v.cpu().numpy() for k, v in model(data).items() if k in ("cls_preds", "reg_preds")}

    hip = run()
    assert hip["cls_preds"].shape[0] == len(rl) and np.isfinite(hip["cls_preds"]).all()
    sd = {k: v.detach().cpu() for k, v in model.fusion_net.state_dict().items()}

    class Restated(torch.nn.Module):
        def forward(self, x, record_len, affine_matrix):
            y = R.cobevt_forward(sd, args["cobevt"], x.detach().cpu().double(), record_len, affine_matrix.cpu())
            return y.float().to(x.device)

    model.fusion_net = Restated()
    ref = run()
    for k in ("cls_preds", "reg_preds"):
        assert_close(hip[k], ref[k], 2e-4, 5e-5, f"stage-1 shell with cobevt: {k}")
