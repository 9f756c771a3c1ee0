"""Training the max fusion and the who2com fusion on the GPU: gencomm_warp_maxfuse_bwd against float64 and against the reference's
float32 CPU gradient (winners on exact ties), determinism on rigid transforms, MaxFusion under autograd, Who2comFusion against the
reference's own outputs and gradients (tests/golden/who2com.npz), and one stage-1 training step with each fusion.

Criterion of the float64 comparisons, as tests/test_gpu_lss_train.py: relative rms error <= 2 x the error of the fp32 ATen autograd of
the same restatement against the same float64 result, floored at 1e-6. Output elements whose float64 top two warped values are
closer than 1e-5 max|x| without being equal (near ties: float32 may pick the other agent) are excluded by zeroing the probe there; their
share is asserted to stay under 1e-3. Exact ties are never excluded."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import fusion_train_restatement as R
from helpers import GOLDEN, assert_close, load_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _hip_max_grad(x, rl, affine, G):
    from gencomm_amd import MaxFusion
    xx = torch.from_numpy(x).to(DEV).requires_grad_(True)
    out = MaxFusion()(xx, torch.tensor(rl), torch.from_numpy(affine).to(DEV))
    out.backward(torch.from_numpy(G).to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), xx.grad.cpu().numpy()


def _check_against_references(name, x, rl, affine, G, res, got_out, got):
    (o64, d64), (o32, d32) = res[torch.float64], res[torch.float32]
    assert np.isfinite(got).all()
    assert R.rel_rms(got_out, o64) <= 1e-5
    e_hip, e_aten = R.rel_rms(got, d64), R.rel_rms(d32, d64)
    print(f"maxfuse backward {name}: relative rms error against float64: HIP {e_hip:.3e}, fp32 ATen {e_aten:.3e}")
    assert e_hip <= max(2.0 * e_aten, 1e-6), (name, e_hip, e_aten)


@pytest.mark.parametrize("name", list(R.CASES))
def test_maxfuse_backward_vs_float64_and_cpu_winners(name):
    """Measured on MI355X, relative rms error against float64, HIP (fp32 ATen autograd of the same restatement), near-tie share:
        identity_ties   6.30e-16 (2.77e-07)   0
        rigid_relu      8.54e-07 (2.36e-06)   6.2e-05
        halfpix_quant   1.10e-07 (1.88e-07)   0
        max_agents      1.74e-06 (2.37e-06)   9.5e-05
        nontame         4.60e-07 (4.90e-07)   0"""
    C, H, W, rl, kind, rigid = R.CASES[name]
    x, rl, affine, G = R.build_case(name)
    near = R.near_tie_mask(x, rl, affine).numpy()
    share = float(near.mean())
    print(f"maxfuse backward {name}: near-tie share {share:.3e}")
    assert share <= R.NEAR_TIE_CAP
    G = G * ~near
    res = R.reference_grads(x, rl, affine, G)
    got_out, got = _hip_max_grad(x, rl, affine, G)
    _check_against_references(name, x, rl, affine, G, res, got_out, got)
    d32 = res[torch.float32][1]
    if kind in ("equal", "relu", "quant"):
        # The winners are those of the reference's float32 CPU gradient (lowest agent index on exact ties). One other winner moves
        # a tap of weight >= 1/4 times |G| >= 1/4 from one agent to another; float32 rounding moves 1e-6 of that. The supports are
        # compared above the rounding residue of cells that touch a lattice point (a tap of weight ~1e-6 exists in one float32
        # evaluation order and not in another): wherever one gradient is larger than 2e-4 the other is not zero.
        assert np.abs(got - d32).max() <= 1e-4, (name, float(np.abs(got - d32).max()))
        assert np.all(got[np.abs(d32) > 2e-4] != 0) and np.all(d32[np.abs(got) > 2e-4] != 0)
        off = np.cumsum([0] + rl)
        for b in range(len(rl)):
            for j in range(off[b], off[b + 1]):
                if not d32[j].any():
                    assert not got[j].any(), (name, "agent", j, "wins nowhere in the reference: exact zeros")
    if kind == "equal":      # all-agent ties everywhere: the ego takes everything, bit for bit
        ego = np.cumsum([0] + rl[:-1])
        assert np.array_equal(got[ego], G)
        assert np.count_nonzero(np.delete(got, ego, axis=0)) == 0
    if kind == "quant":      # exact non-zero ties between agents 1 and 2 (same transform, equal rows): agent 1 takes them
        assert np.count_nonzero(got[1, :, 0:4]) > 0 and np.count_nonzero(got[2, :, 0:3]) == 0 and np.count_nonzero(got[2, :, 9:11]) == 0
        assert np.count_nonzero(got[2, :, 5:8]) > 0 and np.count_nonzero(got[1, :, 5:8]) == 0      # one higher: agent 2 wins or the ego
    if rigid:                # no float atomics on these paths: two runs are bit-identical
        _, again = _hip_max_grad(x, rl, affine, G)
        assert np.array_equal(got, again)


def test_maxfuse_backward_vs_the_reference_fixture():
    g = load_case("maxfuse_train")
    rl = [int(v) for v in g["record_len"]]
    assert float(g["near_tie_share"]) <= R.NEAR_TIE_CAP
    got_out, got = _hip_max_grad(g["x"], rl, g["affine"], g["G"])
    e_hip, e_ref = R.rel_rms(got, g["dx64"]), R.rel_rms(g["dx32"], g["dx64"])
    print(f"maxfuse backward fixture: relative rms error against the reference's float64 gradient: HIP {e_hip:.3e}, reference float32 {e_ref:.3e}")
    assert_close(got_out, g["out32"], 1e-4, 1e-5, "max fusion forward")
    assert e_hip <= max(2.0 * e_ref, 1e-6)
    assert np.abs(got - g["dx32"]).max() <= 1e-4
    assert np.count_nonzero(got[4]) == 0          # scene 1's agent outside the map ties at 0 with its neighbour and never wins


def test_maxfuse_backward_without_scratch_scatters_every_agent():
    """scratch == NULL: no plan, no winner map, every agent takes the float atomics; same gradient."""
    from gencomm_amd import _lib
    from gencomm_amd.fusion import gather_ego_thetas
    from gencomm_amd.runtime import dev_ints, ptr, stream_ptr
    x, rl, affine, G = R.build_case("rigid_relu")
    G = G * ~R.near_tie_mask(x, rl, affine).numpy()
    _, want = _hip_max_grad(x, rl, affine, G)
    xx, gg = torch.from_numpy(x).to(DEV), torch.from_numpy(G).to(DEV)
    theta = gather_ego_thetas(torch.from_numpy(affine), rl).to(DEV)
    off = dev_ints(list(np.cumsum([0] + rl)), DEV)
    gx = torch.full_like(xx, float("nan"))
    n, C, H, W = xx.shape
    _lib.check(_lib.lib().gencomm_warp_maxfuse_bwd(ptr(xx), ptr(theta), ptr(off), ptr(gg), ptr(gx), None, len(rl), n, C, H, W, stream_ptr(DEV)),
               "gencomm_warp_maxfuse_bwd")
    torch.cuda.synchronize()
    got = gx.cpu().numpy()
    res = R.reference_grads(x, rl, affine, G)
    e_hip, e_aten = R.rel_rms(got, res[torch.float64][1]), R.rel_rms(res[torch.float32][1], res[torch.float64][1])
    print(f"maxfuse backward, scatter only: relative rms error against float64: HIP {e_hip:.3e}, fp32 ATen {e_aten:.3e}")
    assert e_hip <= max(2.0 * e_aten, 1e-6)
    # Against the gather path: the identity ego is written at its own pixel there, while the scatter applies the float32 cell of the
    # identity warp, whose coordinate ((g + 1) W - 1) / 2 carries up to W 2^-23 of rounding (two roundings of 2^-24 scaled by W / 2 ... W):
    # a tap-weight residue of that size times |G| moves to a neighbouring pixel.
    atol = W * 2.0 ** -22 * float(np.abs(G).max())
    assert_close(got, want, 1e-5, atol, "scatter path against the gather path")


def test_max_fusion_under_autograd():
    from gencomm_amd import MaxFusion
    x, rl, affine, G = R.build_case("rigid_relu")
    fus, aff = MaxFusion(), torch.from_numpy(affine).to(DEV)
    xx = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        plain = fus(xx, rl, aff)
    assert not fus(xx, rl, aff).requires_grad                     # an input without a gradient still takes the old path
    xg = xx.clone().requires_grad_(True)
    out = fus(xg, rl, aff)
    assert out.requires_grad and torch.equal(out.detach(), plain)   # bit for bit the no-grad output
    (out * torch.from_numpy(G).to(DEV)).sum().backward()
    assert xg.grad is not None and xg.grad.shape == xg.shape and torch.isfinite(xg.grad).all() and torch.count_nonzero(xg.grad) > 0
    with pytest.raises(ValueError):
        fus(xg, [9], aff[:1])


def test_who2com_forward_and_gradients_vs_the_reference_fixture():
    """Tolerances of the Where2comm fixture tests: rtol 1e-4 / atol 1e-5 forward, 2e-4 / 2e-5 gradients, against the reference's float32
    values."""
    from gencomm_amd import Who2comFusion
    g = load_case("who2com")
    rl = [int(v) for v in g["record_len"]]
    net = Who2comFusion(int(g["x"].shape[1]))
    with torch.no_grad():
        net.decode_layer.weight.copy_(torch.from_numpy(g["weight"]))
        net.decode_layer.bias.copy_(torch.from_numpy(g["bias"]))
    net = net.to(DEV)
    x, aff = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["affine"]).to(DEV)
    with torch.no_grad():
        plain = net(x, torch.tensor(rl), aff)
    assert list(plain.shape) == list(g["out32"].shape)
    assert_close(plain.cpu().numpy(), g["out32"], 1e-4, 1e-5, "who2com HIP forward")
    xg = x.clone().requires_grad_(True)
    out = net(xg, torch.tensor(rl), aff)
    assert torch.equal(out.detach(), plain)
    (out * torch.from_numpy(g["G"]).to(DEV)).sum().backward()
    for name, got, want in (("dx", xg.grad, g["dx32"]), ("d weight", net.decode_layer.weight.grad, g["gw32"]), ("d bias", net.decode_layer.bias.grad, g["gb32"])):
        got = got.cpu().numpy()
        print(f"who2com {name}: relative rms error against float64: HIP {R.rel_rms(got, g[{'dx': 'dx64', 'd weight': 'gw64', 'd bias': 'gb64'}[name]]):.3e}, "
              f"reference float32 {R.rel_rms(want, g[{'dx': 'dx64', 'd weight': 'gw64', 'd bias': 'gb64'}[name]]):.3e}")
        assert_close(got, want, 2e-4, 2e-5, "who2com HIP " + name)


@pytest.mark.parametrize("method", ["max", "who2com"])
def test_stage1_training_step_with_the_fusion(method):
    """One stage-1 training step on the synthetic batch of tests/test_shell.py with the loss of
    tests/test_gpu_backward.py::test_stage1_training_step_reaches_every_trained_module: every trainable parameter upstream of the fusion
    (and who2com's decode_layer) receives a finite, non-zero gradient."""
    from gencomm_amd import synth
    from gencomm_amd.heter_model_baseline_w_gencomm_stage1 import HeterModelBaselineWGenCommStage1
    g = load_case("shell")
    with open(os.path.join(GOLDEN, "shell_state_dict_keys.json")) as f:
        args = copy.deepcopy(json.load(f)["args"])
    args["fusion_method"] = method
    if method == "who2com":
        args["who2com"] = 128
    model = HeterModelBaselineWGenCommStage1(args)
    synth.fill_params_(model, int(g["weight_seed"]))
    synth.fill_bn_stats_(model, int(g["bn_seed"]))
    model = model.to(DEV).train()
    rl = [int(v) for v in g["record_len"]]
    pil = synth.make_pillars(int(g["M"]), sum(rl), int(g["nx"]), int(g["ny"]), int(g["data_seed"]), voxel_size=[0.4, 0.4, 4.0], pc_range=args["lidar_range"])
    ptm = synth.make_pairwise_t_matrix(rl, 5, int(g["pose_seed"]), max_shift=float(g["max_shift"]))
    data = {"agent_modality_list": ["m1"] * sum(rl), "record_len": torch.tensor(rl), "pairwise_t_matrix": torch.from_numpy(ptm).to(DEV),
            "inputs_m1": {k: torch.from_numpy(pil[k]).to(DEV) for k in ("voxel_features", "voxel_coords", "voxel_num_points")}}
    out = model(data)
    loss = (out["cls_preds"].square().mean() + out["reg_preds"].square().mean() + out["dir_preds"].square().mean()
            + (out["pred_feature"] - out["gt_feature"].detach()).square().mean())
    loss.backward()
    upstream = ("encoder_m1.", "backbone_m1.", "shrinker_m1.", "message_extractor_m1.", "gencomm.", "enhancer.", "fusion_net.")
    checked = 0
    dead = {n for n, _ in model.enhancer.named_parameters() if not n.startswith(("block_1.norm", "block_1.mlp", "split_attn"))}   # never run by the reference's forward
    for n, p in model.named_parameters():
        if not p.requires_grad or not n.startswith(upstream) or (n.startswith("enhancer.") and n[len("enhancer."):] in dead):
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0.0, n
        checked += 1
    assert checked > 40
    if method == "who2com":
        assert float(model.fusion_net.decode_layer.weight.grad.abs().sum()) > 0 and float(model.fusion_net.decode_layer.bias.grad.abs().sum()) > 0
    print(f"stage-1 training step with fusion_method {method}: loss {float(loss):.4f}, {checked} upstream parameters with a non-zero gradient")
