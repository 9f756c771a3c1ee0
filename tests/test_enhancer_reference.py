"""Pins tests/enhancer_reference.py, the float64 truth of test_gpu_enhancer_kernels.py: its composition against oracle/torch_port.py in
float64, against the golden Enhancer outputs (recorded from the reference's own module) in float32, and the depthwise stage's padding on a
3 x 3 map against sums written out by hand. CPU only."""
import math

import pytest
import torch

import enhancer_reference as R
from helpers import assert_close, build_inputs, build_modules, eval_noise, load_case, sub
from oracle import torch_port as O


@pytest.mark.parametrize("n,C,H,W", [(2, 16, 5, 7), (1, 24, 3, 3), (3, 64, 9, 4), (1, 40, 1, 6)])
def test_float64_composition_equals_the_oracle(n, C, H, W):
    sd = R.random_sd(C, 100 + C)
    x = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(C + H)).double()
    r = R.forward(sd, x, torch.float64)
    ref = O.enhancer_forward({k: v.double() for k, v in sd.items()}, x, [n])
    assert r["out"].shape == ref.shape == (n, C, H, W)
    assert float((r["out"] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    # the intermediates are what their names say
    assert r["x1"].shape == r["x2"].shape == r["G"].shape == (n, H, W, 2 * C) and r["Hd"].shape == (n, H, W, 4 * C)
    assert torch.equal(r["Z"][..., C // 4:], r["Zln"][..., C // 4:])           # channels >= dc pass the partial convolution untouched
    assert torch.allclose(r["mean"], r["O"].mean((1, 2)), rtol=1e-13, atol=1e-13)
    assert torch.equal(r["out"], (r["O"] * r["gate"][:, None, None, :]).permute(0, 3, 1, 2))


@pytest.mark.parametrize("name", ["tiny", "ragged", "mid"])
def test_float32_reproduces_the_golden_enhancer_outputs(name):
    """The fixtures hold the reference module's `enhanced` (strided) for the prediction its own GenComm produced: the oracle regenerates
    that prediction, this module enhances it scene by scene in float32, at the fixtures' own tolerance (test_oracle_golden.py)."""
    g = load_case(name)
    cfg, gen, enh = build_modules(g)
    inp = build_inputs(g)
    n0, sn = eval_noise(g)
    H, W, px = int(g["H"]), int(g["W"]), float(g["px_m"])
    sd_g = {k: v.detach() for k, v in gen.state_dict().items()}
    with torch.no_grad():
        pred = O.path_forward(sd_g, None, cfg, inp["feat"], inp["cond"], inp["record_len"], inp["pairwise_t_matrix"], H * px, W * px, n0, sn)["pred_feature"]
        sd = {k: v.detach() for k, v in enh.state_dict().items()}
        out, o = [], 0
        for n in O.regroup_lens(inp["record_len"]):
            out.append(R.forward(sd, pred[o:o + n], torch.float32)["out"])
            o += n
    assert_close(sub(torch.cat(out, 0), int(g["stride"])), g["enhanced"], 1e-5, 1e-6, "enhanced")


def _gelu(v):
    return 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))


def test_depthwise_stage_pads_gelu_x1_with_zeros_not_with_gelu_of_the_bias():
    """3 x 3 map, C = 8, Linear1 bias of order 1. Corner (0, 0) of G written out by hand: the depthwise convolution sees five taps outside
    the image, where its input GELU(x1) is ZERO. A kernel that recomputes Linear1 on halo pixels from zero tokens would put GELU(bias)
    there instead (what a zero token gives); that corner value must be more than 1e-3 away, or the GPU tests could not tell the two."""
    C, H, W = 8, 3, 3
    hid = 2 * C
    sd = R.cast(R.random_sd(C, 7, bias1=1.0), torch.float64)
    x = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(8)).double()
    r = R.forward(sd, x, torch.float64)
    Hd, dw, db, b1 = r["Hd"][0], sd[R.PM + "dwconv.0.weight"], sd[R.PM + "dwconv.0.bias"], sd[R.PM + "linear1.0.bias"]
    worst = 0.0
    for (y, xx) in ((0, 0), (0, 2), (2, 0), (2, 2), (1, 1), (0, 1)):
        for ch in range(hid):
            s_zero, s_bias = float(db[ch]), float(db[ch])
            for dy in range(3):
                for dx in range(3):
                    yy, xs = y - 1 + dy, xx - 1 + dx
                    inside = 0 <= yy < H and 0 <= xs < W
                    wv = float(dw[ch, 0, dy, dx])
                    s_zero += wv * (float(Hd[yy, xs, ch]) if inside else 0.0)
                    s_bias += wv * (float(Hd[yy, xs, ch]) if inside else _gelu(float(b1[ch])))
            g_zero, g_bias = _gelu(s_zero) * float(Hd[y, xx, hid + ch]), _gelu(s_bias) * float(Hd[y, xx, hid + ch])
            assert abs(g_zero - float(r["G"][0, y, xx, ch])) <= 1e-12 * max(1.0, abs(g_zero)), (y, xx, ch)
            if (y, xx) == (0, 0):
                worst = max(worst, abs(g_zero - g_bias))
            if (y, xx) == (1, 1):
                assert g_zero == g_bias                                    # the centre pixel has no tap outside
    assert worst > 1e-3, worst


def test_subsets_name_the_edges():
    m = R.subsets(2, 21, 37, 16, 16)
    assert set(m) == {"border ring", "last partial tile in x (16)", "last partial tile in y (16)", "agent 0", "agent 1"}
    assert int(m["border ring"][0].sum()) == 2 * 37 + 2 * 19 and int(m["last partial tile in x (16)"][0].sum()) == 21 * 5
    assert int(m["last partial tile in y (16)"][1].sum()) == 5 * 37 and "agent 0" not in R.subsets(1, 8, 8, 8, 8)
