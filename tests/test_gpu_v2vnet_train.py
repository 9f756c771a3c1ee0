"""Training of the V2VNet fusion on the GPU: the four new kernels called directly through the C ABI, each against torch autograd of the
same operation in float64 on the CPU, then `V2VNetFusion(args, trainable=True)` against the reference's stored float64 gradients
(tests/golden/v2vnet_train.npz, v2vnet_train_d.npz), a scene of eight agents, determinism, frozen parameters / input, and the rebuild of
the prepared weights after an optimizer step.

Kernel criterion (as test_gpu_v2vnet.py): truth = float64 autograd on the CPU, yardstick = the same in float32; the kernel's relative rms
error against the truth <= max(2 x the yardstick's, 1e-6). Outputs are pre-filled with NaN, so an element left unwritten fails the test."""
import math

import numpy as np
import pytest
import torch

import fusion_train_restatement as FR
import v2vnet_restatement as R
import v2vnet_train_restatement as TR
from test_gpu_v2vnet import DEV, SHAPES, _call, _check, _ints, _p, _st, _thetas

pytestmark = pytest.mark.gpu


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _poison():
    junk = torch.full((8 << 20,), float("nan"), device=DEV)   # NaNs in the memory the allocator hands out next
    del junk


# ---- gencomm_gru_gate_bwd -----------------------------------------------------------------------------------------------------------
def _gate_grad(g, dh):
    g = g.clone().requires_grad_()
    R.gate(g).backward(dh)
    return g.grad


@pytest.mark.parametrize("n,C,HW", [(3, 5, 63), (2, 8, 240)])
def test_gru_gate_bwd_vs_float64(n, C, HW):
    rng = np.random.RandomState(HW + 1)
    g = torch.from_numpy((2.0 * rng.standard_normal((n, 2 * C, HW))).astype(np.float32))
    g[0, 0, :4] = torch.tensor([-30.0, 30.0, 0.0, -0.0])       # a saturated update gate ...
    g[0, C, :4] = torch.tensor([30.0, -30.0, 1e-4, 0.5])       # ... and a saturated candidate
    g[1, 1, :2], g[1, C + 1, :2] = torch.tensor([30.0, -30.0]), torch.tensor([0.3, -0.7])
    dh = torch.from_numpy(rng.standard_normal((n, C, HW)).astype(np.float32))
    dg = _nan(n, 2 * C, HW)
    gd, dd = g.to(DEV), dh.to(DEV)
    _call("gencomm_gru_gate_bwd", _p(gd), _p(dd), _p(dg), n, C, HW, _st())
    got = dg.cpu()
    _check(f"gru_gate_bwd n {n} C {C} HW {HW}", got.numpy(), _gate_grad(g.double(), dh.double()).numpy(), _gate_grad(g, dh).numpy())
    sat = torch.stack([got[0, 0, :2], got[0, C, :2], got[1, 1, :2]])          # where the gate saturates: finite and tiny, not NaN
    assert torch.isfinite(sat).all() and float(sat.abs().max()) <= 1e-9


# ---- gencomm_v2v_aggregate_train_fwd / gencomm_v2v_aggregate_bwd --------------------------------------------------------------------
def _agg_inputs(C, H, W, seed):
    """test_gpu_v2vnet._aggregate_case with seeded values: nodes of 1, 3 and 8 pairs; the 3-pair node's other agents are off the map."""
    rng = np.random.RandomState(1000 * seed + C * H)
    I, _, half, off = _thetas(H, W)
    rigid = [FR.rot(H, W, rng.uniform(-math.pi, math.pi), *rng.uniform(-0.3 * W, 0.3 * W, 2)) for _ in range(6)]
    theta = np.stack([I] + [I, off, FR.theta(H, W, ty=-2.0 * H - 0.37)] + [I, half] + rigid)
    y = torch.from_numpy(rng.standard_normal((12, C, H, W)).astype(np.float32))
    e = torch.from_numpy(rng.standard_normal((3, C, H, W)).astype(np.float32))
    h = torch.from_numpy(rng.standard_normal((5, C, H, W)).astype(np.float32))
    return y, e, h, torch.from_numpy(theta), [4, 0, 2], [0, 1, 4, 12]


def _live_winners(y, e, theta, pair_off):
    """Per node: (float64 winner map, live positions, smallest float64 margin over them)."""
    mask = R.warp(torch.ones(y.shape[0], 1, *y.shape[2:], dtype=torch.float64), theta)
    out = []
    for k in range(len(pair_off) - 1):
        a, b = pair_off[k], pair_off[k + 1]
        m = (y[a:b].double() + e[k:k + 1].double()) * mask[a:b]
        if b - a == 1:
            out.append((torch.zeros(m.shape[1:], dtype=torch.int64), torch.ones(m.shape[1:], dtype=torch.bool), float("inf")))
            continue
        win, run = TR.winners(m)
        mk = mask[a:b].expand_as(m)
        on = (mk.gather(0, win[None])[0] > 0) | (mk.gather(0, run[None])[0] > 0)
        gap = (m.gather(0, win[None]) - m.gather(0, run[None]))[0]
        out.append((win, on, float(gap[on].min()) if on.any() else float("inf")))
    return out


_QUALIFIED = {}


def _qualified_inputs(C, H, W):
    """The first of the seeds 0..7 whose float64 margin between winner and runner-up is >= 1e-4 at every live position."""
    if (C, H, W) not in _QUALIFIED:
        for seed in range(8):
            case = _agg_inputs(C, H, W, seed)
            wins = _live_winners(case[0], case[1], case[3], case[5])
            print(f"aggregate inputs C {C} {H}x{W} seed {seed}: smallest live margin {min(w[2] for w in wins):.3e}")
            if min(w[2] for w in wins) >= 1e-4:
                _QUALIFIED[(C, H, W)] = (case, wins)
                break
        else:
            pytest.fail("none of the seeds 0..7 has a float64 margin >= 1e-4 at every live position")
    return _QUALIFIED[(C, H, W)]


def _train_fwd(dev, winner, n_nodes, C, H, W, op, out_mode):
    out = _nan(n_nodes, C if out_mode else 2 * C, H, W)
    _call("gencomm_v2v_aggregate_train_fwd", *[_p(t) for t in dev], _p(out), _p(winner), n_nodes, C, H, W, op, out_mode, _st())
    return out


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_aggregate_train_fwd_bits_and_winner_map(C, H, W):
    (y, e, h, theta, node_row, pair_off), wins = _qualified_inputs(C, H, W)
    dev = [t.to(DEV) for t in (y, e, h, theta)] + [_ints(node_row), _ints(pair_off)]
    for op in (0, 1):
        for out_mode in (0, 1):
            ref = _nan(3, C if out_mode else 2 * C, H, W)
            _call("gencomm_v2v_aggregate_fwd", *[_p(t) for t in dev], _p(ref), 3, C, H, W, op, out_mode, _st())
            winner = torch.full((3, C, H, W), 255, dtype=torch.uint8, device=DEV) if op == 1 else None     # null is allowed for the mean
            out = _train_fwd(dev, winner, 3, C, H, W, op, out_mode)
            assert torch.isfinite(ref).all() and torch.equal(out, ref), (op, out_mode)                    # the inference entry's bits
            if op == 1:
                got = winner.cpu().long()
                for k, (win, on, _) in enumerate(wins):
                    assert int(got[k].max()) < pair_off[k + 1] - pair_off[k]                              # every element written, in range
                    assert torch.equal(got[k][on], win[on]), k                                             # = argmax of the float64 messages


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_aggregate_train_fwd_exact_tie_goes_to_the_lower_index(C, H, W):
    rng = np.random.RandomState(7)
    I, _, half, _ = _thetas(H, W)
    theta = torch.from_numpy(np.stack([half, I, I]))             # pairs 1 and 2 carry the same values under a mask of exactly 1
    y = torch.from_numpy(rng.standard_normal((3, C, H, W)).astype(np.float32))
    y[0] = -100.0
    y[2] = y[1]
    e = torch.from_numpy(rng.standard_normal((1, C, H, W)).astype(np.float32))
    h = torch.zeros(1, C, H, W)
    dev = [t.to(DEV) for t in (y, e, h, theta)] + [_ints([0]), _ints([0, 3])]
    winner = torch.full((1, C, H, W), 255, dtype=torch.uint8, device=DEV)
    _train_fwd(dev, winner, 1, C, H, W, 1, 0)
    m = (y + e) * R.warp(torch.ones(3, 1, H, W), theta)
    assert torch.equal(m[1], m[2]) and bool((m[1] > m[0]).all())
    assert bool((winner.cpu() == 1).all())


def _agg_grads(y, e, h, theta, node_row, pair_off, op, out_mode, dout):
    y, e = y.clone().requires_grad_(), e.clone().requires_grad_()
    R.aggregate(y, e, h, theta, node_row, pair_off, op, out_mode).backward(dout)
    return y.grad, e.grad


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_aggregate_bwd_vs_float64(C, H, W):
    (y, e, h, theta, node_row, pair_off), _ = _qualified_inputs(C, H, W)
    dev = [t.to(DEV) for t in (y, e, h, theta)] + [_ints(node_row), _ints(pair_off)]
    rng = np.random.RandomState(C + W)
    for op in (0, 1):
        for out_mode in (0, 1):
            dout = torch.from_numpy(rng.standard_normal((3, C if out_mode else 2 * C, H, W)).astype(np.float32))
            winner = torch.full((3, C, H, W), 255, dtype=torch.uint8, device=DEV) if op == 1 else None
            _train_fwd(dev, winner, 3, C, H, W, op, out_mode)
            dy, de, dd = _nan(12, C, H, W), _nan(3, C, H, W), dout.to(DEV)
            _call("gencomm_v2v_aggregate_bwd", _p(dd), _p(dev[3]), _p(dev[4]), _p(dev[5]), _p(winner), _p(dy), _p(de), 3, C, H, W, op, out_mode, _st())
            ty, te = _agg_grads(y.double(), e.double(), h.double(), theta, node_row, pair_off, op, out_mode, dout.double())
            fy, fe = _agg_grads(y, e, h, theta, node_row, pair_off, op, out_mode, dout)
            what = f"aggregate_bwd C {C} {H}x{W} op {op} out_mode {out_mode}"
            _check(what + " dy", dy.cpu().numpy(), ty.numpy(), fy.numpy())
            _check(what + " de", de.cpu().numpy(), te.numpy(), fe.numpy())
            assert float(dy[2:4].abs().max()) == 0.0 and float(ty[2:4].abs().max()) == 0.0        # the off-map pairs: exact zeros


# ---- gencomm_v2v_warp_pairs_bwd -----------------------------------------------------------------------------------------------------
def _warp_grad(x, src, theta, dwarped):
    x = x.clone().requires_grad_()
    R.warp(x[src], theta).backward(dwarped)
    return x.grad


def _warp_bwd(dwarped, theta, src, rows, C, H, W, accumulate, base=None):
    from gencomm_amd import _lib
    from gencomm_amd.v2vnet import pairs_by_source_row
    P = len(src)
    rpo, rp = pairs_by_source_row(src, rows)
    dx = base.to(DEV).clone() if accumulate else _nan(rows, C, H, W)
    scratch = torch.empty(_lib.check_size(_lib.lib().gencomm_v2v_warp_pairs_bwd_scratch_floats(P), "scratch"), device=DEV)
    keep = [dwarped.to(DEV), theta.to(DEV), _ints(src), _ints(rpo), _ints(rp)]
    _call("gencomm_v2v_warp_pairs_bwd", *[_p(t) for t in keep], _p(dx), _p(scratch), P, rows, C, H, W, accumulate, _st())
    return dx.cpu()


def _warp_cases(H, W):
    I, rot, half, off = _thetas(H, W)
    rng = np.random.RandomState(H)
    rigid = [FR.rot(H, W, rng.uniform(-math.pi, math.pi), *rng.uniform(-0.3 * W, 0.3 * W, 2)) for _ in range(8)]
    zoom = FR.theta(H, W)
    zoom[:, :2] *= 0.5                                           # magnifies by 2: a source pixel feeds about 16 outputs -> not tame
    src13 = [0] + [1 + j for _ in range(3) for j in range(3)]    # the pair table of record_len [1, 3]
    th13 = [I] + [I, rot, half] + [rigid[0], I, off] + [rigid[1], rigid[2], I]
    return {"record_len [1, 3]": (src13, 4, np.stack(th13), True),
            "fan-in 8": ([0] * 8, 2, np.stack([I, rot, half, off] + rigid[3:7]), True),      # row 1 is read by no pair
            "zoom (scatter)": ([0, 1, 1, 0], 2, np.stack([zoom, I, rot, half]), False)}


@pytest.mark.parametrize("C,H,W", SHAPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_warp_pairs_bwd_vs_float64(C, H, W, accumulate):
    for name, (src, rows, theta, tame) in _warp_cases(H, W).items():
        rng = np.random.RandomState(len(src) * W)
        theta = torch.from_numpy(theta)
        dwarped = torch.from_numpy(rng.standard_normal((len(src), C, H, W)).astype(np.float32))
        base = torch.from_numpy(rng.standard_normal((rows, C, H, W)).astype(np.float32))
        x = torch.zeros(rows, C, H, W)
        truth, yard = _warp_grad(x.double(), src, theta, dwarped.double()), _warp_grad(x, src, theta, dwarped)
        if accumulate:
            truth, yard = truth + base.double(), yard + base
        got = _warp_bwd(dwarped, theta, src, rows, C, H, W, accumulate, base)
        _check(f"warp_pairs_bwd {name} C {C} {H}x{W} accumulate {accumulate}", got.numpy(), truth.numpy(), yard.numpy())
        if name == "fan-in 8":                                   # the row no pair reads: zeros, or what it held
            assert torch.equal(got[1], base[1] if accumulate else torch.zeros(C, H, W))
        if tame:
            _poison()
            assert torch.equal(got, _warp_bwd(dwarped, theta, src, rows, C, H, W, accumulate, base)), name    # one writer per element


# ---- gencomm_conv2d_wgrad_fixed (the weight gradient the training path uses) ---------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,k,H,W", [(26, 8, 8, 3, 6, 10),      # 26 workgroups per channel pair, below the direct-atomics threshold
                                              (3, 16, 12, 1, 7, 9),       # 1x1, ragged channel chunks
                                              (2, 6, 5, 3, 40, 70),       # several tiles per sample
                                              (3, 32, 64, 3, 8, 12),      # the wide 3x3 split-K route
                                              (2, 32, 32, 1, 8, 12)])     # a wide 1x1 layer: the chunk kernel, not the atomics GEMM
def test_conv2d_wgrad_fixed_vs_float64_and_two_runs(n, cin, cout, k, H, W):
    import torch.nn.functional as F
    from gencomm_amd import train_ops as T
    rng = np.random.RandomState(n * cin + k)
    x = torch.from_numpy(rng.standard_normal((n, cin, H, W)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((n, cout, H, W)).astype(np.float32))

    def grads(dt):
        w = torch.zeros(cout, cin, k, k, dtype=dt, requires_grad=True)
        b = torch.zeros(cout, dtype=dt, requires_grad=True)
        F.conv2d(x.to(dt), w, b, padding=k // 2).backward(dy.to(dt))
        return w.grad.numpy(), b.grad.numpy()

    (tw, tb), (yw, yb) = grads(torch.float64), grads(torch.float32)
    xd, dd = x.to(DEV), dy.to(DEV)
    _poison()
    dw, db = T.conv2d_wgrad_fixed(dd, xd, k, True)
    dw, db = dw.clone(), db.clone()
    _check(f"wgrad_fixed {n}x{cin}->{cout} k{k} {H}x{W} dw", dw.cpu().numpy(), tw, yw)
    _check(f"wgrad_fixed {n}x{cin}->{cout} k{k} {H}x{W} db", db.cpu().numpy(), tb, yb)
    _poison()
    dw2, db2 = T.conv2d_wgrad_fixed(dd, xd, k, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dw3, none = T.conv2d_wgrad_fixed(dd, xd, k, False)
    assert none is None and torch.equal(dw3, dw)


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def _module(args, sd, trainable=True):
    from gencomm_amd import V2VNetFusion
    m = V2VNetFusion(args, trainable=trainable).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _step(m, c, x_grad=True):
    """One forward + backward of a fixture case: (out, d x or None, {name: gradient or None})."""
    m.zero_grad(set_to_none=True)
    x = torch.from_numpy(c["x"]).to(DEV).requires_grad_(x_grad)
    out = m(x, c["record_len"], torch.from_numpy(c["affine"]).to(DEV))
    out.backward(torch.from_numpy(c["grad_out"]).to(DEV))
    return out.detach(), x.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


@pytest.mark.parametrize("tag", TR.TRAIN_CASES)
def test_module_gradients_vs_reference_golden(tag):
    """Every gradient against the reference's float64 gradient: relative rms <= max(2 x the reference float32 run's own, 1e-6)."""
    c = TR.load_train_case(tag)
    m = _module(c["args"], c["sd"])
    out, dx, grads = _step(m, c)
    with torch.no_grad():
        plain = _module(c["args"], c["sd"], trainable=False)(torch.from_numpy(c["x"]).to(DEV), c["record_len"], torch.from_numpy(c["affine"]).to(DEV))
    assert torch.equal(out, plain)                               # the training forward has the inference forward's bits
    C = c["args"]["in_channels"]
    worst = []
    for name, got in [("x", dx)] + list(grads.items()):
        if name != "x" and name not in c["g64"]:
            assert got is None, name                             # absent in the reference: None here
            continue
        want = c["gx64"] if name == "x" else c["g64"][name]
        assert got is not None and tuple(got.shape) == want.shape and torch.isfinite(got).all(), name
        e = R.rel_rms(got.cpu().numpy(), want)
        print(f"v2vnet training case {tag} {name}: HIP rel rms {e:.3e}, reference float32 {c['ref'][name]:.3e}")
        worst.append((e <= max(2.0 * c["ref"][name], 1e-6), name, e, c["ref"][name]))
        if name.startswith("conv_gru."):
            assert all(float(b.abs().max()) == 0.0 for b in TR.reset_and_hidden_blocks(name, got, C)), name     # exact zeros, as tensors
    assert all(w[0] for w in worst), [w for w in worst if not w[0]]
    if tag == "bt":
        assert float(dx[sum(TR.BT["record_len"][:2]) + 3].abs().max()) == 0.0        # the off-map agent


def test_single_scene_of_eight_agents_vs_restatement_autograd():
    c = dict(C=8, H=8, W=12, agg="avg", gru=True, layers=1, iters=2)
    args = R.case_args(c)
    from gencomm_amd import V2VNetFusion, synth
    m = V2VNetFusion(args, trainable=True).eval()
    synth.fill_params_(m, 41)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    case = dict(x=R.make_x(8, 8, 8, 12, 42), record_len=[8], affine=R.make_affine([8], 8, 8, 12, 43),
                grad_out=np.random.RandomState(44).standard_normal((1, 8, 8, 12)).astype(np.float32))
    _, tx, tg = TR.restatement_grads(sd, args, case["x"], [8], case["affine"], case["grad_out"], torch.float64)
    _, yx, yg = TR.restatement_grads(sd, args, case["x"], [8], case["affine"], case["grad_out"], torch.float32)
    _, dx, grads = _step(m.to(DEV), case)
    _check("v2vnet training, 8 agents, d x", dx.cpu().numpy(), tx, yx)
    for k in sd:
        _check(f"v2vnet training, 8 agents, {k}", grads[k].cpu().numpy(), tg[k], yg[k])


def test_two_training_steps_are_bit_identical():
    """Output, d x and every parameter gradient: the kernels of this path have one writer per element and the weight gradients go through
    gencomm_conv2d_wgrad_fixed (partial sums added in a fixed order)."""
    c = TR.load_train_case("bt")
    m = _module(c["args"], c["sd"])
    _poison()
    out_a, dx_a, g_a = _step(m, c)
    _poison()
    out_b, dx_b, g_b = _step(m, c)
    assert torch.equal(out_a, out_b) and torch.equal(dx_a, dx_b)
    diff = [k for k in g_a if not torch.equal(g_a[k], g_b[k])]
    assert not diff, diff
    d = TR.load_train_case("d")                                  # ... and with every convolution on the wide routes
    md = _module(d["args"], d["sd"])
    (_, dx_a, g_a), (_, dx_b, g_b) = _step(md, d), _step(md, d)
    assert torch.equal(dx_a, dx_b) and not [k for k in g_a if not torch.equal(g_a[k], g_b[k])]


def test_frozen_parameters_and_frozen_input():
    c = TR.load_train_case("bt")
    m = _module(c["args"], c["sd"])
    _, dx, grads = _step(m, c)
    _, dx_none, grads_nox = _step(m, c, x_grad=False)            # the input does not require grad: the first round's warp adjoint is skipped
    assert dx_none is None and all(torch.equal(grads[k], grads_nox[k]) for k in grads)
    for p in m.parameters():
        p.requires_grad_(False)
    _, dx_frozen, grads_frozen = _step(m, c)
    assert all(g is None for g in grads_frozen.values()) and torch.equal(dx_frozen, dx)


def test_prepared_weights_are_rebuilt_after_an_optimizer_step():
    """Two SGD steps on the HIP path and on the restatement (float64: truth, float32: yardstick); the third forward's outputs compared."""
    c = TR.load_train_case("a")
    m = _module(c["args"], c["sd"])
    x, aff, go = torch.from_numpy(c["x"]), torch.from_numpy(c["affine"]), torch.from_numpy(c["grad_out"])
    lr = 0.05 * float(np.sqrt((c["sd"]["msg_cnn.weight"].numpy() ** 2).mean()) / np.sqrt((c["g64"]["msg_cnn.weight"] ** 2).mean()))
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    outs = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        out = m(x.to(DEV), c["record_len"], aff.to(DEV))
        outs.append(out.detach().cpu())
        out.backward(go.to(DEV))
        opt.step()
    with torch.no_grad():
        outs.append(m(x.to(DEV), c["record_len"], aff.to(DEV)).cpu())
    ref = {}
    for dt in (torch.float64, torch.float32):
        p = {k: v.clone().to(dt) for k, v in c["sd"].items()}
        for _ in range(2):
            _, _, g = TR.restatement_grads(p, c["args"], c["x"], c["record_len"], c["affine"], c["grad_out"], dt)
            p = {k: v - lr * torch.from_numpy(g[k]) for k, v in p.items()}
        with torch.no_grad():
            ref[dt] = R.v2vnet_forward(p, c["args"], x.to(dt), c["record_len"], aff).numpy()
    _check("v2vnet after two SGD steps", outs[2].numpy(), ref[torch.float64], ref[torch.float32])
    assert R.rel_rms(outs[2].numpy(), outs[0].numpy()) > 1e-3       # the steps moved the output: stale prepared weights would not
