"""Training MPDA's feature aligner on the GPU: the new kernels (gencomm_quad_attn_train_fwd / _bwd, gencomm_resize_bilinear_bwd,
gencomm_leaky_relu_fwd / _bwd) against float64, and the autograd Functions of gencomm_amd/mpda_bwd.py against the reference's stored
gradients (tests/golden/mpda_train_*.npz) and against the float64 restatement (tests/mpda_train_restatement.py).

Criterion (tests/test_gpu_cobevt_train.py's): truth = float64 on the CPU, yardstick = the same computation in float32 (for the fixture
cases: the reference's own float32 run, stored); the HIP result's relative rms error against the truth <= max(2 x the yardstick's,
1e-6), per tensor. Both numbers are printed.

Gradients that are mathematically zero have no relative error: the bias of every ``to_k`` Linear and of the LayerNorm in front of
it (either shifts all four keys of a group by the same vector, so every score of a query by q . shift: the softmax is invariant) and,
in ``train()`` mode, the bias of a convolution in front of a BatchNorm with batch statistics (the mean removes it). Their float64
"truth" is rounding noise around 1e-17, or exactly 0. Those tensors -- named in `zero_truth` below, nothing else -- are judged in
absolute terms against the scale of the same layer's weight gradient: rms(g) <= max(2 x the float32 yardstick's rms, 1e-6 x rms(the
weight's gradient)), which is the criterion above with the layer's [weight | bias] as the scale.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mpda_restatement as R
import mpda_train_restatement as TR
from gencomm_amd import _lib, synth
from gencomm_amd.runtime import ptr, stream_ptr
from test_mpda_train import package_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def npy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def rel(a, truth):
    a, truth = np.asarray(npy(a), np.float64), np.asarray(npy(truth), np.float64)
    return float(np.linalg.norm(a - truth) / np.linalg.norm(truth))


def check(what, got, truth, yard):
    """`yard`: the yardstick's own relative rms error (a number), or the float32 result it is computed from."""
    assert np.isfinite(npy(got)).all(), f"{what}: not finite"
    assert tuple(npy(got).shape) == tuple(npy(truth).shape), (what, npy(got).shape, npy(truth).shape)
    e = rel(got, truth)
    y = float(yard) if np.ndim(yard) == 0 and not torch.is_tensor(yard) else rel(yard, truth)
    print(f"{what}: relative rms against float64: HIP {e:.3e}, float32 yardstick {y:.3e}")
    assert e <= max(2.0 * y, 1e-6), (what, e, y)


def zero_truth(name, batch_stats):
    return name.endswith(("to_k.0.bias", "to_k.1.bias")) or (batch_stats and ".module." in name and name.endswith((".0.bias", ".3.bias")))


def check_zero(what, got, yard32, weight_truth):
    rms = lambda a: float(np.sqrt((np.asarray(npy(a), np.float64) ** 2).mean()))
    e, y, scale = rms(got), rms(yard32), rms(weight_truth)
    print(f"{what} (mathematically zero): rms HIP {e:.3e}, float32 yardstick {y:.3e}, the weight gradient's rms {scale:.3e}")
    assert np.isfinite(npy(got)).all() and e <= max(2.0 * y, 1e-6 * scale), (what, e, y, scale)


def poison():
    junk = torch.full((4 << 20,), float("nan"), device=DEV)   # NaNs in the memory the allocator hands out next
    del junk


# ---- the attention kernels ------------------------------------------------------------------------------------------------------------
PAD = 4   # channels in front of and behind the q / k / v blocks: non-zero channel offsets, q_ct > heads dim_head


def _quad_case(dh, grid, form, hw, heads=2, N=3, seed=0, keep_p=None):
    """Inputs of one kernel case. form: 'self' (one qkv tensor, bias), 'cross' (Nkv = N), 'bcast' (Nkv = 1).
    -> dict with the device tensors (q, kv tensors with PAD channels around the blocks), offsets, and the CPU float64 leaves."""
    H_, W_ = hw
    inner, G = heads * dh, (H_ // 2) * (W_ // 2)
    g = torch.Generator().manual_seed(1000 * dh + 10 * H_ + 2 * grid + {"self": 0, "cross": 1, "bcast": 2}[form] + seed)
    Nkv = 1 if form == "bcast" else N
    q, k, v = torch.randn(N, inner, H_, W_, generator=g), torch.randn(Nkv, inner, H_, W_, generator=g), torch.randn(Nkv, inner, H_, W_, generator=g)
    k = k * 1.5                                              # scores of a few units: a softmax that is not flat
    table = 0.5 * torch.randn(9, heads, generator=g) if form == "self" else None
    dout = torch.randn(N, inner, H_, W_, generator=g)
    keep = (torch.rand(N, heads, G, 16, generator=g) >= keep_p) if keep_p is not None else None
    return dict(q=q, k=k, v=v, table=table, dout=dout, keep=keep, ks=1.0 / (1.0 - keep_p) if keep_p is not None else 1.0, heads=heads, dh=dh,
                grid=grid, form=form, N=N, Nkv=Nkv, H=H_, W=W_, inner=inner)


def _quad_truth(c, dtype):
    """(out, dq, dk, dv, dtable or None) by torch autograd on the CPU in `dtype`."""
    q, k, v = (c[n].to(dtype).requires_grad_(True) for n in "qkv")
    t = c["table"].to(dtype).requires_grad_(True) if c["table"] is not None else None
    out = TR.quad_attention(q, k, v, t, R.rel_pos_indices(2), c["heads"], c["dh"], bool(c["grid"]), c["keep"], c["ks"])
    got = torch.autograd.grad((out * c["dout"].to(dtype)).sum(), [q, k, v] + ([t] if t is not None else []))
    return (out.detach(), *got, *([None] if t is None else []))


def _quad_device(c):
    """The device tensors in the kernel's argument form, PAD channels around the blocks: self -> one [N, 3 inner + 2 PAD] tensor."""
    inner = c["inner"]
    if c["form"] == "self":
        t = torch.randn(c["N"], 3 * inner + 2 * PAD, c["H"], c["W"])
        t[:, PAD:PAD + 3 * inner] = torch.cat([c["q"], c["k"], c["v"]], dim=1)
        t = t.to(DEV)
        return t, t, t, (PAD, PAD + inner, PAD + 2 * inner)
    qt = torch.randn(c["N"], inner + 2 * PAD, c["H"], c["W"])
    qt[:, PAD:PAD + inner] = c["q"]
    kv = torch.randn(c["Nkv"], 2 * inner + 2 * PAD, c["H"], c["W"])
    kv[:, PAD:PAD + 2 * inner] = torch.cat([c["k"], c["v"]], dim=1)
    kv = kv.to(DEV)
    return qt.to(DEV), kv, kv, (PAD, PAD, PAD + inner)


def _run_bwd(c, keep_words=None):
    """gencomm_quad_attn_bwd through the package's wrapper -> (dq, dk, dv, dtable) as CPU tensors of the blocks alone, plus the
    full output tensors (to see that nothing outside the blocks was written)."""
    from gencomm_amd.mpda import quad_attention_bwd
    qd, kd, vd, (qo, ko, vo) = _quad_device(c)
    poison()
    table = c["table"].to(DEV) if c["table"] is not None else None
    dq, dk, dv, dt = quad_attention_bwd(qd, kd, vd, table, c["dout"].to(DEV), c["heads"], c["dh"], c["grid"], qo, ko, vo, keep_words, c["ks"],
                                        self_form=c["form"] == "self")
    inner = c["inner"]
    blocks = (dq[:, qo:qo + inner].cpu(), dk[:, ko:ko + inner].cpu(), dv[:, vo:vo + inner].cpu(), None if dt is None else dt.cpu())
    return blocks, (dq, dk, dv)


@pytest.mark.parametrize("hw", [(4, 6), (12, 22)])
@pytest.mark.parametrize("form", ["self", "cross", "bcast"])
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_quad_attention_backward_kernel_vs_float64(dh, grid, form, hw):
    """4 x 6: 6 groups, one partial workgroup. 12 x 22: 66 groups, two workgroups (the last partial): the fixed-order dbias sum and the
    broadcast dk / dv sums cross workgroups. Blocks at channel offset 4 in tensors with 8 channels more than heads dim_head."""
    c = _quad_case(dh, grid, form, hw)
    t64, t32 = _quad_truth(c, torch.float64), _quad_truth(c, torch.float32)
    (dq, dk, dv, dt), full = _run_bwd(c)
    what = f"quad_attn_bwd dh {dh} {'grid' if grid else 'window'} {form} {hw}"
    for name, got, i in (("dq", dq, 1), ("dk", dk, 2), ("dv", dv, 3)):
        check(f"{what} {name}", got, t64[i], t32[i])
    if form == "self":
        check(f"{what} dbias", dt, t64[4], t32[4])
        assert tuple(dt.shape) == (9, c["heads"])
        pad = torch.cat([full[0][:, :PAD], full[0][:, -PAD:]], dim=1)
        assert not pad.any()                                  # the channels around the blocks were not written
    else:
        assert dt is None
        for t in full:
            assert not torch.cat([t[:, :PAD], t[:, -PAD:]], dim=1).any()
        assert tuple(dk.shape)[0] == c["Nkv"]


@pytest.mark.parametrize("form,grid,dh", [("self", 0, 32), ("self", 1, 16), ("bcast", 1, 32), ("cross", 0, 64)])
def test_attention_dropout_with_a_supplied_keep_mask(form, grid, dh):
    """p = 0.5: the forward and all four gradients against the float64 restatement under the SAME mask; keep = NULL, and an all-ones
    mask at scale 1, reproduce gencomm_quad_attn_fwd's bits."""
    from gencomm_amd.mpda import pack_keep, quad_attention, quad_attention_train
    c = _quad_case(dh, grid, form, (12, 22), keep_p=0.5)
    t64, t32 = _quad_truth(c, torch.float64), _quad_truth(c, torch.float32)
    words = pack_keep(c["keep"].to(DEV))
    qd, kd, vd, offs = _quad_device(c)
    table = c["table"].to(DEV) if c["table"] is not None else None
    what = f"quad attention dropout 0.5 dh {dh} {'grid' if grid else 'window'} {form}"
    out = quad_attention_train(qd, kd, vd, table, c["heads"], dh, grid, *offs, words, c["ks"])
    check(f"{what} out", out.cpu(), t64[0], t32[0])
    (dq, dk, dv, dt), _ = _run_bwd(c, words)
    for name, got, i in (("dq", dq, 1), ("dk", dk, 2), ("dv", dv, 3)):
        check(f"{what} {name}", got, t64[i], t32[i])
    if form == "self":
        check(f"{what} dbias", dt, t64[4], t32[4])
    dropped = 1.0 - float(c["keep"].float().mean())
    assert 0.45 < dropped < 0.55, dropped
    base = quad_attention(qd, kd, vd, table, c["heads"], dh, grid, *offs)
    assert not torch.equal(out, base)
    assert torch.equal(quad_attention_train(qd, kd, vd, table, c["heads"], dh, grid, *offs), base)
    ones = pack_keep(torch.ones_like(c["keep"]).to(DEV))
    assert torch.equal(quad_attention_train(qd, kd, vd, table, c["heads"], dh, grid, *offs, ones, 1.0), base)


@pytest.mark.parametrize("form,grid", [("self", 0), ("self", 1), ("bcast", 0), ("bcast", 1), ("cross", 1)])
def test_attention_backward_is_bit_identical_and_stays_inside_its_buffers(form, grid):
    """Two calls of the C entry write the same bits to dq, dk, dv and dbias; 1024 guard floats in front of and behind every output
    buffer (and the workspace) keep their sentinel."""
    c = _quad_case(32, grid, form, (12, 22), keep_p=0.5 if form == "self" else None)
    from gencomm_amd.mpda import pack_keep
    l, inner, hw, N, Nkv, heads = _lib.lib(), c["inner"], c["H"] * c["W"], c["N"], c["Nkv"], c["heads"]
    GUARD, SENT = 1024, -12345.0
    q, k, v, dout = (c[n].to(DEV).contiguous() for n in ("q", "k", "v", "dout"))
    table = c["table"].to(DEV) if c["table"] is not None else None
    words = pack_keep(c["keep"].to(DEV)) if c["keep"] is not None else None
    need = l.gencomm_quad_attn_bwd_workspace_bytes(N, Nkv, heads, 32, c["H"], c["W"], int(table is not None))
    assert (need > 0) == (form != "cross")                               # cross with a map per query map and no table: no workspace
    sizes = dict(dq=N * inner * hw, dk=Nkv * inner * hw, dv=Nkv * inner * hw, dbias=9 * heads, ws=need // 4)

    def run():
        bufs = {n: torch.full((s + 2 * GUARD,), SENT, device=DEV) for n, s in sizes.items()}
        p = {n: ptr(b) + 4 * GUARD for n, b in bufs.items()}
        if form == "self":       # dq | dk | dv as the channel blocks of one dqkv tensor
            bufs["dqkv"] = torch.full((3 * N * inner * hw + 2 * GUARD,), SENT, device=DEV)
            p["dq"] = ptr(bufs["dqkv"]) + 4 * GUARD
            p["dk"], p["dv"] = p["dq"] + 4 * inner * hw, p["dq"] + 8 * inner * hw
            qkv = torch.cat([q, k, v], dim=1).contiguous()
            src = (ptr(qkv), ptr(qkv) + 4 * inner * hw, ptr(qkv) + 8 * inner * hw, 3 * inner)
        else:
            qkv, src = None, (ptr(q), ptr(k), ptr(v), inner)
        _lib.check(l.gencomm_quad_attn_bwd(src[0], src[1], src[2], ptr(table), ptr(words), c["ks"], ptr(dout), p["dq"], p["dk"], p["dv"],
                                           p["dbias"] if table is not None else None, N, Nkv, heads, 32, c["H"], c["W"], src[3], src[3], grid,
                                           p["ws"], need, stream_ptr(torch.device(DEV))), "gencomm_quad_attn_bwd")
        torch.cuda.synchronize()
        del qkv
        return {n: b.cpu() for n, b in bufs.items()}

    a, b = run(), run()
    outs = ("dqkv", "dbias") if form == "self" else ("dq", "dk", "dv")
    for n in outs:
        body = a[n][GUARD:-GUARD]
        assert torch.equal(body, b[n][GUARD:-GUARD]), n                       # bit-identical
        assert not (body == SENT).any(), n                                    # every element written
    for n, t in a.items():
        assert (t[:GUARD] == SENT).all() and (t[-GUARD:] == SENT).all(), n    # guards untouched
    if form != "self":
        assert (a["dbias"] == SENT).all()                                     # no table: dbias is not written


# ---- the resize adjoint and the LeakyReLU -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [((6, 10), (4, 6)), ((4, 6), (7, 9)), ((5, 3), (5, 3)), ((2, 2), (9, 5)), ((1, 4), (4, 1))])
def test_resize_bilinear_backward_vs_float64(sizes):
    from gencomm_amd.mpda import resize_bilinear_bwd
    (hi, wi), (ho, wo) = sizes
    g = torch.Generator().manual_seed(hi * 100 + wo)
    dy = torch.randn(2, 3, ho, wo, generator=g)
    dy[0, 0, 0, 0] = -0.0

    def truth(dtype):
        x = torch.zeros(2, 3, hi, wi, dtype=dtype, requires_grad=True)
        return torch.autograd.grad(F.interpolate(x, size=[ho, wo], mode="bilinear", align_corners=False), x, dy.to(dtype))[0]

    poison()
    dx = resize_bilinear_bwd(dy.to(DEV), (hi, wi))
    check(f"resize_bilinear_bwd {sizes}", dx.cpu(), truth(torch.float64), truth(torch.float32))
    assert torch.equal(dx, resize_bilinear_bwd(dy.to(DEV), (hi, wi)))                       # two runs: the same bits
    if (hi, wi) == (ho, wo):
        assert torch.equal(dx.cpu().view(torch.int32), dy.view(torch.int32))              # the same size: dy, bit for bit (-0.0 included)


def test_leaky_relu_forward_and_backward_are_exact():
    from gencomm_amd.mpda import leaky_relu, leaky_relu_bwd
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 5, 7, 11, generator=g)                                   # 1155 values: no multiple of 64
    flat = x.view(-1)
    flat[:8] = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 3e38, -3e38])
    dy = torch.randn(3, 5, 7, 11, generator=g)
    for slope in (0.01, 0.0):
        want = F.leaky_relu(x, slope)
        y = leaky_relu(x.to(DEV), slope)
        assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32)), slope
        xr = x.clone().requires_grad_(True)
        want_dx, = torch.autograd.grad(F.leaky_relu(xr, slope), xr, dy)
        dx = leaky_relu_bwd(y, dy.to(DEV), slope)
        assert torch.equal(dx.cpu().view(torch.int32), want_dx.view(torch.int32)), slope


# ---- the modules ------------------------------------------------------------------------------------------------------------------------
def _dev_inputs(arrs):
    return [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in arrs]


def _golden_step(tag, m):
    """One step of the package's module on a golden case -> dict under the fixture's names (device tensors)."""
    c = TR.TRAIN_CASES[tag]
    t = _dev_inputs(TR.case_inputs(tag))
    fn = lambda shape: torch.from_numpy(TR.functional(tag, shape)).to(DEV)
    rec = {}
    poison()
    if c["kind"] == "resizer":
        out = m(t[0], t[1])
        out.backward(fn(out.shape))
        rec.update(out=out, d_cav=t[1].grad)
    elif c["kind"] == "cdt":
        out = m(t[0], t[1])
        out.backward(fn(out.shape))
        rec.update(out=out, d_ego=t[0].grad, d_cav=t[1].grad)
    elif c["kind"] == "da":
        out = m(t[0])
        out.backward(fn(out.shape))
        rec.update(out=out, d_x=t[0].grad)
    else:
        aligned, logits = m(t[0], c["record_len"])
        TR.align_loss(aligned, logits, fn(aligned.shape), c["record_len"]).backward()
        rec.update(aligned=aligned, logits=logits, d_x=t[0].grad)
    for k, p in m.named_parameters():
        rec["g:" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    if c["mode"] == "train":
        rec.update({"rs:" + k: b for k, b in m.named_buffers() if k.endswith(("running_mean", "running_var"))})
    return rec


@pytest.mark.parametrize("tag", list(TR.TRAIN_CASES))
def test_module_gradients_vs_reference_golden(tag):
    """Output, input gradients (collaborator and ego), every parameter gradient, and the BatchNorm running statistics after the
    train() step, against the reference's own float64 step; yardstick: the reference's float32 step."""
    c, rec = TR.TRAIN_CASES[tag], TR.load_golden(tag)
    m = package_module(tag).to(DEV)
    got = _golden_step(tag, m)
    names = TR.stored_names(rec)
    assert sorted(got) == names
    batch = c["mode"] == "train"
    for k in names:
        y32, y64, e_ref = TR.stored(rec, k)
        if tag == "rebuttal" and k.startswith(("g:resizer", "g:cdt")):  # the resizer and cdt are not run: exactly zero
            assert not np.abs(y64).max() > 0 and not npy(got[k]).any(), k
        elif zero_truth(k, batch):
            check_zero(f"mpda train case {tag} {k}", got[k], y32, TR.stored(rec, k[:-4] + "weight")[1])
        else:
            check(f"mpda train case {tag} {k}", got[k], y64, e_ref)
    if batch:
        assert all(int(b) == 1 for k, b in m.named_buffers() if k.endswith("num_batches_tracked"))
    if tag == "rebuttal":
        assert torch.equal(got["aligned"].cpu(), torch.from_numpy(TR.case_inputs(tag)[0]))


def test_reversal_factor():
    """The classifier-only loss: d aligned = -9.1 x the head's plain input gradient (the restatement with the reversal layer removed);
    the head's own parameter gradients carry no factor."""
    tag = "da"
    m = package_module(tag).to(DEV)
    x = _dev_inputs(TR.case_inputs(tag))[0]
    labels = TR.class_labels([3], TR.H, TR.W)
    F.binary_cross_entropy_with_logits(m(x), labels.to(DEV)).backward()

    def plain(dtype):
        sd = TR.leaf_sd(m, dtype)
        xc = torch.from_numpy(TR.case_inputs(tag)[0]).to(dtype).requires_grad_(True)
        loss = F.binary_cross_entropy_with_logits(TR.da_head(sd, "", xc, None), labels.to(dtype))
        gx, gw = torch.autograd.grad(loss, [xc, sd["conv1_da.weight"]])
        return gx, gw

    (x64, w64), (x32, w32) = plain(torch.float64), plain(torch.float32)
    check("DAImgHead d x against -9.1 x the plain gradient", x.grad, -9.1 * x64, -9.1 * x32)
    check("DAImgHead d conv1_da.weight (unscaled)", m.conv1_da.weight.grad, w64, w32)


SHIPPED = {"resizer": {"input_channel": 256, "output_channel": 256,
                       "wg_att": {"input_dim": 256, "mlp_dim": 256, "window_size": 2, "dim_head": 32, "drop_out": 0.1, "depth": 1},
                       "residual": {"input_dim": 256, "depth": 2}},
           "cdt": {"input_dim": 256, "window_size": 2, "dim_head": 32, "heads": 16, "depth": 1}, "classifier": 256}


def _restated_step(m, args, x, record_len, g, dtype, batch_stats=False, masks=None):
    """One aligner step on the restatement -> dict as _golden_step's (CPU tensors)."""
    sd = TR.leaf_sd(m, dtype)
    xc = torch.from_numpy(x).to(dtype).requires_grad_(True)
    it = iter([t.cpu() for t in masks]) if masks is not None else None
    aligned, logits = TR.mpda_align(sd, args, xc, record_len, batch_stats, it)
    gi, gp = TR.grads_of(TR.align_loss(aligned, logits, torch.from_numpy(g).to(dtype), record_len), sd, {"x": xc})
    rec = dict(aligned=aligned.detach(), logits=logits.detach(), d_x=gi["x"])
    rec.update({"g:" + k: v for k, v in gp.items()})
    if batch_stats:
        rec.update({"rs:" + k: v for k, v in sd.items() if k.endswith(("running_mean", "running_var"))})
    return rec


def _module_step(m, x, record_len, g):
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    poison()
    aligned, logits = m(xd, record_len)
    TR.align_loss(aligned, logits, torch.from_numpy(g).to(DEV), record_len).backward()
    rec = dict(aligned=aligned.detach(), logits=logits.detach(), d_x=xd.grad)
    rec.update({"g:" + k: p.grad for k, p in m.named_parameters()})
    return rec


def _check_step(what, got, t64, t32, batch_stats=False):
    for k in t64:
        if zero_truth(k, batch_stats):
            check_zero(f"{what} {k}", got[k], t32[k], t64[k[:-4] + "weight"])
        else:
            check(f"{what} {k}", got[k], t64[k], t32[k])


def test_module_gradients_vs_restatement_at_the_shipped_widths():
    """m1m2_att.yaml's widths (resizer 256 channels, dim_head 32; cdt 16 heads x 32) on an 8 x 12 map, one ego and 2 collaborators."""
    from gencomm_amd import MPDAAlign
    m = MPDAAlign(SHIPPED, trainable=True).eval()
    synth.fill_params_(m, 4711)
    synth.fill_bn_stats_(m, 4761)
    rng = np.random.RandomState(4712)
    x, g = rng.standard_normal((3, 256, 8, 12)).astype(np.float32), rng.standard_normal((3, 256, 8, 12)).astype(np.float32)
    t64, t32 = (_restated_step(m, SHIPPED, x, [3], g, dt) for dt in (torch.float64, torch.float32))
    got = _module_step(m.to(DEV), x, [3], g)
    assert sorted(got) == sorted(t64)
    _check_step("mpda train, shipped widths", got, t64, t32)


def _draw_masks(n, Cc, mlp, heads, hw_list, p):
    """The documented order, per SwapFusionEncoder call (hw_list: its map per call), window then grid."""
    masks = []
    for (h, w) in hw_list:
        for _ in range(2):
            masks.append(torch.rand(n, heads, (h // 2) * (w // 2), 16, device=DEV) >= p)
            for ch in (Cc, mlp, Cc):
                masks.append((torch.rand_like(torch.empty(n, ch, h, w, device=DEV)) >= p).float() / (1.0 - p))
    return masks


def test_dropout_and_batch_statistics_in_the_module():
    """train() mode, drop_out 0.1, BatchNorm batch statistics live (3 x 4 x 6 = 72 values per channel): the test re-seeds, draws the
    masks itself in the documented order and replays them through the float64 restatement."""
    from gencomm_amd import LearnableResizer
    tag = "resizer_eval"
    args = TR.case_args(tag)["resizer"]
    assert args["wg_att"]["drop_out"] == 0.1
    ego, cav = TR.case_inputs(tag)
    g = TR.functional(tag, (3, TR.C, TR.H, TR.W))

    def fresh():
        m = LearnableResizer(args, trainable=True)
        synth.fill_params_(m, 99)
        synth.fill_bn_stats_(m, 149)
        return m.train()

    def step(m):
        e, c = torch.from_numpy(ego).to(DEV), torch.from_numpy(cav).to(DEV).requires_grad_(True)
        out = m(e, c)
        out.backward(torch.from_numpy(g).to(DEV))
        rec = dict(out=out.detach(), d_cav=c.grad)
        rec.update({"g:" + k: p.grad for k, p in m.named_parameters()})
        rec.update({"rs:" + k: b.clone() for k, b in m.named_buffers() if k.endswith(("running_mean", "running_var"))})
        return rec

    def restated(dtype, masks):
        m = fresh()
        sd = TR.leaf_sd(m, dtype)
        c = torch.from_numpy(cav).to(dtype).requires_grad_(True)
        out = TR.resizer(sd, "", torch.from_numpy(ego).to(dtype), c, TR.DIM_HEAD, 2, True, iter([t.cpu() for t in masks]), 0.1)
        gi, gp = TR.grads_of((out * torch.from_numpy(g).to(dtype)).sum(), sd, {"cav": c})
        rec = dict(out=out.detach(), d_cav=gi["cav"])
        rec.update({"g:" + k: v for k, v in gp.items()})
        rec.update({"rs:" + k: v for k, v in sd.items() if k.endswith(("running_mean", "running_var"))})
        return rec

    torch.manual_seed(1234)
    got = step(fresh().to(DEV))
    again = step(fresh().to(DEV))                                  # the generator moved on: other masks
    assert not torch.equal(got["out"], again["out"])
    torch.manual_seed(1234)
    masks = _draw_masks(3, TR.C, TR.MLP_DIM, TR.C // TR.DIM_HEAD, [(TR.H, TR.W)] * 2, 0.1)
    assert len(masks) == 16
    dropped = float(torch.stack([1.0 - (t != 0).float().mean() for t in masks]).mean())
    assert 0.07 < dropped < 0.13, dropped
    t64, t32 = restated(torch.float64, masks), restated(torch.float32, masks)
    assert sorted(got) == sorted(t64)
    _check_step("mpda resizer train() with dropout 0.1 and batch statistics", got, t64, t32, batch_stats=True)
    with torch.no_grad():                                           # train() mode draws masks without gradients too
        torch.manual_seed(1234)
        y = fresh().to(DEV)(torch.from_numpy(ego).to(DEV), torch.from_numpy(cav).to(DEV))
    assert torch.equal(y, got["out"])


def test_stage2_pattern_frozen_parameters_still_pass_the_input_gradient(monkeypatch):
    """Every parameter frozen, the input trainable: dx equals the full run's, every parameter gradient is None and no weight-gradient
    entry is called."""
    from gencomm_amd import train_ops as T
    tag = "align"
    m = package_module(tag).to(DEV)
    x, rl = TR.case_inputs(tag)[0], TR.TRAIN_CASES[tag]["record_len"]
    g = TR.functional(tag, x.shape)
    calls = {"n": 0}
    for name in ("conv2d_wgrad", "conv2d_wgrad_fixed"):
        orig = getattr(T, name)

        def counted(*a, _orig=orig, **kw):
            calls["n"] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(T, name, counted)
    full = _module_step(m, x, rl, g)
    assert calls["n"] > 20 and all(v is not None for k, v in full.items() if k.startswith("g:"))
    for p in m.parameters():
        p.requires_grad_(False)
    calls["n"] = 0
    frozen = _module_step(m, x, rl, g)
    assert calls["n"] == 0
    assert all(v is None for k, v in frozen.items() if k.startswith("g:"))
    assert torch.equal(frozen["aligned"], full["aligned"]) and torch.equal(frozen["logits"], full["logits"])
    assert torch.equal(frozen["d_x"], full["d_x"])
    rec = TR.load_golden(tag)
    check("mpda train, every parameter frozen: dx", frozen["d_x"], TR.stored(rec, "d_x")[1], TR.stored(rec, "d_x")[2])


def test_inference_path_bits():
    """A trainable module under no_grad in eval() equals the default module's output bit for bit on the c32 fixture case; so does the
    forward inside a grad-enabled eval() call."""
    from gencomm_amd import CrossDomainFusionEncoder, DAImgHead, LearnableResizer, MPDAAlign
    c = R.CASES["c32"]
    args = R.case_args(c)
    s_res, s_cdt, s_da, s_al = R.case_seeds("c32")
    ego, cav, cdt_cav, x = (torch.from_numpy(a).to(DEV) for a in R.case_inputs("c32"))

    def pair(make, seed):
        out = []
        for t in (False, True):
            m = make(t).eval()
            synth.fill_params_(m, seed)
            synth.fill_bn_stats_(m, seed + 50)
            out.append(m.to(DEV))
        return out

    cases = ((pair(lambda t: LearnableResizer(args["resizer"], trainable=t), s_res), lambda m, r: m(ego, cav.clone().requires_grad_(r))),
             (pair(lambda t: CrossDomainFusionEncoder(args["cdt"], trainable=t), s_cdt), lambda m, r: m(ego, cdt_cav.clone().requires_grad_(r))),
             (pair(lambda t: DAImgHead(c["C"], trainable=t), s_da), lambda m, r: m(cdt_cav.clone().requires_grad_(r))),
             (pair(lambda t: MPDAAlign(args, trainable=t), s_al), lambda m, r: m(x.clone().requires_grad_(r), c["record_len"])))
    for (default, trainable), call in cases:
        with torch.no_grad():
            want, got = call(default, False), call(trainable, False)
        tup = lambda y: y if isinstance(y, tuple) else (y,)
        for a, b in zip(tup(want), tup(got)):
            assert torch.equal(a, b), type(default).__name__
        live = call(trainable, True)                                  # gradients enabled: the training forward
        for a, b in zip(tup(want), tup(live)):
            assert b.requires_grad and torch.equal(a, b.detach()), type(default).__name__


def test_second_backward_raises():
    """The tape is released after the first backward: a second one through the same forward names itself."""
    m = package_module("resizer_eval").to(DEV)
    ego, cav = _dev_inputs(TR.case_inputs("resizer_eval"))
    out = m(ego, cav)
    g = torch.ones_like(out)
    out.backward(g, retain_graph=True)
    with pytest.raises(RuntimeError, match="backward through the same forward twice"):
        out.backward(g, retain_graph=True)
    m2 = package_module("cdt").to(DEV)
    ego, cav = _dev_inputs(TR.case_inputs("cdt"))
    out = m2(ego, cav)
    out.backward(torch.ones_like(out), retain_graph=True)
    with pytest.raises(RuntimeError, match="CrossDomainFunction: backward through the same forward twice"):
        out.backward(torch.ones_like(out))


def test_ego_only_scene_skips_the_discarded_branch_in_train_mode():
    """The stated difference: the reference runs resizer + cdt on an ego-only scene and discards the result, which in
    train() mode still moves the resizer's BatchNorm running statistics; here the discarded work is skipped, so an ego-only scene
    leaves them alone: after a step over scenes [1, 3] every BatchNorm has counted ONE batch (the reference: two), after [1, 1] none.
    The gradient is the same either way: the ego passes through, and the classifier sees it."""
    m = package_module("align").to(DEV).train()
    x = torch.from_numpy(TR.case_inputs("align")[0]).to(DEV)
    before = {k: b.clone() for k, b in m.named_buffers()}
    xs = x[:2].clone().requires_grad_(True)
    aligned, logits = m(xs, [1, 1])
    (aligned.sum() + logits.sum()).backward()
    assert torch.equal(aligned, xs.detach()) and xs.grad is not None
    assert all(torch.equal(b, before[k]) for k, b in m.named_buffers())
    xs = x[:4].clone().requires_grad_(True)
    aligned, logits = m(xs, [1, 3])
    (aligned.sum() + logits.sum()).backward()
    counts = {k: int(b) for k, b in m.named_buffers() if k.endswith("num_batches_tracked")}
    assert len(counts) == 4 and set(counts.values()) == {1}, counts
    assert all(not torch.equal(b, before[k]) for k, b in m.named_buffers() if k.endswith("running_mean"))
    assert torch.equal(aligned[0], xs.detach()[0])
