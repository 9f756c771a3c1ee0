"""Training-mode BatchNorm on the four HIP paths against float64 torch (tests/bn_reference.py for the truth and the bounds):

  bn2d    composed 2-D entries (gencomm_bn2d_train_fwd / _bwd through train_ops.bn2d_train_fwd / _bwd)
  convbn  fused Conv2d + BatchNorm2d + ReLU (bev_backbone.conv2d_hip in train mode: _ConvBnTrainFn)
  pfn     Linear + BatchNorm1d + ReLU + slot max (point_pillar._PillarNetFusedFn; pfn_composed: _PillarNetFn)
  rows    BatchNorm1d over the active rows of a sparse layer (second.sparse_conv_bn_relu with a 1x1x1 SubMConv3d: a row GEMM)

Outputs, every gradient, the running statistics and the batch counter after several steps; momentum 0.01 / 0.1 / 1 / None; no running
statistics; a counter on the CPU; gradient accumulation; eval mode; the single-value error; and the paths against each other."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from bn_reference import C_GRAD, C_OUT, Report, Triple

pytestmark = pytest.mark.gpu


# ---- the paths --------------------------------------------------------------------------------------------------------------------
class _Bn2dComposed(torch.autograd.Function):
    """train_ops.bn2d_train_fwd / _bwd as an autograd function; misalign: x (and dy) are handed over 4 bytes into their storage."""

    @staticmethod
    def forward(ctx, x, bn, relu, misalign, gamma, beta):
        from gencomm_amd import train_ops as T
        if misalign:
            x = _shifted(x)
        y, save = T.bn2d_train_fwd(x, bn, relu)
        ctx.bn, ctx.relu, ctx.misalign = bn, relu, misalign
        ctx.save_for_backward(x, y, save)
        return y

    @staticmethod
    def backward(ctx, gy):
        from gencomm_amd import train_ops as T
        x, y, save = ctx.saved_tensors
        gy = _shifted(gy) if ctx.misalign else gy.contiguous()
        dx, dg, db = T.bn2d_train_bwd(x, y, gy, save, ctx.bn.weight, ctx.relu)
        return dx, None, None, None, dg, db


def _shifted(t):
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class Bn2d(nn.Module):
    def __init__(self, C, eps=1e-3, momentum=0.1, relu=True, track=True, misalign=False):
        super().__init__()
        self.bn = nn.BatchNorm2d(C, eps=eps, momentum=momentum, track_running_stats=track)
        self.relu, self.misalign = relu, misalign

    def ref(self, x):
        y = self.bn(x)
        return F.relu(y) if self.relu else y

    def hip(self, x):
        return _Bn2dComposed.apply(x, self.bn, self.relu, self.misalign, self.bn.weight, self.bn.bias)


class ConvBn(nn.Module):
    def __init__(self, cin, cout, k=3, stride=1, bias=False, eps=1e-3, momentum=0.1, track=True):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=bias)
        self.bn = nn.BatchNorm2d(cout, eps=eps, momentum=momentum, track_running_stats=track)

    def ref(self, x):
        return F.relu(self.bn(self.conv(x)))

    def hip(self, x):
        from gencomm_amd.bev_backbone import conv2d_hip
        return conv2d_hip(x, self.conv, self.bn, relu=True)


class Pfn(nn.Module):
    def __init__(self, F_, C, eps=1e-3, momentum=0.1, track=True, fused=True):
        super().__init__()
        self.linear = nn.Linear(F_, C, bias=False)
        self.norm = nn.BatchNorm1d(C, eps=eps, momentum=momentum, track_running_stats=track)
        self.fused = fused

    def ref(self, feats):   # pillar_vfe.py:31-54: the padded (zero) slots are part of the batch statistics
        x = self.norm(self.linear(feats).permute(0, 2, 1)).permute(0, 2, 1)
        return torch.max(F.relu(x), dim=1)[0]

    def hip(self, feats):
        from gencomm_amd.point_pillar import _PillarNetFn, _PillarNetFusedFn
        from gencomm_amd.train_ops import bn_batch_statistics
        M, P, F_ = feats.shape
        if self.fused and bn_batch_statistics(self.norm):   # the gate of PointPillar._encode_train
            return _PillarNetFusedFn.apply(feats.contiguous(), self, self.linear.weight, self.norm.weight, self.norm.bias)
        x4 = feats.permute(2, 0, 1).reshape(1, F_, 1, M * P).contiguous()
        return _PillarNetFn.apply(x4, self, M, P, self.linear.weight, self.norm.weight, self.norm.bias)


class Rows(nn.Module):
    def __init__(self, cin, C, eps=1e-3, momentum=0.1, track=True):
        super().__init__()
        from gencomm_amd.second import SubMConv3d
        self.conv = SubMConv3d(cin, C, 1)
        self.bn = nn.BatchNorm1d(C, eps=eps, momentum=momentum, track_running_stats=track)
        if C > 64:   # the sparse weight / input gradients cover at most 64 channels (VoxelBackBone8x): BatchNorm's own gradients only
            self.conv.weight.requires_grad_(False)

    def ref(self, feat):
        return F.relu(self.bn(feat @ self.conv.weight.reshape(self.conv.out_channels, -1).t()))

    def hip(self, feat):
        from gencomm_amd.second import SparseTensor, sparse_conv_bn_relu
        n = feat.shape[0]
        keys = torch.arange(n, dtype=torch.int64, device=feat.device)
        return sparse_conv_bn_relu(SparseTensor(keys, feat, 1, [1, 64, max(1, (n + 63) // 64)]), self.conv, self.bn, True).features


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64).float()


def _pillars(g, M, P, F_):
    feats = _randn(g, M, P, F_) * 2.0 + 0.5
    npts = torch.randint(1, P + 1, (M,), generator=g)
    npts[0] = P if M > 1 else npts[0]
    return feats * (torch.arange(P).view(1, P) < npts.view(M, 1)).unsqueeze(-1).float()


def _affine(m, g, gamma_sign=1.0, beta_shift=0.0):
    for mod in m.modules():
        if isinstance(mod, nn.modules.batchnorm._BatchNorm) and mod.weight is not None:
            with torch.no_grad():
                C = mod.weight.shape[0]
                mod.weight.copy_(gamma_sign * (0.5 + torch.rand(C, generator=g, dtype=torch.float64).float()))
                mod.bias.copy_(0.3 * _randn(g, C) + beta_shift)
        elif isinstance(mod, (nn.Conv2d, nn.Linear)) or type(mod).__name__ == "SubMConv3d":
            with torch.no_grad():
                mod.weight.copy_(_randn(g, *mod.weight.shape) / math.sqrt(mod.weight[0].numel()))
                if getattr(mod, "bias", None) is not None:
                    mod.bias.copy_(0.1 * _randn(g, *mod.bias.shape))
    return m


def _make(path, seed=0, gamma_sign=1.0, beta_shift=0.0, **kw):
    """(module, batch(seed) -> (inputs, w), grad_inputs) for one path."""
    g = torch.Generator().manual_seed(seed)
    if path == "bn2d":
        n, C, H, W = kw.pop("shape", (2, 16, 12, 20))
        data = kw.pop("data", "randn")
        m = Bn2d(C, **kw)

        def batch(s):
            gg = torch.Generator().manual_seed(1000 + s)
            x = _randn(gg, n, C, H, W)
            if data == "offset":
                x = (1e3 + 1e-2 * _randn(gg, n, C, H, W).double()).float()
            elif data == "const":
                x[:, 0] = 0.75
            else:
                x = x * 1.5 + 0.25
            return [x], _randn(gg, n, C, H, W)
        gi = (0,)
    elif path == "convbn":
        n, cin, H, W = kw.pop("shape", (2, 13, 18, 22))
        cout, k, stride, bias = kw.pop("cout", 24), kw.pop("k", 3), kw.pop("stride", 1), kw.pop("bias", False)
        m = ConvBn(cin, cout, k, stride, bias, **kw)
        Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1

        def batch(s):
            gg = torch.Generator().manual_seed(2000 + s)
            return [_randn(gg, n, cin, H, W)], _randn(gg, n, cout, Ho, Wo)
        gi = (0,)
    elif path in ("pfn", "pfn_composed"):
        M, P, F_, C = kw.pop("shape", (300, 16, 10, 64))
        m = Pfn(F_, C, fused=path == "pfn", **kw)

        def batch(s):
            gg = torch.Generator().manual_seed(3000 + s)
            return [_pillars(gg, M, P, F_)], _randn(gg, M, C)
        gi = ()
    elif path == "rows":
        n, cin, C = kw.pop("shape", (700, 16, 32))
        m = Rows(cin, C, **kw)

        def batch(s):
            gg = torch.Generator().manual_seed(4000 + s)
            return [_randn(gg, n, cin) * 1.3 - 0.2], _randn(gg, n, C)
        gi = (0,) if C <= 64 else ()
    else:
        raise ValueError(path)
    return _affine(m, g, gamma_sign, beta_shift), batch, gi


def _triple(m):
    return Triple(m, type(m).ref, type(m).hip).train()


def _run(title, path, steps=3, check_every_step=True, **kw):
    m, batch, gi = _make(path, **kw)
    t = _triple(m)
    rep = Report(title)
    for s in range(steps):
        inputs, w = batch(s)
        res = t.step(inputs, w, gi)
        if check_every_step or s == 0:
            t.check_step(rep, res, f"step {s} ")
    t.check_buffers(rep)
    rep.show()
    return t, rep


# ---- 1. shapes and variants ---------------------------------------------------------------------------------------------------
BN2D_SHAPES = {
    "v4": dict(shape=(2, 64, 16, 24)),
    "v1_hw_odd": dict(shape=(2, 3, 15, 17)),
    "v1_misaligned": dict(shape=(2, 64, 16, 24), misalign=True),
    "chunks64_v4": dict(shape=(2, 64, 200, 704), steps=1),
    "chunks64_v1": dict(shape=(3, 8, 199, 703), steps=2),
    "tiny_nhw2": dict(shape=(1, 3, 1, 2)),
    "tiny_nhw3": dict(shape=(3, 4, 1, 1)),
    "c1": dict(shape=(4, 1, 8, 8)),
    "c256": dict(shape=(2, 256, 8, 12)),
    "no_relu": dict(shape=(2, 32, 7, 9), relu=False),
}


@pytest.mark.parametrize("case", list(BN2D_SHAPES))
def test_bn2d_composed_shapes(case):
    kw = dict(BN2D_SHAPES[case])
    _run(f"bn2d[{case}]", "bn2d", **kw)


CONV_CASES = {
    "k3s1": dict(cout=24),
    "k3s1_bias": dict(cout=24, bias=True),
    "k1s1_bias": dict(k=1, cout=40, bias=True),
    "k3s2": dict(stride=2, cout=72),
    "k1s2_bias": dict(k=1, stride=2, cout=20, bias=True),
    "k3s1_hw4": dict(shape=(2, 40, 16, 20), cout=48, bias=True),
    "k3s1_odd_cin3": dict(shape=(3, 3, 9, 13), cout=64),
}


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_convbn_fused_vs_float64(case):
    _run(f"convbn[{case}]", "convbn", **CONV_CASES[case])


PFN_CASES = {
    "f9_c32": dict(shape=(257, 16, 9, 32)),
    "f10_c64": dict(shape=(300, 32, 10, 64)),
    "f11_c64": dict(shape=(123, 20, 11, 64)),
    "m1": dict(shape=(1, 32, 10, 64)),
    "m40000": dict(shape=(40000, 6, 10, 64), steps=1),
}


@pytest.mark.parametrize("path", ["pfn", "pfn_composed"])
@pytest.mark.parametrize("case", list(PFN_CASES))
def test_pfn_vs_float64(path, case):
    _run(f"{path}[{case}]", path, **PFN_CASES[case])


@pytest.mark.parametrize("C", [16, 32, 64, 128])
@pytest.mark.parametrize("n", [2, 3, 5000])
def test_rows_vs_float64(C, n):
    _run(f"rows[C{C} n{n}]", "rows", shape=(n, 16, C))


# ---- 2. data edges ------------------------------------------------------------------------------------------------------------
EDGES = {
    "constant_channel": dict(data="const"),
    "offset_1e3": dict(data="offset"),
    "negative_gamma": dict(gamma_sign=-1.0),
    "beta_very_negative": dict(beta_shift=-2.5),
    "eps_1e-5": dict(eps=1e-5),
}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("shape", [(2, 8, 16, 24), (2, 8, 15, 17)], ids=["v4", "v1"])
def test_bn2d_data_edges(edge, shape):
    _run(f"bn2d[{edge} {shape}]", "bn2d", shape=shape, **EDGES[edge])


@pytest.mark.parametrize("path", ["convbn", "pfn", "rows"])
@pytest.mark.parametrize("edge", ["negative_gamma", "beta_very_negative", "eps_1e-5"])
def test_data_edges_other_paths(path, edge):
    _run(f"{path}[{edge}]", path, **EDGES[edge])


def test_rows_constant_channel_and_offset():
    """The row statistics under a constant channel (variance 0: rstd = 1 / sqrt(eps)) and a large common offset."""
    from gencomm_amd.second import SparseTensor, sparse_conv_bn_relu
    for name, fill in (("constant", lambda x: x.fill_(0.75)), ("offset", lambda x: x.copy_(1e3 + 1e-2 * torch.randn_like(x)))):
        g = torch.Generator().manual_seed(7)
        bn = nn.BatchNorm1d(16, eps=1e-3, momentum=1.0)
        x = _randn(g, 900, 16)
        fill(x[:, :4])
        ref = F.batch_norm(x.double(), None, None, bn.weight.double(), bn.bias.double(), True, 0.0, bn.eps)
        # the same statistics through the row kernels: an identity 1x1x1 convolution in front
        from gencomm_amd.second import SubMConv3d
        conv = SubMConv3d(16, 16, 1).cuda()
        with torch.no_grad():
            conv.weight.copy_(torch.eye(16).view(16, 1, 1, 1, 16))
        bnh = bn.cuda()
        with torch.no_grad():
            st = SparseTensor(torch.arange(900, device="cuda"), x.cuda(), 1, [1, 64, 15])
            y = sparse_conv_bn_relu(st, conv, bnh, False).features
        err = float((y.cpu().double() - ref).abs().max())
        f32 = float((F.batch_norm(x, None, None, bn.weight.detach().cpu(), bn.bias.detach().cpu(), True, 0.0, bn.eps).double() - ref).abs().max())
        bound = max(4 * f32, C_OUT * float(ref.abs().max()))
        print(f"rows[{name}] out: max err {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (name, err, bound)
        rv = x[:, :4].double().var(0, unbiased=True)
        assert torch.allclose(bnh.running_var[:4].cpu().double(), rv, rtol=1e-6, atol=1e-12), (bnh.running_var[:4], rv)


# ---- 3. running statistics ----------------------------------------------------------------------------------------------------
STAT_PATHS = ["bn2d", "convbn", "pfn", "pfn_composed", "rows"]


@pytest.mark.parametrize("path", STAT_PATHS)
@pytest.mark.parametrize("momentum", [0.01, 0.1, 1.0, None], ids=["m0.01", "m0.1", "m1", "cumulative"])
def test_running_statistics(path, momentum):
    """running_mean / running_var after 3 batches (momentum 1: the UNBIASED variance of the last batch; None: the cumulative average) and
    num_batches_tracked == 3 exactly."""
    t, _ = _run(f"{path}[momentum {momentum}]", path, momentum=momentum, check_every_step=False)
    nbt = [b for k, b in t.mh.named_buffers() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 1 and int(nbt[0]) == 3, nbt


@pytest.mark.parametrize("path", STAT_PATHS)
def test_no_running_statistics(path):
    """track_running_stats=False: the buffers stay None, outputs and gradients use the batch statistics."""
    t, _ = _run(f"{path}[track_running_stats=False]", path, track=False, steps=2)
    for m in t.mh.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            assert m.running_mean is None and m.running_var is None and m.num_batches_tracked is None


@pytest.mark.parametrize("path", ["bn2d", "convbn", "pfn", "rows"])
def test_counter_on_the_cpu(path):
    """A num_batches_tracked that lives on the CPU (it takes conv + BN off the fused gate): still counted, and nothing writes through it
    from the device."""
    m, batch, gi = _make(path, momentum=0.1)
    t = _triple(m)
    for mod in t.mh.modules():
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            mod.num_batches_tracked = mod.num_batches_tracked.cpu()
    rep = Report(f"{path}[counter on the CPU]")
    for s in range(3):
        t.check_step(rep, t.step(*batch(s), gi), f"step {s} ")
    t.check_buffers(rep)
    rep.show()


# ---- 4. semantics -------------------------------------------------------------------------------------------------------------
GRAD_PATHS = ["bn2d", "convbn", "pfn", "pfn_composed", "rows"]


def _grads(t):
    return {k: p.grad.detach().cpu().double().clone() for k, p in t.mh.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("path", GRAD_PATHS)
def test_gradients_accumulate(path):
    """Two backward passes without zero_grad give the sum of the single passes; so does one pass onto a non-zero .grad (the kernels'
    write-vs-accumulate bit and the zero-pool blobs sit under this)."""
    m, batch, gi = _make(path, momentum=0.1)
    t = _triple(m)
    inputs, w = batch(0)
    t.step(inputs, w, gi)
    single = _grads(t)
    assert single
    t.step(inputs, w, gi, zero_grad=False)
    twice = _grads(t)
    g = torch.Generator().manual_seed(11)
    for k, p in t.mh.named_parameters():
        if p.grad is not None:
            p.grad = _randn(g, *p.shape).to(p.device)
    pre = _grads(t)
    for mod in (t.m64, t.m32):
        mod.zero_grad(set_to_none=True)
    t.step(inputs, w, gi, zero_grad=False)
    onto = _grads(t)
    for k in single:
        scale = float(single[k].abs().max()) + 1e-30
        # batch statistics move between the passes only through the running buffers, which the outputs do not read: same gradients
        assert float((twice[k] - 2 * single[k]).abs().max()) <= 1e-6 * scale, (k, "two passes")
        assert float((onto[k] - (pre[k] + single[k])).abs().max()) <= 1e-6 * (scale + float(pre[k].abs().max())), (k, "onto a non-zero .grad")
    print(f"{path}: gradient accumulation ok over {sorted(single)}")


@pytest.mark.parametrize("path", GRAD_PATHS)
def test_five_steps_with_other_pool_users_between(path):
    """Five training steps on five batches, other users of the zero pool and of the BatchNorm scratch between them: every step sees only
    its own batch (stale scratch would show as an error against float64)."""
    from gencomm_amd import train_ops as T
    from gencomm_amd.runtime import zeros as pool_zeros
    m, batch, gi = _make(path, momentum=0.1)
    t = _triple(m)
    rep = Report(f"{path}[five steps]")
    other = nn.BatchNorm2d(48).cuda().train()
    for s in range(5):
        t.check_step(rep, t.step(*batch(s), gi), f"step {s} ")
        junk = pool_zeros(4096, torch.float64, torch.device("cuda"))
        junk.fill_(123.0)
        xo = torch.randn(2, 48, 11, 12, device="cuda") * 5 + 3
        yo, so = T.bn2d_train_fwd(xo, other, True)
        T.bn2d_train_bwd(xo, yo, torch.randn_like(yo), so, other.weight, True)
    t.check_buffers(rep)
    rep.show()


@pytest.mark.parametrize("path", ["convbn", "pfn_composed", "rows"])   # bn2d: the raw entries are batch statistics by contract
def test_eval_mode_with_gradients(path):
    """Eval mode with requires_grad: the running statistics normalise, and the backward has no statistic terms."""
    m, batch, gi = _make(path, momentum=0.3)
    t = _triple(m)
    t.step(*batch(0), gi)         # move the running statistics away from (0, 1)
    t.train(False)
    rep = Report(f"{path}[eval with gradients]")
    t.check_step(rep, t.step(*batch(1), gi), "")
    t.check_buffers(rep)
    rep.show()


@pytest.mark.parametrize("path", GRAD_PATHS)
def test_eval_mode_without_running_statistics(path):
    """Eval mode with track_running_stats=False: torch normalises with the batch statistics (bn_training = training or running_mean is
    None); so must every HIP path, with and without gradients."""
    m, batch, gi = _make(path, track=False)
    t = _triple(m).train(False)
    rep = Report(f"{path}[eval, no running statistics]")
    for s in range(2):
        t.check_step(rep, t.step(*batch(s), gi), f"step {s} ")
    inputs, _ = batch(2)
    with torch.no_grad():
        for p in t.mh.parameters():
            p.requires_grad_(False)
        got = type(t.mh).hip(t.mh, inputs[0].cuda())
        want = type(t.m64).ref(t.m64, inputs[0].double())
        f32 = type(t.m32).ref(t.m32, inputs[0])
    rep.check("no_grad out", got, want, f32, C_OUT)
    rep.show()


@pytest.mark.parametrize("path", ["bn2d", "convbn", "rows"])
def test_single_value_per_channel_raises(path):
    """One value per channel: the same ValueError torch raises (n H W = 1 for 2-D, a single active site for the rows)."""
    shape = {"bn2d": dict(shape=(1, 8, 1, 1)), "convbn": dict(shape=(1, 5, 1, 1), k=1), "rows": dict(shape=(1, 16, 32))}[path]
    m, batch, gi = _make(path, **shape)
    t = _triple(m)
    inputs, _ = batch(0)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        type(t.m32).ref(t.m32, inputs[0])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        type(t.mh).hip(t.mh, inputs[0].cuda().requires_grad_(True))
    with pytest.raises(ValueError, match="more than 1 value per channel"), torch.no_grad():
        type(t.mh).hip(t.mh, inputs[0].cuda())


# ---- 5. agreement between paths -------------------------------------------------------------------------------------------------
def _agree(title, a, b, ref, bound_c):
    a, b, ref = (t.detach().cpu().double() for t in (a, b, ref))
    ea, eb = float((a - ref).abs().max()), float((b - ref).abs().max())
    bound = max(ea, eb, bound_c * float(ref.abs().max()))
    d = float((a - b).abs().max())
    print(f"{title}: max |a - b| {d:.2e} (bound {bound:.2e}; against float64 {ea:.2e} / {eb:.2e})")
    assert d <= bound, (title, d, bound)


@pytest.mark.parametrize("case", ["k3s1", "k1s1_bias", "k3s2"])
def test_convbn_fused_vs_composed(case):
    """The fused conv + BN entries against the composed ones (forced by a counter on the CPU), on the same layer and batch."""
    m, batch, gi = _make("convbn", **CONV_CASES[case])
    a, b = _triple(m), _triple(m)
    for mod in b.mh.modules():
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            mod.num_batches_tracked = mod.num_batches_tracked.cpu()
    inputs, w = batch(0)
    ra, rb = a.step(inputs, w, gi), b.step(inputs, w, gi)
    for k in ra:
        _agree(f"convbn[{case}] fused vs composed {k}", ra[k][0], rb[k][0], ra[k][1], C_OUT if k == "out" else C_GRAD)


def test_pfn_fused_vs_composed():
    m, batch, gi = _make("pfn", shape=(500, 32, 10, 64))
    a = _triple(m)
    b = _triple(m)
    b.mh.fused = False
    inputs, w = batch(0)
    ra, rb = a.step(inputs, w, gi), b.step(inputs, w, gi)
    for k in ra:
        _agree(f"pfn fused vs composed {k}", ra[k][0], rb[k][0], ra[k][1], C_OUT if k == "out" else C_GRAD)


def test_convbn_backward_streams(modes):
    """The fused stride-1 backward (MODE_BWD_STREAMS 0) against the side-stream composition (1 on a large map, 2 always)."""
    m, batch, gi = _make("convbn", shape=(2, 16, 256, 288), cout=32, bias=True)
    inputs, w = batch(0)
    runs = {}
    for mode in (0, 1, 2):
        modes(bwd_streams=mode)
        t = _triple(m)
        runs[mode] = t.step(inputs, w, gi)
    for mode in (1, 2):
        for k in runs[0]:
            _agree(f"convbn bwd_streams 0 vs {mode} {k}", runs[0][k][0], runs[mode][k][0], runs[0][k][1], C_OUT if k == "out" else C_GRAD)
