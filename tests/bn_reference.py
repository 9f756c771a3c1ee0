"""Float64 truth for the training-mode BatchNorm tests (test_gpu_bn_train.py).

One torch module (BatchNorm with the Conv2d / Linear / row GEMM in front where a HIP path fuses one) is copied three ways: float64 on the
CPU (the truth), float32 on the CPU (torch's own fp32 error, which sets the bound) and float32 on the GPU (the HIP path under test).  All
three see the same batches and the same upstream gradient w; the loss is (out * w).sum().  A HIP result passes when

    max|err| <= max(4 max|err_torch_fp32|, c max|ref|)   and   rms(err) <= max(2 rms(err_torch_fp32), c rms(ref))

with c = C_OUT for outputs and C_GRAD for gradients (the c terms are floors for cases where torch fp32 happens to be exact)."""
import copy
import math

import torch

C_OUT = 4e-6
C_GRAD = 2e-5
RTOL_STATS = 1e-6


class Report:
    """Worst margin per quantity: printed by the tests (pytest -s), asserted as it goes."""

    def __init__(self, title):
        self.title, self.lines, self.worst = title, [], 0.0

    def check(self, what, got, ref, f32, c):
        got, ref, f32 = (t.detach().cpu().double() for t in (got, ref, f32))
        assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
        e, ef = (got - ref).abs(), (f32 - ref).abs()
        bound = max(4.0 * float(ef.max()), c * float(ref.abs().max()))
        rms, rms_bound = _rms(e), max(2.0 * _rms(ef), c * _rms(ref))
        emax = float(e.max()) if e.numel() else 0.0
        ratio = max(emax / bound if bound > 0 else (0.0 if emax == 0 else math.inf), rms / rms_bound if rms_bound > 0 else (0.0 if rms == 0 else math.inf))
        self.worst = max(self.worst, ratio)
        line = (f"{self.title} {what}: max err {emax:.2e} (bound {bound:.2e}, torch fp32 {float(ef.max()):.2e}), "
                f"rms {rms:.2e} (bound {rms_bound:.2e}), use {ratio:.2f}")
        self.lines.append(line)
        assert math.isfinite(emax) and emax <= bound and rms <= rms_bound, line

    def stats(self, what, got, ref, rtol=RTOL_STATS):
        got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
        e = (got - ref).abs()
        tol = rtol * ref.abs() + 0.5 * rtol * float(ref.abs().max())   # float32 rounding of near-zero entries
        use = float((e / tol).max()) if e.numel() else 0.0
        line = f"{self.title} {what}: max rel err {float((e / ref.abs().clamp_min(1e-30)).max()):.2e} (rtol {rtol:.0e}), use {use:.2f}"
        self.lines.append(line)
        assert use <= 1.0, line

    def show(self):
        for line in self.lines:
            print(line)
        print(f"{self.title}: worst use of the bound {self.worst:.2f}")


def _rms(t):
    return float(t.square().mean().sqrt()) if t.numel() else 0.0


class Triple:
    """The module under test in float64 / float32 on the CPU and float32 on the GPU.  step(): one training step of each on the same
    batch; the GPU one through `hip(module, *inputs)`, the CPU ones through `ref(module, *inputs)` (plain torch ops)."""

    def __init__(self, module, ref, hip, device="cuda"):
        self.m64 = copy.deepcopy(module).double()
        self.m32 = copy.deepcopy(module).float()
        self.mh = copy.deepcopy(module).float().to(device)
        self.ref, self.hip, self.device = ref, hip, device

    def train(self, mode=True):
        for m in (self.m64, self.m32, self.mh):
            m.train(mode)
        return self

    def step(self, inputs, w, grad_inputs=(0,), zero_grad=True):
        """inputs: CPU float32 tensors; w: CPU float32 upstream gradient. Returns {name: (hip, f64, f32)} of the output, the gradients of
        inputs[i] for i in grad_inputs ("d_in<i>") and of every parameter that requires one ("d_<name>")."""
        res = {}
        outs = []
        for m, dt, dev, fn in ((self.m64, torch.float64, "cpu", self.ref), (self.m32, torch.float32, "cpu", self.ref),
                               (self.mh, torch.float32, self.device, self.hip)):
            if zero_grad:
                m.zero_grad(set_to_none=True)
            xs = [t.to(dev, dt).clone().requires_grad_(i in grad_inputs) for i, t in enumerate(inputs)]
            out = fn(m, *xs)
            (out * w.to(dev, dt)).sum().backward()
            outs.append((out, [xs[i].grad for i in grad_inputs], {k: p.grad for k, p in m.named_parameters() if p.requires_grad}))
        (oh, gh, ph), (o64, g64, p64), (o32, g32, p32) = outs[2], outs[0], outs[1]
        res["out"] = (oh, o64, o32)
        for i, a, b, c in zip(grad_inputs, gh, g64, g32):
            res[f"d_in{i}"] = (a, b, c)
        for k in p64:
            res["d_" + k] = (ph[k], p64[k], p32[k])
        return res

    def check_step(self, rep, res, prefix=""):
        for k, (got, ref, f32) in res.items():
            assert got is not None, prefix + k
            rep.check(prefix + k, got, ref, f32, C_OUT if k == "out" else C_GRAD)

    def check_buffers(self, rep):
        b64 = dict(self.m64.named_buffers())
        for k, b in self.mh.named_buffers():
            if b.is_floating_point():
                rep.stats(k, b, b64[k])
            else:
                assert int(b) == int(b64[k]), (k, int(b), int(b64[k]))

