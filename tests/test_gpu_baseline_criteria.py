"""The HEAL and MPDA training criteria on the GPU (``gencomm_pyramid_occ_loss``, ``gencomm_domain_bce_loss``,
``gencomm_amd/baseline_criteria.py``) against what the reference's own modules produced in float64
(tests/golden/baseline_criteria.npz). The bar is the project's: max(2 e_ref, 1e-6), e_ref the error of the reference's own float32
run; a loss by its relative difference, a gradient by its rms-relative difference per tensor.

Every e_ref of the fixture is below 2e-7, so the bar is 1e-6 throughout. Measured on an MI355X when these tests were written (each
test prints its figures): losses within 5.6e-8, ``loss_dict`` entries within 1.4e-7, level losses within 2.5e-7, gradients within
1.6e-7 rms."""
import json

import numpy as np
import pytest
import torch

import baseline_criteria_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bar(e_ref):
    return max(2.0 * float(e_ref), 1e-6)


@pytest.fixture(scope="module")
def store():
    return np.load(R.GOLDEN)


def case_of(store, name):
    kind, args, extra = str(store[f"{name}/kind"]), json.loads(str(store[f"{name}/args"])), json.loads(str(store[f"{name}/extra"]))
    inp = {k.split("/in/")[1]: store[k] for k in store.files if k.startswith(f"{name}/in/")}
    return kind, args, inp, extra


def run_gpu(store, name, cotangent=None, crit_cls=None):
    """One step of case `name` through the package's criterion -> (total, loss_dict, {name: gradient}, criterion)."""
    from gencomm_amd import baseline_criteria as BC
    kind, args, inp, extra = case_of(store, name)
    t = R.tensors(inp, torch.float32, DEV)
    out, tgt = R.dicts(kind, t, extra.get("record_len"))
    junk = torch.full((1 << 20,), float("nan"), device=DEV)   # NaNs in the memory the allocator hands out next
    del junk
    if kind == "mpda":
        crit = BC.PointPillarMPDALoss(args)
        total = crit(out, tgt, validate=extra["validate"])
    else:
        crit = (crit_cls or BC.PointPillarPyramidLoss)(args)
        total = crit(out, tgt, "_single" if kind == "occ" else "")
    (total if cotangent is None else total * cotangent).backward()
    grads = {k: v.grad for k, v in t.items() if v.requires_grad and v.grad is not None}
    return total.detach(), dict(crit.loss_dict), grads, crit


CASES = list(R.all_cases())


@pytest.mark.parametrize("name", CASES)
def test_case_vs_reference(name, store):
    total, d, grads, crit = run_gpu(store, name)
    torch.cuda.synchronize()
    lim = bar(R.rel(store[f"{name}/loss32"], store[f"{name}/loss64"]))
    err = R.rel(total, store[f"{name}/loss64"])
    print(f"{name} loss {float(total):.7f}: rel err {err:.2e} (bar {lim:.1e})")
    assert np.isfinite(float(total)) and err <= lim, (name, "loss", err, lim)
    stored = {k.split("/dict64/")[1] for k in store.files if k.startswith(f"{name}/dict64/")}
    assert stored == set(d), (stored, set(d))
    for k in sorted(d):
        lim, err = bar(R.rel(store[f"{name}/dict32/{k}"], store[f"{name}/dict64/{k}"])), R.rel(d[k], store[f"{name}/dict64/{k}"])
        print(f"{name} loss_dict[{k}]: rel err {err:.2e} (bar {lim:.1e})")
        assert not d[k].requires_grad and err <= lim, (name, k, err, lim)
    want = {k.split("/grad64/")[1] for k in store.files if k.startswith(f"{name}/grad64/")}
    assert want == set(grads), (want, set(grads))
    for k in sorted(grads):
        g64 = store[f"{name}/grad64/{k}"]
        lim, err = bar(store[f"{name}/e32/{k}"]), R.rms_rel(grads[k].cpu().numpy(), g64)
        print(f"{name} d {k}: rms-rel err {err:.2e} (bar {lim:.1e})")
        assert tuple(grads[k].shape) == g64.shape and torch.isfinite(grads[k]).all() and err <= lim, (name, k, err, lim)
    if case_of(store, name)[0] == "occ":
        levels = crit.level_losses.cpu()
        assert abs(float(levels.double().sum()) - float(total)) <= 1e-6 * abs(float(total))
        for i, v in enumerate(levels):
            lim = bar(R.rel(store[f"{name}/level32/{i}"], store[f"{name}/level64/{i}"]))
            err = R.rel(v, store[f"{name}/level64/{i}"])
            print(f"{name} level {i}: rel err {err:.2e} (bar {lim:.1e})")
            assert err <= lim, (name, i, err, lim)


def test_collab_form_is_the_depth_criterion_bit_for_bit(store):
    from gencomm_amd import PointPillarDepthLoss
    a = run_gpu(store, "pyr_collab")
    b = run_gpu(store, "pyr_collab", crit_cls=lambda args: PointPillarDepthLoss({k: v for k, v in args.items() if k != "pyramid"}))
    assert torch.equal(a[0], b[0]) and sorted(a[1]) == sorted(b[1]) and sorted(a[2]) == sorted(b[2])
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.parametrize("name", ["occ_wide", "pyr_single", "mpda", "mpda_b"])
def test_two_runs_are_bit_identical_and_a_cotangent_scales_exactly(name, store):
    a, b, h = run_gpu(store, name), run_gpu(store, name), run_gpu(store, name, cotangent=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], h[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
        assert torch.equal(a[2][k] * 0.5, h[2][k]) and a[2][k].abs().max() > 0, k    # a cotangent of 0.5 halves every gradient exactly


def test_validate_leaves_the_domain_term_out(store):
    tr, va = run_gpu(store, "mpda"), run_gpu(store, "mpda_val")
    assert "da_feature" in tr[2] and "da_feature" not in va[2]
    assert float(va[1]["da_loss"]) == 0.0 and float(tr[1]["da_loss"]) > 0.0
    heads = sum(float(va[1][k]) for k in ("cls_loss", "reg_loss", "dir_loss"))
    assert abs(float(va[0]) - heads) <= 1e-6 * heads
    assert abs(float(tr[0]) - float(va[0]) - 2.0 * float(tr[1]["da_loss"])) <= 2e-6 * float(tr[0])   # added twice, logged once
    for k in ("psm", "rm", "dm"):
        assert torch.equal(tr[2][k], va[2][k]), k


def test_second_derivative_raises(store):
    from gencomm_amd import baseline_criteria as BC
    kind, args, inp, extra = case_of(store, "occ_k3")
    t = R.tensors(inp, torch.float32, DEV)
    out, tgt = R.dicts(kind, t)
    one = lambda: torch.ones((), device=DEV, requires_grad=True)      # a cotangent with a history: what a gradient penalty hands in
    (g,) = torch.autograd.grad(BC.PointPillarPyramidLoss(args)(out, tgt, "_single"), t["occ0"], one(), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    x = t["occ0"].detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(BC.domain_bce_loss(x, [1, 1]), x, one(), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    (g,) = torch.autograd.grad(BC.domain_bce_loss(x, [1, 1]), x, create_graph=True)   # a constant cotangent: the gradient has no history at all
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---------------------------------------------------------------------------------------------- composition with the trainable cores
def _judge(what, got, t64, t32, floor=0.0):
    import pyramid_train_restatement as TR
    e, y = TR.rel_rms(TR.np64(got), TR.np64(t64), floor), TR.rel_rms(TR.np64(t32), TR.np64(t64), floor)
    print(f"{what}: rms-rel err {e:.2e}, float32 yardstick {y:.2e}")
    assert np.isfinite(TR.np64(got)).all() and e <= bar(y), (what, e, y)


def test_pyramid_fusion_single_pass_trains_under_the_occupancy_criterion():
    """PyramidFusion(trainable=True).forward_single on the 24 x 40 map of the `single` training case, its three occupancy maps into
    PointPillarPyramidLoss (collab, "_single"), backward: the loss, the input gradient and the three heads' gradients against torch
    autograd of the restatements in float64; yardstick: the same in float32.

    The labels are sparse, as detection labels are (0.4 % of the anchors positive, 2 % in the don't-care band). A head's bias gradient
    is ONE number, the sum of its level's occupancy gradient, in which positive cells pull one way and negative cells the other; it is
    judged by its relative error, so it must not be what is left of two cancelling halves (tests/pyramid_train_restatement.py,
    case_inputs, on the same matter: there the cotangents are chosen positive; here the criterion chooses them). With 2 % positives the
    level-1 sum is a tenth of the sum of its magnitudes in float64 and every float32 rounding of a cell counts ten times; with these
    labels the ratio stays below 2 at every level, which is asserted on the float64 step."""
    import pyramid_restatement as PR
    import pyramid_train_restatement as TR
    from gencomm_amd import PointPillarPyramidLoss, PyramidFusion
    x = TR.case_inputs("single")[0]
    lab = np.random.RandomState(7401).rand(1, TR.H0, TR.W0, 2)
    pos, neg = (lab < 0.004).astype(np.float32), (lab > 0.02).astype(np.float32)
    args = R.pyramid_args([1, 2, 4], [0.4, 0.2, 0.1])
    heads = [f"single_head_{i}.{p}" for i in range(3) for p in ("weight", "bias")]

    def restated(dtype):
        m = TR.restatement(dtype).train()
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        _, occs = m.forward_single(xt)
        assert [tuple(o.shape) for o in occs] == [(1, 1, 24, 40), (1, 1, 12, 20), (1, 1, 6, 10)]
        for o in occs:
            o.retain_grad()
        loss = R.occ_loss(occs, torch.from_numpy(pos).to(dtype), torch.from_numpy(neg).to(dtype), [1, 2, 4], [0.4, 0.2, 0.1], 2.0, 2.0, 0.25)[0]
        loss.backward()
        named = dict(m.named_parameters())
        return loss.detach(), xt.grad, {k: named[k].grad for k in heads}, [o.grad for o in occs]

    t64, t32 = restated(torch.float64), restated(torch.float32)
    assert pos.sum() >= 8 and all(float(g.abs().sum() / g.sum().abs()) < 2.0 for g in t64[3])
    torch.manual_seed(0)
    m = PR.fill_params_(PyramidFusion(PR.cfg(), input_channels=64, trainable=True)).to(DEV).train()
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    _, occs = m.forward_single(xd)
    crit = PointPillarPyramidLoss(args)
    loss = crit({"pyramid": "collab", "occ_single_list": occs}, {"pos_equal_one": torch.from_numpy(pos).to(DEV), "neg_equal_one": torch.from_numpy(neg).to(DEV)},
                "_single")
    loss.backward()
    lim, err = bar(R.rel(t32[0], t64[0])), R.rel(loss.detach(), t64[0])
    print(f"pyramid single + criterion loss {float(loss.detach()):.6f}: rel err {err:.2e} (bar {lim:.1e})")
    assert err <= lim
    _judge("pyramid single + criterion d x", xd.grad, t64[1], t32[1])
    named = dict(m.named_parameters())
    for k in heads:
        _judge(f"pyramid single + criterion d {k}", named[k].grad, t64[2][k], t32[2][k])


def test_mpda_aligner_trains_under_the_mpda_criterion():
    """MPDAAlign(trainable=True) on the `align` training case (record_len [1, 3, 2]); its class_logits are the da_feature of
    PointPillarMPDALoss, whose head maps do not depend on the aligner: every gradient of the aligner comes through the classifier's
    gradient-reversal layer (-9.1) from the domain term, which the criterion adds twice."""
    import mpda_train_restatement as TR
    from gencomm_amd import PointPillarMPDALoss
    from test_gpu_mpda_train import check, check_zero, zero_truth
    from test_mpda_train import package_module
    tag = "align"
    rl = TR.TRAIN_CASES[tag]["record_len"]
    x = TR.case_inputs(tag)[0]
    heads = R.head_inputs(7402, len(rl), 6, 10)
    m = package_module(tag)

    def restated(dtype, reversal=-9.1, twice=True):
        sd = TR.leaf_sd(m, dtype)
        xc = torch.from_numpy(x).to(dtype).requires_grad_(True)
        _, logits = TR.mpda_align(sd, TR.case_args(tag), xc, rl, reversal=reversal)
        t = R.tensors(heads, dtype, grad=False)
        out, tgt = R.dicts("mpda", dict(t, da_feature=logits), rl)
        loss = R.mpda_loss(R.MPDA_ARGS, out, tgt)[0] if twice else R.domain_bce_stable(logits, rl)
        gi, gp = TR.grads_of(loss, sd, {"x": xc})
        return loss.detach(), gi["x"], gp

    t64, t32 = restated(torch.float64), restated(torch.float32)
    m = m.to(DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    _, logits = m(xd, rl)
    out, tgt = R.dicts("mpda", dict(R.tensors(heads, torch.float32, DEV, grad=False), da_feature=logits), rl)
    crit = PointPillarMPDALoss(R.MPDA_ARGS)
    loss = crit(out, tgt)
    loss.backward()
    lim, err = bar(R.rel(t32[0], t64[0])), R.rel(loss.detach(), t64[0])
    print(f"mpda aligner + criterion loss {float(loss.detach()):.6f}: rel err {err:.2e} (bar {lim:.1e})")
    assert err <= lim
    check("mpda aligner + criterion d x", xd.grad, t64[1], t32[1])
    got = {k: p.grad for k, p in m.named_parameters()}
    assert sorted(got) == sorted(t64[2])
    for k in t64[2]:
        if zero_truth(k, False):
            check_zero(f"mpda aligner + criterion d {k}", got[k], t32[2][k], t64[2][k[:-4] + "weight"])
        else:
            check(f"mpda aligner + criterion d {k}", got[k], t64[2][k], t32[2][k])
    # the reversal scale with the doubled term: -9.1 x 2 x the plain gradient of ONE domain term without the reversal layer
    p64, p32 = restated(torch.float64, None, False), restated(torch.float32, None, False)
    check("mpda aligner d x against -18.2 x the plain single-term gradient", xd.grad, -18.2 * p64[1], -18.2 * p32[1])
    k = "resizer.wg_att_1.layers.0.block.1.fn.to_out.0.weight"
    check(f"mpda aligner d {k} against -18.2 x the plain single-term gradient", got[k], -18.2 * p64[2][k], -18.2 * p32[2][k])
