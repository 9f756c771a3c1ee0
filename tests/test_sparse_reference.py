"""CPU tests that pin tests/sparse_reference.py (the coordinate-based float64 reference the GPU sparse-kernel tests rest on) before
anything rests on it: hand-worked single-voxel cases, and agreement with the dense-volume oracle (oracle/second_port.py: dense
masks, dense convolutions, float64 autograd for the input / weight gradients) on grids of at most 9 x 9 x 9."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sparse_reference as R

GRIDS = [(5, 7, 6), (6, 1, 9), (9, 8, 8)]
SUBM = [(3, 3, 3), (3, 1, 1), (1, 1, 1)]
STRIDED = [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))]


def _scene(dims, B, seed, fill=0.3, C=3):
    rng = np.random.RandomState(seed)
    cells = [(b, z, y, x) for b in range(B) for z in range(dims[0]) for y in range(dims[1]) for x in range(dims[2])]
    pick = rng.permutation(len(cells))[:max(int(fill * len(cells)), 1)]
    coords = np.array([cells[i] for i in pick], dtype=np.int64)
    return coords, rng.standard_normal((len(coords), C))


def test_key_order_and_out_of_grid_rows():
    dims = (3, 4, 5)
    coords = np.array([[1, 0, 0, 0], [0, 2, 3, 4], [0, 0, 0, -1], [0, 0, 0, 1], [0, 3, 0, 0], [2, 0, 0, 0], [0, 0, 4, 0], [0, 0, 0, 0]])
    keys, perm = R.index(coords, 2, dims)
    assert keys.tolist() == [0, 1, 59, 60, R.NO_KEY, R.NO_KEY, R.NO_KEY, R.NO_KEY]      # ((b D + z) H + y) W + x
    assert perm.tolist() == [7, 3, 1, 0, 2, 4, 5, 6]                                      # no-key rows last, in input order
    assert R.decode(59, dims) == (0, 2, 3, 4) and R.decode(60, dims) == (1, 0, 0, 0)
    k0, p0 = R.index(np.zeros((0, 4), dtype=np.int64), 1, dims)
    assert len(k0) == 0 and len(p0) == 0


def test_hand_worked_single_voxel_cases():
    """The cases of test_oracle_known_answers_submanifold_and_strided_site_sets, from coordinates."""
    dims = (9, 9, 9)
    w = np.arange(2 * 27 * 3, dtype=np.float64).reshape(2, 27, 3) / 100.0
    f = np.array([[1.0, 2.0, 3.0]])
    scale, shift = np.array([1.0, 2.0]), np.array([0.5, -0.25])
    keys, _ = R.index([[0, 4, 4, 4]], 1, dims)
    nbr = R.subm_rules(keys, dims, (3, 3, 3))
    assert nbr[:, 0].tolist() == [-1] * 13 + [0] + [-1] * 13                              # one voxel: centre tap only
    y = R.gather_gemm(f, nbr, R.effective_weight(w, 27, 3, 2, 0), scale, shift, True)
    assert np.allclose(y[0], np.maximum((w[:, 13, :] @ f[0]) * scale + shift, 0), atol=1e-12)
    # strided k 3, stride 2, pad 1: an even coordinate lies in ONE receptive field per axis, an odd one in TWO
    geo = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
    assert R.out_dims(dims, *geo) == [5, 5, 5]
    even = R.sites(keys, dims, *geo)
    assert [R.decode(k, (5, 5, 5)) for k in even] == [(0, 2, 2, 2)]
    keys5, _ = R.index([[0, 5, 5, 5]], 1, dims)
    odd = R.sites(keys5, dims, *geo)
    assert sorted(R.decode(k, (5, 5, 5)) for k in odd) == [(0, z, y, x) for z in (2, 3) for y in (2, 3) for x in (2, 3)]
    nb5 = R.rules(odd, (5, 5, 5), keys5, dims, *geo)
    j333 = [R.decode(k, (5, 5, 5)) for k in odd].index((0, 3, 3, 3))
    assert nb5[:, j333].tolist() == [0] + [-1] * 26                                       # output (3,3,3) covers inputs 5..7: tap 0 in every axis
    y5 = R.gather_gemm(f, nb5, R.effective_weight(w, 27, 3, 2, 0), scale, shift, True)
    assert np.allclose(y5[j333], np.maximum((w[:, 0, :] @ f[0]) * scale + shift, 0), atol=1e-12)
    # a truncated strided layer: D = 6, kernel (3, 1, 1), stride 2, pad 0 -> two output planes (inputs 0..2, 2..4); z = 5 reaches nothing
    t = ((3, 1, 1), (2, 1, 1), (0, 0, 0))
    assert R.out_dims((6, 2, 2), *t) == [2, 2, 2]
    k5, _ = R.index([[0, 5, 0, 0], [0, 5, 1, 1]], 1, (6, 2, 2))
    assert len(R.sites(k5, (6, 2, 2), *t)) == 0
    k2, _ = R.index([[0, 2, 1, 0]], 1, (6, 2, 2))
    assert [R.decode(k, (2, 2, 2)) for k in R.sites(k2, (6, 2, 2), *t)] == [(0, 0, 1, 0), (0, 1, 1, 0)]
    # no wrap across the row / plane / sample boundary: (y, W-1) and (y+1, 0) are neighbours in key space only
    kk, _ = R.index([[0, 0, 0, 4], [0, 0, 1, 0], [0, 2, 3, 4], [1, 0, 0, 0]], 2, (3, 4, 5))
    assert kk.tolist() == [4, 5, 59, 60]
    nb = R.subm_rules(kk, (3, 4, 5), (3, 3, 3))
    assert (nb >= 0).sum() == 4 and nb[13].tolist() == [0, 1, 2, 3]
    # MeanVFE divides the sum over ALL slots by max(num_points, 1)
    v = np.array([[[1.0, 2.0], [3.0, 4.0], [0.0, 0.0]], [[5.0, 6.0], [0.0, 0.0], [0.0, 0.0]]])
    assert np.array_equal(R.mean_vfe(v, [2, 0]), [[2.0, 3.0], [5.0, 6.0]])
    assert np.array_equal(R.mean_vfe(v, [2, 0], perm=[1, 0]), [[5.0, 6.0], [2.0, 3.0]])


def _dense_inputs(coords, feats, B, dims):
    import second_port as S
    x, m = S.to_dense(torch.from_numpy(feats), torch.from_numpy(coords), B, list(dims))
    return x.requires_grad_(True), m


@pytest.mark.parametrize("dims", GRIDS, ids=str)
@pytest.mark.parametrize("kernel", SUBM, ids=str)
def test_subm_rulebook_and_gather_gemm_reproduce_the_dense_oracle(dims, kernel):
    import second_port as S
    B, cin, cout, K = 2, 3, 2, R.prod3(kernel)
    coords, feats = _scene(dims, B, seed=sum(dims) + K)
    rng = np.random.RandomState(K)
    w = rng.standard_normal((cout, *kernel, cin))
    keys, perm = R.index(coords, B, dims)
    assert np.array_equal(R.dense(feats[perm], keys, B, dims), S.to_dense(torch.from_numpy(feats), torch.from_numpy(coords), B, list(dims))[0].numpy())
    nbr = R.subm_rules(keys, dims, kernel)
    y = R.gather_gemm(feats[perm], nbr, R.effective_weight(w, K, cin, cout, 0), np.ones(cout), np.zeros(cout), False)
    x, m = _dense_inputs(coords, feats, B, dims)
    wt = torch.from_numpy(w).requires_grad_(True)
    yd = F.conv3d(x, S.torch_weight(wt, kernel), padding=tuple(k // 2 for k in kernel)) * m
    assert np.allclose(R.dense(y, keys, B, dims), yd.detach().numpy(), rtol=0, atol=1e-12)
    # the spconv 1.x layout holds the same numbers
    w1 = np.ascontiguousarray(w.reshape(cout, K, cin).transpose(1, 2, 0))
    assert np.array_equal(R.effective_weight(w1, K, cin, cout, 1), R.effective_weight(w, K, cin, cout, 0))
    # gradients: input gradient = the same gather-GEMM on dy with the layout-3 weight and the FORWARD rulebook; weight gradient
    gy = rng.standard_normal(y.shape)
    gx, gw = torch.autograd.grad((yd * torch.from_numpy(R.dense(gy, keys, B, dims))).sum(), [x, wt])
    dx = R.gather_gemm(gy, nbr, R.effective_weight(w, K, cout, cin, 3), np.ones(cin), np.zeros(cin), False)
    assert np.allclose(R.dense(dx, keys, B, dims), (gx * m).numpy(), rtol=0, atol=1e-12)
    dw = R.wgrad(feats[perm], gy, nbr, np.zeros((cout, K, cin)))
    assert np.allclose(dw, gw.numpy().reshape(cout, K, cin), rtol=0, atol=1e-12)
    dw1 = R.wgrad(feats[perm], gy, nbr, np.full((cout, K, cin), 0.5))
    assert np.allclose(dw1, dw + 0.5, rtol=0, atol=1e-12)                                # the contract is +=


@pytest.mark.parametrize("dims", GRIDS, ids=str)
@pytest.mark.parametrize("geo", STRIDED, ids=str)
@pytest.mark.parametrize("fill", [0.3, 0.03])
def test_strided_sites_rulebooks_and_gather_gemm_reproduce_the_dense_oracle(dims, geo, fill):
    import second_port as S
    kernel, stride, pad = geo
    B, cin, cout, K = 2, 3, 2, R.prod3(kernel)
    coords, feats = _scene(dims, B, seed=sum(dims) + K + int(100 * fill), fill=fill)
    rng = np.random.RandomState(K + 1)
    w = rng.standard_normal((cout, *kernel, cin))
    keys, perm = R.index(coords, B, dims)
    od = R.out_dims(dims, kernel, stride, pad)
    x, m = _dense_inputs(coords, feats, B, dims)
    mo = (F.max_pool3d(m, kernel, stride, pad) > 0).double()
    assert list(mo.shape[2:]) == od
    okeys = R.sites(keys, dims, kernel, stride, pad)
    assert np.all(np.diff(okeys) > 0)
    assert [R.decode(k, od) for k in okeys] == [tuple(int(v) for v in (c[0], c[2], c[3], c[4])) for c in torch.nonzero(mo)]
    nbr = R.rules(okeys, od, keys, dims, kernel, stride, pad)
    y = R.gather_gemm(feats[perm], nbr, R.effective_weight(w, K, cin, cout, 0), np.ones(cout), np.zeros(cout), False)
    wt = torch.from_numpy(w).requires_grad_(True)
    yd = F.conv3d(x, S.torch_weight(wt, kernel), stride=stride, padding=pad) * mo
    assert np.allclose(R.dense(y, okeys, B, od), yd.detach().numpy(), rtol=0, atol=1e-12)
    # inverse rulebook + layout 2 = the input gradient; weight gradient
    inv = R.rules_inv(keys, dims, okeys, od, kernel, stride, pad)
    assert inv.shape == (K, len(keys)) and int((inv >= 0).sum()) == int((nbr >= 0).sum())
    gy = rng.standard_normal(y.shape)
    gx, gw = torch.autograd.grad((yd * torch.from_numpy(R.dense(gy, okeys, B, od))).sum(), [x, wt])
    dx = R.gather_gemm(gy, inv, R.effective_weight(w, K, cout, cin, 2), np.ones(cin), np.zeros(cin), False)
    assert np.allclose(R.dense(dx, keys, B, dims), (gx * m).numpy(), rtol=0, atol=1e-12)
    assert np.allclose(R.wgrad(feats[perm], gy, nbr, np.zeros((cout, K, cin))), gw.numpy().reshape(cout, K, cin), rtol=0, atol=1e-12)


def test_scale_shift_relu_magnitude_and_the_float32_evaluation():
    rng = np.random.RandomState(3)
    n_in, n_out, K, cin, cout = 40, 70, 27, 20, 12
    x, w = rng.standard_normal((n_in, cin)), rng.standard_normal((cout, K, cin))
    nbr = rng.randint(-1, n_in, size=(K, n_out)).astype(np.int32)
    scale, shift = rng.uniform(0.5, 2, cout) * rng.choice([-1, 1], cout), rng.standard_normal(cout)
    weff = R.effective_weight(w, K, cin, cout, 0)
    y = R.gather_gemm(x, nbr, weff, scale, shift, True)
    want = np.zeros((n_out, cout))
    for j in range(n_out):
        for o in range(K):
            if nbr[o, j] >= 0:
                want[j] += w[:, o, :] @ x[nbr[o, j]]
    assert np.allclose(y, np.maximum(want * scale + shift, 0), rtol=0, atol=1e-12)
    S_ = R.gather_gemm_magnitude(x, nbr, weff, scale, shift)
    assert (S_ >= np.abs(R.gather_gemm(x, nbr, weff, scale, shift, False)) - 1e-12).all()
    assert (R.gather_gemm_magnitude(x, nbr, weff, scale, shift, tile_max=64) >= S_).all()
    y32 = R.gather_gemm(x.astype(np.float32), nbr, weff.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32), False, dtype=np.float32)
    assert y32.dtype == np.float32
    y64 = R.gather_gemm(x.astype(np.float32), nbr, weff.astype(np.float32), scale.astype(np.float32), shift.astype(np.float32), False)
    r32 = R.worst_ratio(y32, y64, S_)
    assert 0 < r32 < 2.0 ** -20                  # float32 rounding of a 540-term sum, not float64 and not broken
    dy = rng.standard_normal((n_out, cout))
    dw32 = R.wgrad(x.astype(np.float32), dy.astype(np.float32), nbr, np.ones((cout, K, cin), np.float32), dtype=np.float32)
    dw64 = R.wgrad(x.astype(np.float32), dy.astype(np.float32), nbr, np.ones((cout, K, cin)))
    assert dw32.dtype == np.float32
    assert 0 < R.worst_ratio(dw32, dw64, R.wgrad_magnitude(x, dy, nbr, np.ones((cout, K, cin)))) < 2.0 ** -20
