"""The sparse-convolution kernels of the SECOND encoder (gencomm_amd/csrc/sparse_kernels.h) called directly through the entry points
that gencomm_amd/second.py binds, one kernel per test, against the coordinate-based float64 reference tests/sparse_reference.py.

  index builders   gencomm_sp_index_fwd, _rules_fwd, _sites_fwd, _rules_inv_fwd: exact integer equality (keys, perm, rulebooks, site
                   sets, counts) on grids with odd, even and 1-wide axes, sites on every corner and face, neighbours across the row /
                   plane / sample boundary, truncated strided layers, empty inputs and outputs, out-of-grid rows
  gather-GEMM      gencomm_sp_prepare + gencomm_sp_conv_fwd: sp_conv_kernel<CIN> (exact fp32, default mode) and
                   sp_conv_f16s_kernel<CIN> (GENCOMM_MODE_ARITH = 3), on synthetic rulebooks (random int32 in [-1, n_in)); which
                   kernel ran is read from the kernel log
  weight gradient  gencomm_sp_wgrad at every rows_per_block the host chooses (64 .. 1024), ragged last chunks, dw pre-filled (+=)
  MeanVFE, dense   gencomm_mean_vfe_fwd, gencomm_sp_dense_fwd and the gradient of SparseTensor.dense()
  module           SECOND under mode 3 against oracle/second_port.py in float64; out-of-grid voxels change nothing

Floating-point pass rule (no absolute number fixed in advance): per element, |got - ref64| / S with
S = |scale| sum |w| |x| + |shift| (weight gradient: sum |x| |dy| + |pre-filled value|), against the same sums evaluated in numpy float32
offset by offset (worst ratio r32): exact-fp32 kernel and weight gradient <= 4 r32 (another summation order: MFMA k-order, per-offset
partial sums, 64-row chunks and float atomics); two-term split kernel <= 4 r32 + 4 * 2^-22 (2^-22 each for the rounding of either
operand's low half and the dropped lo * lo term, one unit of headroom; where one input of a 64-site tile is 1e4 larger than the rest S
counts every gathered |x| as the tile's largest, as the shared activation scale of the kernel implies). Ratios are pooled over the
n_out / K sweep of one test. Outputs are pre-filled with a sentinel and sit between guard bands, so an element a kernel leaves out or a
write past the end fails the test.

Measured on MI355X (worst ratio of the kernel / r32; see the printed line of each test):
  family (tests)                                        kernel worst ratio   smallest r32   largest worst / bound
  sp_conv_kernel, K = 27 / 3 / 1 (8 shapes each)        3.0e-7 / 3.5e-7 / 2.4e-7   1.3e-7    0.30
  prepare layouts 0 .. 3 (5 shapes each)                2.4e-7                      1.1e-7    0.34
  sp_conv_f16s_kernel unit / tiny / huge (6 each)       2.0e-7 / 2.4e-7 / 1.9e-7   2.0e-7    0.11
  sp_conv_f16s_kernel zero_first_offsets (6)            1.9e-7                      2.3e-7    0.09
  sp_conv_f16s_kernel late_outlier, S per tile (6)      5.2e-8                      4.1e-8    0.04
  sp_wgrad_kernel n_out 1 / 65 / 550          (rows_per_block 64)               1.0e-7 / 2.3e-7 / 6.5e-8   r32 1.0e-7 / 2.3e-7 / 1.7e-7
  sp_wgrad_kernel n_out 2500 / 4700 / 9300 / 19000 (128 / 256 / 512 / 1024)     3.4e-8 / 2.9e-8 / 1.8e-8 / 1.2e-8   r32 6.5e-8 / 5.0e-8 / 3.2e-8 / 2.7e-8
  sp_wgrad_kernel (4,16) (16,32) (64,64), K 3 / 1       2.0e-7                      1.2e-7    0.25
  mean_vfe_kernel P 5 (P 1: exact)                      1.5e-7                      1.1e-7    0.25
  SECOND under mode 3, `3_scenes_clustered`: max |error| 5.4e-7 at max |ref| 1.13 = 0.03 of the rtol 1e-4 / atol 1e-5 bar
  six out-of-grid voxels, train mode: output moved by 5.7e-2 (max |output| 4.6) before SECOND.forward dropped them, 0 after
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_reference as R

pytestmark = pytest.mark.gpu

GUARD = 256
U22 = 2.0 ** -22
GRIDS = [((5, 7, 6), 2), ((6, 1, 9), 6), ((41, 8, 8), 2)]         # (D, H, W), B: odd / even / 1-wide axes; B = 6 so that 6x1x9 holds 257 sites
SUBM = [(3, 3, 3), (3, 1, 1), (1, 1, 1)]
STRIDED = [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))]
SIZES = [1, 255, 256, 257]


def _dev():
    return torch.device("cuda:0")


def _call(name, *args):
    from gencomm_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def _size(name, *args):
    from gencomm_amd import _lib
    return _lib.check_size(getattr(_lib.lib(), name)(*args), name)


def _st():
    from gencomm_amd.runtime import stream_ptr
    return stream_ptr(_dev())


def _p(t):
    return 0 if t is None or t.numel() == 0 else t.data_ptr()


def _i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(dtype).to(_dev())


class Guarded:
    """A device buffer of exactly `shape` elements between two guard bands, pre-filled with a sentinel."""

    def __init__(self, shape, dtype=torch.float32, fill=float("nan"), band=77):
        self.numel = int(np.prod(shape)) if len(shape) else 1
        self.band = band
        self.buf = torch.full((self.numel + 2 * GUARD,), band, dtype=dtype, device=_dev())
        self.t = self.buf[GUARD:GUARD + self.numel].view(*shape)
        self.t.fill_(fill)

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == self.band).all()) and bool((self.buf[GUARD + self.numel:] == self.band).all()), "write outside the buffer"
        return self.t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- entry points
def gpu_index(coords, B, dims):
    n = len(coords)
    c = _t(np.asarray(coords, dtype=np.int32).reshape(n, 4), torch.int32)
    keys, perm = Guarded((n,), torch.int64, fill=-5), Guarded((n,), torch.int32, fill=-5)
    ws = torch.empty(max(_size("gencomm_sp_index_workspace_bytes", n), 1), dtype=torch.uint8, device=_dev())
    _call("gencomm_sp_index_fwd", _p(c), n, B, _i3(dims), _p(keys.t), _p(perm.t), _p(ws), ws.numel(), _st())
    return keys.get(), perm.get()


def gpu_rules(out_keys, in_keys, B, dims_in, kernel, stride, pad):
    K, n_out = R.prod3(kernel), len(out_keys)
    ok, ik = _t(out_keys, torch.int64), _t(in_keys, torch.int64)
    nbr = Guarded((K, n_out), torch.int32, fill=-7)
    _call("gencomm_sp_rules_fwd", _p(ok), n_out, _p(ik), len(in_keys), B, _i3(dims_in), _i3(kernel), _i3(stride), _i3(pad), _p(nbr.t), _st())
    return nbr.get()


def gpu_rules_inv(in_keys, out_keys, B, dims_in, kernel, stride, pad):
    K, n_in = R.prod3(kernel), len(in_keys)
    ok, ik = _t(out_keys, torch.int64), _t(in_keys, torch.int64)
    inv = Guarded((K, n_in), torch.int32, fill=-7)
    _call("gencomm_sp_rules_inv_fwd", _p(ik), n_in, _p(ok), len(out_keys), B, _i3(dims_in), _i3(kernel), _i3(stride), _i3(pad), _p(inv.t), _st())
    return inv.get()


def gpu_sites(in_keys, B, dims_in, kernel, stride, pad):
    """-> (out keys [count], count, capacity)"""
    n_in = len(in_keys)
    cap = _size("gencomm_sp_sites_capacity", n_in, _i3(kernel), _i3(stride))
    ik = _t(in_keys, torch.int64)
    keys, count = Guarded((max(cap, 1),), torch.int64, fill=-5), Guarded((1,), torch.int32, fill=-5)
    ws = torch.empty(max(_size("gencomm_sp_sites_workspace_bytes", n_in, _i3(kernel), _i3(stride)), 1), dtype=torch.uint8, device=_dev())
    _call("gencomm_sp_sites_fwd", _p(ik), n_in, B, _i3(dims_in), _i3(kernel), _i3(stride), _i3(pad), _p(keys.t), _p(count.t), _p(ws), ws.numel(), _st())
    n = int(count.get()[0])
    assert 0 <= n <= cap, (n, cap)
    return keys.get()[:n].copy(), n, cap


def gpu_conv(x, nbr, w_raw, cin, cout, layout, scale, shift, relu):
    K, n_out = nbr.shape
    xd, nd, wd = _t(x, torch.float32), _t(nbr, torch.int32), _t(w_raw, torch.float32)
    prep = Guarded((_size("gencomm_sp_prepared_floats", K, cin, cout),))
    _call("gencomm_sp_prepare", _p(wd), _p(prep.t), K, cin, cout, layout, _st())
    prep.get()
    y, sc, sf = Guarded((n_out, cout)), _t(scale, torch.float32), _t(shift, torch.float32)
    _call("gencomm_sp_conv_fwd", _p(xd), _p(nd), _p(prep.t), _p(sc), _p(sf), _p(y.t), n_out, K, cin, cout, int(relu), _st())
    return y.get()


def gpu_wgrad(x, dy, nbr, dw0):
    K, n_out = nbr.shape
    cin, cout = x.shape[1], dy.shape[1]
    dw = Guarded((cout, K, cin))
    dw.t.copy_(_t(dw0, torch.float32))
    xd, yd, nd = _t(x, torch.float32), _t(dy, torch.float32), _t(nbr, torch.int32)
    _call("gencomm_sp_wgrad", _p(xd), _p(yd), _p(nd), _p(dw.t), n_out, K, cin, cout, _st())
    return dw.get()


# ------------------------------------------------------------------------------------------------------------- scenes
def _scene(dims, B, seed, fill=0.5):
    """Sorted keys of: every corner and face centre of the first and last sample, the pairs (y, W-1) / (y+1, 0), (z, H-1, W-1) /
    (z+1, 0, 0) and (b, D-1, H-1, W-1) / (b+1, 0, 0, 0) that are adjacent in key space only, and a random fill."""
    D, H, W = dims
    rng = np.random.RandomState(seed)
    cells = set()
    for b in {0, B - 1}:
        for z in (0, D // 2, D - 1):
            for y in (0, H // 2, H - 1):
                for x in (0, W // 2, W - 1):
                    if (z in (0, D - 1)) + (y in (0, H - 1)) + (x in (0, W - 1)) >= 1:
                        cells.add((b, z, y, x))
    z1 = min(1, D - 1)
    cells |= {(0, z1, H - 1, W - 1), (0, min(z1 + 1, D - 1), 0, 0), (0, D - 1, H - 1, W - 1), (1, 0, 0, 0)}
    if H > 1:
        cells |= {(0, z1, H // 2 - 1 if H > 2 else 0, W - 1), (0, z1, H // 2 if H > 2 else 1, 0)}
    total = B * D * H * W
    for k in rng.permutation(total)[:int(fill * total)]:
        cells.add(R.decode(int(k), dims))
    return np.array(sorted(R.encode(*c, dims) for c in cells), dtype=np.int64)


def _subset(keys, n, rng):
    return np.sort(keys[rng.permutation(len(keys))[:n]])


# ------------------------------------------------------------------------------------------------------------- index builders
@pytest.mark.parametrize("n", [0, 1, 257])
def test_index_keys_ascending_perm_and_out_of_grid_rows(n):
    dims, B = (5, 7, 6), 3
    rng = np.random.RandomState(n)
    cells = [k for k in rng.permutation(B * 5 * 7 * 6) if R.decode(int(k), dims)[0] != 1]       # sample 1 of 3 stays empty
    coords = np.array([R.decode(int(k), dims) for k in cells[:n]], dtype=np.int32).reshape(-1, 4)
    if n == 257:   # out-of-grid rows in between: a negative coordinate, a coordinate equal to its dim, b >= B, b < 0
        bad = np.array([[0, -1, 0, 0], [0, 0, 7, 0], [2, 0, 0, 6], [3, 0, 0, 0], [-1, 1, 1, 1], [0, 5, 0, 0], [0, 0, 0, -1]], dtype=np.int32)
        coords[rng.permutation(n)[:len(bad)]] = bad
    keys, perm = gpu_index(coords, B, dims)
    want_keys, want_perm = R.index(coords, B, dims)
    assert np.array_equal(keys, want_keys) and np.array_equal(perm, want_perm)
    if n == 257:
        assert int((keys == R.NO_KEY).sum()) == 7 and (keys[-7:] == R.NO_KEY).all() and (np.diff(keys[:-7]) > 0).all()
    if n == 1:     # a single out-of-grid row
        keys, perm = gpu_index([[0, 5, 0, 0]], B, dims)
        assert keys.tolist() == [R.NO_KEY] and perm.tolist() == [0]


@pytest.mark.parametrize("dims,B", GRIDS, ids=str)
@pytest.mark.parametrize("kernel", SUBM, ids=str)
def test_rules_submanifold(dims, B, kernel):
    rng = np.random.RandomState(11)
    scene = _scene(dims, B, seed=1, fill=0.85)
    ran = []
    for n in [None] + SIZES:
        keys = scene if n is None else _subset(scene, n, rng)
        assert n is None or len(keys) == n
        got = gpu_rules(keys, keys, B, dims, kernel, (1, 1, 1), tuple(k // 2 for k in kernel))
        assert np.array_equal(got, R.subm_rules(keys, dims, kernel)), (dims, kernel, n)
        assert np.array_equal(got[R.prod3(kernel) // 2], np.arange(len(keys)))             # the centre tap is the site itself
        ran.append(len(keys))
    # rows without a key (out-of-grid voxels sort last) read nothing and are read by nothing
    keys = np.concatenate([_subset(scene, 60, rng), [R.NO_KEY] * 4])
    got = gpu_rules(keys, keys, B, dims, kernel, (1, 1, 1), tuple(k // 2 for k in kernel))
    assert np.array_equal(got, R.subm_rules(keys, dims, kernel)) and (got[:, 60:] == -1).all() and (got < 60).all()
    print(f"sp_rules_kernel SubM {kernel} on {dims} x {B}: n_out {ran} exact")


@pytest.mark.parametrize("dims,B", GRIDS, ids=str)
@pytest.mark.parametrize("geo", STRIDED, ids=str)
def test_rules_sites_and_inverse_rules_strided(dims, B, geo):
    kernel, stride, pad = geo
    rng = np.random.RandomState(12)
    K = R.prod3(kernel)
    od = R.out_dims(dims, kernel, stride, pad)
    ran = []
    for fill in (0.5, 0.04):
        scene = _scene(dims, B, seed=2, fill=fill)
        got_keys, count, cap = gpu_sites(scene, B, dims, kernel, stride, pad)
        want_keys = R.sites(scene, dims, kernel, stride, pad)
        assert count == len(want_keys) and np.array_equal(got_keys, want_keys) and (np.diff(got_keys) > 0).all(), (dims, geo, fill, count, len(want_keys))
        sizes = [None] + [n for n in SIZES if n <= len(want_keys)]
        assert dims != (41, 8, 8) or fill != 0.5 or sizes == [None] + SIZES
        for n in sizes:
            ok = want_keys if n is None else _subset(want_keys, n, rng)
            nbr = gpu_rules(ok, scene, B, dims, kernel, stride, pad)
            assert np.array_equal(nbr, R.rules(ok, od, scene, dims, kernel, stride, pad)), (dims, geo, fill, n)
            inv = gpu_rules_inv(scene, ok, B, dims, kernel, stride, pad)
            assert np.array_equal(inv, R.rules_inv(scene, dims, ok, od, kernel, stride, pad)), (dims, geo, fill, n)
            # inv[o][i] == j exactly when nbr[o][j] == i, on the kernels' own results
            o_, j_ = np.nonzero(nbr >= 0)
            assert (inv[o_, nbr[o_, j_]] == j_).all() and int((inv >= 0).sum()) == len(o_)
            ran.append((len(ok), int(((inv >= 0).sum(0) == 0).sum())))
    assert any(unread > 0 for _, unread in ran)                                              # input sites that no output reads
    print(f"sp_candidates / sp_rules / sp_rules_inv {geo} on {dims} x {B} -> {od}: (n_out, unread inputs) {ran} exact; sites <= capacity {cap}")


def test_sites_truncated_layer_empty_output_and_empty_input():
    """D = 6, kernel (3, 1, 1), stride 2, pad 0: (6 - 3) % 2 != 0, the plane z = 5 lies in no receptive field."""
    dims, B = (6, 3, 4), 2
    geo = ((3, 1, 1), (2, 1, 1), (0, 0, 0))
    assert R.out_dims(dims, *geo) == [2, 3, 4]
    scene = _scene(dims, B, seed=3, fill=0.6)
    z = np.array([R.decode(k, dims)[1] for k in scene])
    assert (z == 5).sum() > 10
    keys, count, _ = gpu_sites(scene, B, dims, *geo)
    assert np.array_equal(keys, R.sites(scene, dims, *geo))
    only5 = scene[z == 5]
    without5 = gpu_sites(scene[z != 5], B, dims, *geo)[0]
    assert np.array_equal(keys, without5)                                                    # sites at z = 5 produce nothing
    keys0, count0, cap0 = gpu_sites(only5, B, dims, *geo)
    assert count0 == 0 and len(keys0) == 0 and cap0 == 2 * len(only5)
    # an empty output set: the rulebook and the convolution with n_out = 0 return OK and write nothing
    assert gpu_rules(keys0, only5, B, dims, *geo).shape == (3, 0)
    assert gpu_rules_inv(only5, keys0, B, dims, *geo).tolist() == [[-1] * len(only5)] * 3
    y = gpu_conv(np.ones((len(only5), 16), np.float32), np.zeros((3, 0), np.int32), np.ones((32, 3, 16), np.float32), 16, 32, 0, np.ones(32), np.ones(32), 1)
    assert y.shape == (0, 32)
    # no input site at all
    empty = np.zeros(0, dtype=np.int64)
    k_, c_, cap_ = gpu_sites(empty, B, dims, *geo)
    assert c_ == 0 and cap_ == 0
    assert gpu_rules_inv(empty, empty, B, dims, *geo).shape == (3, 0)
    # rows without a key produce no candidate
    k_, c_, _ = gpu_sites(np.concatenate([scene, [R.NO_KEY] * 3]), B, dims, *geo)
    assert np.array_equal(k_, keys)


# ------------------------------------------------------------------------------------------------------------- gather-GEMM
def _raw_weight(rng, K, cin, cout, layout):
    shape = {0: (cout, K, cin), 1: (K, cin, cout), 2: (cin, K, cout), 3: (cin, K, cout)}[layout]
    return (rng.standard_normal(shape) * np.sqrt(2.0 / (cin * max(K, 2) / 2))).astype(np.float32)


def _rulebook(rng, K, n_out, n_in, p_none=0.4):
    nbr = rng.randint(0, n_in, size=(K, n_out)).astype(np.int32)
    nbr[rng.random_sample((K, n_out)) < p_none] = -1
    return nbr


def _scale_shift(rng, cout):
    return ((rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32), rng.standard_normal(cout).astype(np.float32))


class Pool:
    """worst |got - ref64| / S of the kernel and of the float32 evaluation over the runs of one test"""

    def __init__(self):
        self.worst, self.r32, self.runs = 0.0, 0.0, 0

    def conv(self, x, nbr, w_raw, cin, cout, layout, scale, shift, relu, tile_max=None):
        K = nbr.shape[0]
        got = gpu_conv(x, nbr, w_raw, cin, cout, layout, scale, shift, relu)
        weff = R.effective_weight(w_raw, K, cin, cout, layout)
        ref = R.gather_gemm(x, nbr, weff, scale, shift, relu)
        y32 = R.gather_gemm(x, nbr, weff.astype(np.float32), scale, shift, relu, dtype=np.float32)
        mag = R.gather_gemm_magnitude(x, nbr, weff, scale, shift, tile_max)
        self.worst = max(self.worst, R.worst_ratio(got, ref, mag))
        self.r32 = max(self.r32, R.worst_ratio(y32, ref, mag))
        self.runs += 1
        return got, ref

    def wgrad(self, x, dy, nbr, dw0):
        got = gpu_wgrad(x, dy, nbr, dw0)
        ref = R.wgrad(x, dy, nbr, dw0)
        mag = R.wgrad_magnitude(x, dy, nbr, dw0)
        self.worst = max(self.worst, R.worst_ratio(got, ref, mag))
        self.r32 = max(self.r32, R.worst_ratio(R.wgrad(x, dy, nbr, dw0, dtype=np.float32), ref, mag))
        self.runs += 1
        return got, ref

    def check(self, what, extra=0.0):
        bound = 4 * self.r32 + extra
        print(f"{what}: {self.runs} runs, worst ratio {self.worst:.3e}, r32 {self.r32:.3e}, bound {bound:.3e}")
        assert self.worst <= bound, (what, self.worst, self.r32, bound)


def _cin_padded(cin):
    return 4 if cin <= 4 else 16 if cin <= 16 else 32 if cin <= 32 else 64


@pytest.mark.parametrize("cin,cout", [(4, 16), (3, 16), (16, 4), (16, 32), (20, 48), (32, 64), (64, 64), (64, 128)])
@pytest.mark.parametrize("K", [27, 3, 1])
def test_conv_exact_fp32(cin, cout, K):
    from gencomm_amd import _lib
    rng = np.random.RandomState(cin * 131 + cout * 7 + K)
    pool = Pool()
    with _lib.kernel_log() as kl:
        for n_out in (1, 63, 64, 65, 257):
            for relu in (0, 1):
                n_in = 50
                x = rng.standard_normal((n_in, cin)).astype(np.float32)
                scale, shift = _scale_shift(rng, cout)
                pool.conv(x, _rulebook(rng, K, n_out, n_in), _raw_weight(rng, K, cin, cout, 0), cin, cout, 0, scale, shift, relu)
    assert kl.counts == {f"sp_conv_kernel<{_cin_padded(cin)}>": pool.runs}, kl.counts
    pool.check(f"sp_conv_kernel<{_cin_padded(cin)}> Cin {cin} Cout {cout} K {K}")


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("cin,cout,K", [(16, 4, 27), (20, 48, 27), (64, 64, 27), (32, 64, 3), (3, 16, 3)])
def test_conv_prepare_layouts(layout, cin, cout, K):
    """Layout 0: spconv 2.x [Cout][K][Cin]; 1: spconv 1.x [K][Cin][Cout]; 2 / 3: the input gradient of a forward weight (channels swapped;
    3 mirrors the offsets). The rulebook is asymmetric in the offsets, so a missing or a doubled mirror shows."""
    rng = np.random.RandomState(layout * 1000 + cin + cout + K)
    pool = Pool()
    n_in, n_out = 70, 65
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    scale, shift = _scale_shift(rng, cout)
    w = _raw_weight(rng, K, cin, cout, layout)
    pool.conv(x, _rulebook(rng, K, n_out, n_in), w, cin, cout, layout, scale, shift, 0)
    if layout in (2, 3) and cin != cout:   # the transform differs from the forward one by more than rounding
        assert not np.array_equal(R.effective_weight(w, K, cin, cout, layout), R.effective_weight(w.reshape(-1), K, cin, cout, 0))
    pool.check(f"sp_prep_w_kernel layout {layout} Cin {cin} Cout {cout} K {K}")


@pytest.mark.parametrize("cin,cout", [(16, 32), (64, 64)])
def test_conv_dead_tile_and_last_offset_only(cin, cout, modes):
    """A 64-site tile whose rulebook is all -1 writes act(shift), next to live tiles; rows whose only neighbour sits at offset 26."""
    from gencomm_amd import _lib
    rng = np.random.RandomState(cin + cout)
    K, n_in, n_out = 27, 40, 3 * 64 + 5
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = _raw_weight(rng, K, cin, cout, 0)
    for arith in ("split", "split2"):
        if arith == "split2" and cin not in (32, 64):
            continue
        modes(arith=arith)
        pool = Pool()
        for relu in (0, 1):
            scale, shift = _scale_shift(rng, cout)
            nbr = _rulebook(rng, K, n_out, n_in)
            nbr[:, 64:128] = -1                      # dead tile between two live ones
            nbr[:, 128:192] = -1                     # a tile that lives through offset 26 alone, on its even rows
            nbr[26, 128:192:2] = rng.randint(0, n_in, size=32)
            with _lib.kernel_log() as kl:
                got, ref = pool.conv(x, nbr, w, cin, cout, 0, scale, shift, relu)
            assert list(kl.counts) == [f"sp_conv_f16s_kernel<{cin}>" if arith == "split2" else f"sp_conv_kernel<{_cin_padded(cin)}>"]
            act = np.maximum(shift, 0) if relu else shift
            assert np.array_equal(got[64:128], np.broadcast_to(act, (64, cout)))
            assert np.array_equal(got[129:192:2], np.broadcast_to(act, (32, cout)))
            assert not np.array_equal(got[128:192:2], np.broadcast_to(act, (32, cout)))
        pool.check(f"dead tile / offset 26 only, Cin {cin} Cout {cout}, {arith}", extra=4 * U22 if arith == "split2" else 0.0)


SPLIT_CASES = ["unit", "tiny", "huge", "zero_first_offsets", "late_outlier"]


def _split_inputs(rng, case, K, n_out, n_in, cin):
    """-> (x, nbr, tile_max)"""
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    nbr = _rulebook(rng, K, n_out, n_in)
    if case == "tiny":
        x *= np.float32(1e-6)
    elif case == "huge":
        x *= np.float32(1e5)
    elif case == "zero_first_offsets":              # offsets are visited in ascending order: the first third gathers all-zero rows only
        x[:10] = 0.0
        first = nbr[:K // 3]
        first[first >= 0] %= 10
        later = nbr[K // 3:]
        later[(later >= 0) & (later < 10)] += 10
    elif case == "late_outlier":                    # one row 1e4 larger than the rest, reachable only through the LAST visited offset
        x[n_in - 1] *= np.float32(1e4)
        nbr[nbr == n_in - 1] = n_in - 2
        nbr[K - 1, 5 % n_out::64] = n_in - 1        # once per 64-site tile: the scale drops after everything else is accumulated
        return x, nbr, 64
    return x, nbr, None


@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("cout", [32, 64, 128])
@pytest.mark.parametrize("case", SPLIT_CASES)
def test_conv_split2(cin, cout, case, modes):
    from gencomm_amd import _lib
    rng = np.random.RandomState(cin * 3 + cout + len(case))
    modes(arith="split2")
    pool = Pool()
    with _lib.kernel_log() as kl:
        for K in (27, 3, 1):
            for n_out in (1, 63, 64, 65, 257):
                x, nbr, tile_max = _split_inputs(rng, case, K, n_out, 50, cin)
                scale, shift = _scale_shift(rng, cout)
                if case in ("tiny", "huge"):        # the shift at the scale of the sums, so that S measures them and not the shift
                    shift = (shift * np.float32(1e-6 if case == "tiny" else 1e5)).astype(np.float32)
                pool.conv(x, nbr, _raw_weight(rng, K, cin, cout, 0), cin, cout, 0, scale, shift, (K + n_out) & 1, tile_max)
    assert kl.counts == {f"sp_conv_f16s_kernel<{cin}>": pool.runs}, kl.counts
    pool.check(f"sp_conv_f16s_kernel<{cin}> Cout {cout} {case}", extra=4 * U22)


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 128)])
def test_conv_split2_all_zero_input_gives_exactly_act_of_shift(cin, cout, modes):
    from gencomm_amd import _lib
    rng = np.random.RandomState(5)
    modes(arith="split2")
    for relu in (0, 1):
        scale, shift = _scale_shift(rng, cout)
        with _lib.kernel_log() as kl:
            got = gpu_conv(np.zeros((30, cin), np.float32), _rulebook(rng, 27, 130, 30), _raw_weight(rng, 27, cin, cout, 0), cin, cout, 0, scale, shift, relu)
        assert list(kl.counts) == [f"sp_conv_f16s_kernel<{cin}>"]
        assert np.array_equal(got, np.broadcast_to(np.maximum(shift, 0) if relu else shift, got.shape))


# ------------------------------------------------------------------------------------------------------------- weight gradient
def _rows_per_block(n_out, K):
    """the host's rule: the largest of 1024 .. 64 with ceil(n_out / rows) * K >= 512"""
    rows = 1024
    while rows > 64 and -(-n_out // rows) * K < 512:
        rows >>= 1
    return rows


@pytest.mark.parametrize("n_out,rows", [(1, 64), (65, 64), (550, 64), (2500, 128), (4700, 256), (9300, 512), (19000, 1024)])
def test_wgrad_every_rows_per_block(n_out, rows):
    K, cin, cout, n_in = 27, 64, 64, 300
    assert _rows_per_block(n_out, K) == rows and n_out % 64 != 0 and n_out % rows != 0          # a ragged last chunk in a ragged last block
    rng = np.random.RandomState(n_out)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    dy = rng.standard_normal((n_out, cout)).astype(np.float32)
    nbr = _rulebook(rng, K, n_out, n_in)
    nbr[7] = -1                                       # an offset no site uses: its slice of dw keeps the pre-filled value
    nbr[:, 3::17] = -1                                # sites without any neighbour
    dw0 = rng.standard_normal((cout, K, cin)).astype(np.float32)
    pool = Pool()
    got, _ = pool.wgrad(x, dy, nbr, dw0)
    assert np.array_equal(got[:, 7, :], dw0[:, 7, :])
    pool.check(f"sp_wgrad_kernel n_out {n_out} (rows_per_block {rows})")


@pytest.mark.parametrize("cin,cout", [(4, 16), (16, 32), (64, 64)])
@pytest.mark.parametrize("K", [3, 1])
def test_wgrad_small_shapes(cin, cout, K):
    rng = np.random.RandomState(cin + cout + K)
    pool = Pool()
    for n_out in (1, 65, 700, 2500):
        n_in = 90
        x = rng.standard_normal((n_in, cin)).astype(np.float32)
        dy = rng.standard_normal((n_out, cout)).astype(np.float32)
        nbr = _rulebook(rng, K, n_out, n_in)
        if K == 3:
            nbr[1] = -1
        dw0 = rng.standard_normal((cout, K, cin)).astype(np.float32)
        got, _ = pool.wgrad(x, dy, nbr, dw0)
        if K == 3:
            assert np.array_equal(got[:, 1, :], dw0[:, 1, :])
    pool.check(f"sp_wgrad_kernel Cin {cin} Cout {cout} K {K} (rows_per_block {[_rows_per_block(n, K) for n in (1, 65, 700, 2500)]})")


# ------------------------------------------------------------------------------------------------------------- MeanVFE, dense
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("F", [4, 5])
@pytest.mark.parametrize("with_perm", [False, True])
def test_mean_vfe(P, F, with_perm):
    rng = np.random.RandomState(P * 10 + F)
    n = 300
    v = rng.standard_normal((n, P, F)).astype(np.float32)
    num = rng.randint(0, P + 1, size=n).astype(np.int32)
    num[:3] = 0                                       # an empty voxel divides by 1
    perm = rng.permutation(n).astype(np.int32) if with_perm else None
    out = Guarded((n, F))
    vd, nd, pd = _t(v, torch.float32), _t(num, torch.int32), _t(perm, torch.int32) if with_perm else None
    _call("gencomm_mean_vfe_fwd", _p(vd), _p(nd), _p(pd), _p(out.t), n, P, F, _st())
    got = out.get()
    ref = R.mean_vfe(v, num, perm)
    mag = R.mean_vfe(np.abs(v), num, perm)
    worst = R.worst_ratio(got, ref, mag)
    r32 = R.worst_ratio((v.sum(1, dtype=np.float32) / np.maximum(num.astype(np.float32), np.float32(1))[:, None])[perm if with_perm else slice(None)], ref, mag)
    print(f"mean_vfe_kernel P {P} F {F} perm {with_perm}: worst ratio {worst:.3e}, r32 {r32:.3e}")
    assert worst <= 4 * r32                           # P = 1: both are exact (the sum has one term, the divisor is 1)


@pytest.mark.parametrize("C_", [16, 128])
def test_dense_scatter_and_its_gradient(C_):
    from gencomm_amd.second import SparseTensor
    dims, B = (3, 5, 6), 2
    rng = np.random.RandomState(C_)
    keys = np.concatenate([_subset(_scene(dims, B, seed=4, fill=0.4), 50, rng), [R.NO_KEY] * 3])
    feat = rng.standard_normal((len(keys), C_)).astype(np.float32)
    out = Guarded((B, C_, *dims))
    fd, kd = _t(feat, torch.float32), _t(keys, torch.int64)
    _call("gencomm_sp_dense_fwd", _p(fd), _p(kd), len(keys), C_, B, _i3(dims), _p(out.t), _st())
    want = R.dense(feat, keys, B, dims)
    got = out.get()
    assert np.array_equal(got, want)                  # a copy: bit-exact, inactive cells exactly 0, rows without a key skipped
    assert int((got != 0).sum()) == 50 * C_
    # SparseTensor.dense() with a gradient: the backward gathers the dense gradient at the active sites (rows without a key get 0)
    f = _t(feat, torch.float32).requires_grad_(True)
    sp = SparseTensor(_t(keys, torch.int64), f, B, list(dims))
    d = sp.dense()
    assert np.array_equal(d.detach().cpu().numpy(), want)
    g = torch.from_numpy(rng.standard_normal(want.shape).astype(np.float32))
    d.backward(g.to(_dev()))
    want_g = np.zeros_like(feat)
    for j, k in enumerate(keys[:50]):
        b, z, y, x = R.decode(k, dims)
        want_g[j] = g[b, :, z, y, x].numpy()
    assert np.array_equal(f.grad.cpu().numpy(), want_g)
    # n = 0: the volume is zeroed
    out0 = Guarded((B, C_, *dims))
    _call("gencomm_sp_dense_fwd", None, None, 0, C_, B, _i3(dims), _p(out0.t), _st())
    assert not out0.get().any()


# ------------------------------------------------------------------------------------------------------------- the module
def _second_inputs():
    """the `3_scenes_clustered` inputs of tests/test_second.py"""
    from test_second import _args, _module, _voxels
    nx, ny, counts = 48, 32, [300, 40, 1]
    net = _module(_args(nx, ny, cout=64), 5)
    vf, vc, vn = _voxels(np.random.RandomState(7), counts, nx, ny, 40, clustered=True)
    return net, vf, vc, vn, nx, ny


def _run_second(net, vf, vc, vn):
    return net({"inputs_m3": {"voxel_features": vf.cuda(), "voxel_coords": vc.cuda(), "voxel_num_points": vn.cuda()}}, "m3")


def test_second_encoder_under_split2_vs_float64_oracle(modes):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import second_port as S
    from gencomm_amd import _lib
    from helpers import assert_close
    net, vf, vc, vn, nx, ny = _second_inputs()
    sd = {k: (v.detach().double() if v.is_floating_point() else v.detach()) for k, v in net.state_dict().items()}
    ref = S.second_forward(sd, "", vf.double(), vc, vn, [nx, ny, 40]).numpy()
    net = net.cuda()
    modes(arith="split2")
    with torch.no_grad(), _lib.kernel_log() as kl:
        out = _run_second(net, vf, vc, vn).cpu().numpy()
    # 12 layers: conv_input (Cin 4) and conv1 / conv2.0 (Cin 16) stay on the exact kernel, the nine Cin 32 / 64 layers take the split one
    assert {k: v for k, v in kl.counts.items() if k.startswith("sp_conv")} == \
        {"sp_conv_kernel<4>": 1, "sp_conv_kernel<16>": 2, "sp_conv_f16s_kernel<32>": 3, "sp_conv_f16s_kernel<64>": 6}, kl.counts
    err = np.abs(out - ref)
    print(f"SECOND under split2 vs float64 oracle: max |err| {err.max():.3e}, max |ref| {np.abs(ref).max():.3f}, "
          f"worst err / (1e-5 + 1e-4 |ref|) {float((err / (1e-5 + 1e-4 * np.abs(ref))).max()):.3f}")
    assert float(np.abs(ref).max()) > 0.05
    assert_close(out, ref, 1e-4, 1e-5, "SECOND spatial_features under split2")


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_out_of_grid_voxels_change_nothing(train):
    """Voxels outside the grid (a negative coordinate, a coordinate equal to its dim) are dropped by the reference's dataloader; if
    they arrive all the same they change neither the output nor, in train mode, the BatchNorm running statistics."""
    net, vf, vc, vn, nx, ny = _second_inputs()
    net = net.cuda().train(train)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    bad = torch.tensor([[0, -1, 3, 3], [1, 41, 0, 0], [0, 5, ny, 2], [2, 7, 1, nx], [0, 3, -2, 4], [1, 0, 0, -1]], dtype=vc.dtype)
    rng = np.random.RandomState(8)
    vf2 = torch.cat([vf, torch.from_numpy(rng.standard_normal((len(bad), *vf.shape[1:])).astype(np.float32) + 3.0)])
    vc2, vn2 = torch.cat([vc, bad]), torch.cat([vn, torch.full((len(bad),), vf.shape[1], dtype=vn.dtype)])
    p = torch.from_numpy(rng.permutation(len(vc2)))                                           # the out-of-grid rows anywhere in the list
    with torch.no_grad():
        a = _run_second(net, vf, vc, vn)
        sa = {k: v.clone() for k, v in net.state_dict().items()}
        net.load_state_dict(state)
        b = _run_second(net, vf2[p], vc2[p], vn2[p])
        sb = {k: v.clone() for k, v in net.state_dict().items()}
    if train:
        assert any(not torch.equal(sa[k], state[k]) for k in sa if k.endswith("running_mean"))
    worst = max(float((sa[k].double() - sb[k].double()).abs().max()) for k in sa)
    print(f"SECOND with {len(bad)} out-of-grid voxels ({'train' if train else 'eval'}): max |output difference| {float((a - b).abs().max()):.3e}, "
          f"max |state difference| {worst:.3e}")
    if train:   # batch statistics are summed with float64 atomics in any order: the float32 statistics may move by an ulp (6e-8) from
        # run to run, a phantom all-zero row moves them by 1 / n_rows (3e-3)
        for k in sa:
            assert torch.allclose(sa[k].double(), sb[k].double(), rtol=1e-5, atol=1e-6), k
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    else:
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
        assert torch.equal(a, b)
