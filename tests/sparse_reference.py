"""Plain float64 reference of the sparse-convolution operations of csrc/sparse_kernels.h, written from COORDINATES (a Python dict
coord -> row), not from dense volumes: key encoding and ordering, SubM / strided rulebooks, strided output-site sets, the inverse
rulebook, the gather-GEMM, the weight transforms of the four prepare layouts, the weight gradient, MeanVFE and the dense scatter.
Nothing here is shared with the product or with oracle/second_port.py (tests/test_sparse_reference.py pins the two against each
other on small grids).

The gather-GEMM and the weight gradient also exist as a float32 evaluation (numpy float32, accumulated offset by offset; see
gather_gemm / wgrad for the order within an offset): it is the yardstick the GPU tests measure the kernels' rounding against, both
judged per element relative to the magnitude
S = |scale| sum |w| |x| + |shift|  (weight gradient: sum |x| |dy| + |pre-filled value|)."""
import numpy as np

NO_KEY = 0x7FFFFFFFFFFFFFFF   # out-of-grid rows: sorts after every real key


def prod3(k):
    return int(k[0]) * int(k[1]) * int(k[2])


def encode(b, z, y, x, dims):
    D, H, W = dims
    return ((int(b) * D + int(z)) * H + int(y)) * W + int(x)


def decode(key, dims):
    D, H, W = dims
    key = int(key)
    x = key % W; key //= W
    y = key % H; key //= H
    return key // D, key % D, y, x


def in_grid(b, z, y, x, B, dims):
    D, H, W = dims
    return 0 <= b < B and 0 <= z < D and 0 <= y < H and 0 <= x < W


def index(coords, B, dims):
    """coords [n][4] (b, z, y, x) -> (keys ascending int64 [n], perm int32 [n]: sorted row -> input row). Out-of-grid rows get
    NO_KEY; rows with equal keys keep their input order (stable)."""
    keys = [encode(*c, dims) if in_grid(*[int(v) for v in c], B, dims) else NO_KEY for c in np.asarray(coords).reshape(-1, 4)]
    order = sorted(range(len(keys)), key=lambda i: (keys[i], i))
    return np.array([keys[i] for i in order], dtype=np.int64), np.array(order, dtype=np.int32)


def out_dims(dims, kernel, stride, pad):
    return [(dims[j] + 2 * pad[j] - kernel[j]) // stride[j] + 1 for j in range(3)]


def site_table(keys, dims):
    """dict (b, z, y, x) -> row of the sorted key array (NO_KEY rows have no coordinate)."""
    return {decode(k, dims): j for j, k in enumerate(keys) if int(k) != NO_KEY}


def offsets(kernel):
    """kernel offsets in the order o = (kz * kH + ky) * kW + kx"""
    return [(kz, ky, kx) for kz in range(kernel[0]) for ky in range(kernel[1]) for kx in range(kernel[2])]


def rules(out_keys, dims_out, in_keys, dims_in, kernel, stride, pad):
    """nbr [K][n_out] int32: row of the input site out * stride - pad + offset, or -1"""
    table = site_table(in_keys, dims_in)
    nbr = np.full((prod3(kernel), len(out_keys)), -1, dtype=np.int32)
    for j, key in enumerate(out_keys):
        if int(key) == NO_KEY:
            continue
        b, z, y, x = decode(key, dims_out)
        for o, (kz, ky, kx) in enumerate(offsets(kernel)):
            c = (b, z * stride[0] - pad[0] + kz, y * stride[1] - pad[1] + ky, x * stride[2] - pad[2] + kx)
            nbr[o, j] = table.get(c, -1)     # a coordinate outside the grid is in no table: no wrap into the next row / plane / sample
    return nbr


def subm_rules(keys, dims, kernel):
    return rules(keys, dims, keys, dims, kernel, (1, 1, 1), tuple(k // 2 for k in kernel))


def sites(in_keys, dims_in, kernel, stride, pad):
    """ascending keys (on the output grid) of every output position whose receptive field holds an active input site"""
    od = out_dims(dims_in, kernel, stride, pad)
    found = set()
    for key in in_keys:
        if int(key) == NO_KEY:
            continue
        b, z, y, x = decode(key, dims_in)
        for kz, ky, kx in offsets(kernel):
            t = (z + pad[0] - kz, y + pad[1] - ky, x + pad[2] - kx)
            if all(t[a] >= 0 and t[a] % stride[a] == 0 and t[a] // stride[a] < od[a] for a in range(3)):
                found.add(encode(b, t[0] // stride[0], t[1] // stride[1], t[2] // stride[2], od))
    return np.array(sorted(found), dtype=np.int64)


def rules_inv(in_keys, dims_in, out_keys, dims_out, kernel, stride, pad):
    """inv [K][n_in]: the output row that reads input row i through offset o, or -1 (defined from the forward rulebook)"""
    nbr = rules(out_keys, dims_out, in_keys, dims_in, kernel, stride, pad)
    inv = np.full((prod3(kernel), len(in_keys)), -1, dtype=np.int32)
    for o in range(nbr.shape[0]):
        for j in range(nbr.shape[1]):
            if nbr[o, j] >= 0:
                assert inv[o, nbr[o, j]] == -1      # one output position per (input site, offset)
                inv[o, nbr[o, j]] = j
    return inv


def effective_weight(w, K, cin, cout, layout):
    """raw weight as gencomm_sp_prepare reads it -> Weff [K][cout][cin] float64 with y[j][co] = sum_o sum_ci Weff[o][co][ci] x[nbr[o][j]][ci].
    0: spconv 2.x [cout][K][cin].  1: spconv 1.x [K][cin][cout].  2 / 3: the input gradient of a layout-0 forward weight
    [cin][K][cout] (the forward layer's Cout is this convolution's cin): channels swapped; 3 also mirrors the offsets."""
    w = np.asarray(w, dtype=np.float64)
    if layout == 0:
        return w.reshape(cout, K, cin).transpose(1, 0, 2).copy()
    if layout == 1:
        return w.reshape(K, cin, cout).transpose(0, 2, 1).copy()
    t = w.reshape(cin, K, cout).transpose(1, 2, 0)
    return (t[::-1] if layout == 3 else t).copy()


def _gathered(x, nbr_o):
    g = np.zeros((len(nbr_o), x.shape[1]), dtype=x.dtype)
    live = nbr_o >= 0
    g[live] = x[nbr_o[live]]
    return g


def gather_gemm(x, nbr, weff, scale, shift, relu, dtype=np.float64):
    """y[j] = act(scale * sum_o W_o x[nbr[o][j]] + shift) in `dtype`. float32 is the PLAIN evaluation: offset by offset and, within
    an offset, channel by channel, every product rounded to float32 and added to one float32 running sum per output element. (Not a
    BLAS product: sgemm keeps several partial sums per element and fuses multiply and add, so over the 1728 terms of a 27 x 64 sum
    its error is a fifth of a running sum's -- Cin = Cout = 64, K = 27: sgemm 3.7e-8 of S, this running sum 1.9e-7, the exact-fp32
    MFMA kernel on MI355X 1.8e-7 -- and '4 x' of it no longer means 'another summation order of the same arithmetic', which is
    what the factor stands for.)"""
    x, weff = np.asarray(x, dtype=dtype), np.asarray(weff, dtype=dtype)
    acc = np.zeros((nbr.shape[1], weff.shape[1]), dtype=dtype)
    for o in range(nbr.shape[0]):
        if (nbr[o] >= 0).any():
            g = _gathered(x, nbr[o])
            if dtype == np.float32:
                for ci in range(g.shape[1]):
                    acc += g[:, ci:ci + 1] * weff[o][:, ci][None, :]
            else:
                acc += g @ weff[o].T
    y = acc * np.asarray(scale, dtype=dtype) + np.asarray(shift, dtype=dtype)
    return np.maximum(y, 0) if relu else y


def gather_gemm_magnitude(x, nbr, weff, scale, shift, tile_max=None):
    """S = |scale| sum |w| |x| + |shift| per output element (float64). With `tile_max` (rows per tile) every gathered |x| counts as
    the largest |x| that the tile of `tile_max` consecutive output rows gathers (the shared scale of sp_conv_f16s_kernel)."""
    ax, aw = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(weff, dtype=np.float64))
    n_out = nbr.shape[1]
    g = [_gathered(ax, nbr[o]) for o in range(nbr.shape[0])]
    if tile_max:
        for t0 in range(0, n_out, tile_max):
            big = max(float(go[t0:t0 + tile_max].max()) for go in g)
            for o, go in enumerate(g):
                go[t0:t0 + tile_max][nbr[o, t0:t0 + tile_max] >= 0] = big
    acc = np.zeros((n_out, aw.shape[1]))
    for o, go in enumerate(g):
        acc += go @ aw[o].T
    return acc * np.abs(np.asarray(scale, dtype=np.float64)) + np.abs(np.asarray(shift, dtype=np.float64))


def wgrad(x, dy, nbr, dw0, dtype=np.float64):
    """dW[co][o][ci] = dw0 + sum_j x[nbr[o][j]][ci] dy[j][co]   (raw layout 0, [cout][K][cin]); in float32 one float32 matrix product per
    offset (its blocked sums over up to 19 000 rows are a tighter yardstick than a single running sum would be)"""
    x, dy = np.asarray(x, dtype=dtype), np.asarray(dy, dtype=dtype)
    dw = np.array(dw0, dtype=dtype).reshape(dy.shape[1], nbr.shape[0], x.shape[1]).copy()
    for o in range(nbr.shape[0]):
        if (nbr[o] >= 0).any():
            dw[:, o, :] += dy.T @ _gathered(x, nbr[o])
    return dw


def wgrad_magnitude(x, dy, nbr, dw0):
    ax, ady = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(dy, dtype=np.float64))
    return wgrad(ax, ady, nbr, np.abs(np.asarray(dw0, dtype=np.float64)))


def mean_vfe(voxels, num_points, perm=None):
    """sum over ALL point slots / max(num_points, 1); row j of the output = voxel perm[j]"""
    v = np.asarray(voxels, dtype=np.float64)
    out = v.sum(1) / np.maximum(np.asarray(num_points, dtype=np.float64), 1.0)[:, None]
    return out if perm is None else out[np.asarray(perm)]


def dense(feat, keys, B, dims):
    """[B][C][D][H][W], zero where inactive; NO_KEY rows are skipped"""
    feat = np.asarray(feat)
    out = np.zeros((B, feat.shape[1], *dims), dtype=feat.dtype)
    for j, key in enumerate(keys):
        if int(key) != NO_KEY:
            b, z, y, x = decode(key, dims)
            out[b, :, z, y, x] = feat[j]
    return out


def worst_ratio(got, ref64, mag):
    """max |got - ref64| / S over the elements with S > 0; where S == 0 the result must be exactly the reference"""
    got, ref64, mag = (np.asarray(a, dtype=np.float64) for a in (got, ref64, mag))
    assert np.isfinite(got).all()
    zero = mag == 0
    assert np.array_equal(got[zero], ref64[zero])
    if zero.all():
        return 0.0
    return float((np.abs(got - ref64)[~zero] / mag[~zero]).max())
