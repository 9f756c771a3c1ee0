"""The detection-tail kernels (gencomm_amd/csrc/detect_kernels.h, iou3d_kernels.h, box_overlap.h) called directly through the C ABI with raw
pointers, the way gencomm_amd/postprocess.py calls them, against the independent references of tests/detect_reference.py (pinned on the CPU
by tests/test_detect_reference.py).

  quad IoU     gencomm_quad_iou_fwd (the NMS's own quad_iou_d) against exact rational arithmetic on ten families of car-sized boxes with
               centres out to +-140 m / +-40 m. Pass rule: |kernel - exact| <= max(4 r64, 1e-15) per family, r64 = the error of the same
               clipping algorithm in numpy float64 (oracle/detect_port.py) against exact on the same pairs; the factor 4 is for another
               summation order of the area sums. identical -> 1.0, shared edge / corner, disjoint, degenerate -> 0.0 exactly.
  rotated NMS  gencomm_nms_rotated_fwd on hand-built candidates against greedy NMS over the float64 vertex-enumeration IoU: out_index,
               out_count, out_scores exact, out_boxes rows bit-equal, rows beyond out_count untouched. Every input but the exact-threshold
               one has no pair whose decision moves within MARGIN = 100 x the quad-IoU bound (asserted before the GPU is touched).
  decode       gencomm_det_decode_fwd / gencomm_det_mc_decode_fwd / gencomm_det_mc_gather_fwd against float64 decoding of the same float32
               inputs: survivor set, order, anchor index, labels, counts exact; scores and corners within 4 r32, r32 = the error of the
               float32 torch restatement (oracle/detect_port.py) against float64 on a 16 x 32 x 6 map of the same coordinate range and
               transformation. No anchor of any map lies within 8 r32 of a selection boundary (asserted first); the anchors that sit on
               a boundary by construction (zero y extent, classes saturated to 1.0f, direction ties) are compared exactly.
  iou3d_nms, bbox_overlaps   degenerate families against the C oracle (tolerances of tests/test_iou3d_voxel.py) / bit-exact.

Measured on MI355X (worst |error|; see the printed line of each test):
  quad IoU family      n    r64       kernel    bound max(4 r64, 1e-15)
  random              200   2.23e-13  2.23e-13  8.9e-13
  mixed_orientation    30   2.93e-14  2.93e-14  1.2e-13
  containment          24   6.87e-15  6.87e-15  2.7e-14
  crosses              16   2.29e-13  2.29e-13  9.1e-13
  near_coincident      64   8.98e-14  8.98e-14  3.6e-13
  identical (28), identical_rolled (20), shared_edge_corner (36), disjoint (20): r64 0, kernel 0 (exactly 1.0 / 0.0)
  degenerate           60   1.76e-15  0         (before quad_iou_d returned 0 for a box without area: 1.76e-15 on rotated zero-width boxes)
  NMS margin = 100 x 9.1e-13 = 9.1e-11; no input has a pair inside it.
  decode                         r32 score  kernel    r32 corners  kernel    r32 unprojected  kernel
  |x| <= 40 m, single class      8.3e-8     8.5e-8    8.7e-6       7.6e-6
  |x| <= 140 m, single class     8.3e-8     8.7e-8    1.49e-5      1.53e-5
  |x| <= 40 m, multi-class       8.3e-8     8.2e-8    8.2e-6       7.4e-6    3.9e-6           5.3e-6
  |x| <= 140 m, multi-class      8.3e-8     8.6e-8    1.49e-5      1.51e-5   1.49e-5          1.51e-5
  (bound 4 r32 per quantity; the largest kernel / r32 ratio is 1.4, on the unprojected corners of the 17-agent call)
  Before the decode filters rejected non-finite corners, the NaN / infinity test kept 25 candidates where the reference keeps 18
  (fminf / fmaxf skip a NaN, so a box whose corners are all NaN had extents of -inf and passed), and counted 1 violation of 3.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import detect_reference as R

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = -777.0


def _dev():
    return torch.device("cuda:0")


def _lib():
    from gencomm_amd import _lib
    return _lib


def _call(name, *args):
    _lib().check(getattr(_lib().lib(), name)(*args), name)


def _size(name, *args):
    return _lib().check_size(getattr(_lib().lib(), name)(*args), name)


def _st():
    from gencomm_amd.runtime import stream_ptr
    return stream_ptr(_dev())


def _p(t):
    return 0 if t is None else t.data_ptr()


def _t(a, dtype=torch.float32):
    a = np.ascontiguousarray(np.asarray(a))
    if a.size == 0:
        return torch.zeros(1, dtype=dtype, device=_dev())   # a valid pointer that is never read
    return torch.from_numpy(a).to(dtype).to(_dev())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


class Guarded:
    """A device buffer of exactly `shape` elements between two guard bands, pre-filled with a sentinel."""

    def __init__(self, shape, dtype=torch.float32, fill=SENT, band=77):
        self.numel = int(np.prod(shape)) if len(shape) else 1
        self.band = band
        self.buf = torch.full((self.numel + 2 * GUARD,), band, dtype=dtype, device=_dev())
        self.t = self.buf[GUARD:GUARD + self.numel].view(*shape)
        self.t.fill_(fill)

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == self.band).all()) and bool((self.buf[GUARD + self.numel:] == self.band).all()), "write outside the buffer"
        return self.t.cpu().numpy()


def corners_of(quads, z0=-1.8, z1=-0.2):
    """[n, 4, 2] BEV quadrilaterals -> [n, 8, 3] float32 corners as the NMS takes them."""
    quads = np.asarray(quads, np.float32).reshape(-1, 4, 2)
    c = np.zeros((quads.shape[0], 8, 3), np.float32)
    c[:, :4, :2] = quads; c[:, 4:, :2] = quads
    c[:, :4, 2] = z0; c[:, 4:, 2] = z1
    return c


# ============================================================================================================== quad IoU
def gpu_quad_iou(A, B):
    ca, cb = corners_of(A), corners_of(B)
    out = Guarded((len(ca), len(cb)), torch.float64, fill=SENT)
    ta, tb = _t(ca), _t(cb)                     # named: a temporary's memory would be handed to the next allocation
    _call("gencomm_quad_iou_fwd", _p(ta), len(ca), _p(tb), len(cb), _p(out.t), _st())
    return out.get()


def quad_bound(name=None):
    yard = R.iou_yardsticks()
    if name is not None:
        return max(4 * yard[name][1], 1e-15)
    return max(max(4 * y[1], 1e-15) for y in yard.values())


def nms_margin():
    return 100 * quad_bound()


@pytest.mark.parametrize("name", ["random", "identical", "identical_rolled", "shared_edge_corner", "containment", "crosses",
                                  "near_coincident", "degenerate", "disjoint", "mixed_orientation"])
def test_quad_iou_against_exact(name):
    P, Q = R.iou_families()[name]
    _, r64, exact = R.iou_yardsticks()[name]
    got = np.diagonal(gpu_quad_iou(P, Q)).copy()          # pair k = (P[k], Q[k]); the off-diagonal pairs are the layout test's business
    assert np.isfinite(got).all()
    err = max(abs(Fraction(float(g)) - e) for g, e in zip(got, exact))
    bound = quad_bound(name)
    print(f"quad IoU {name}: n {len(got)}, r64 {r64:.2e}, kernel worst error {float(err):.2e}, bound {bound:.2e}")
    if name in R.EXACT_FAMILIES:
        assert (got == R.EXACT_FAMILIES[name]).all(), got[got != R.EXACT_FAMILIES[name]]
    assert err <= bound


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 5), (5, 3), (7, 37), (16, 16), (0, 5), (5, 0)])
def test_quad_iou_matrix_layout(na, nb):
    P, Q = R.iou_families()["random"]
    A, B = P[:na], np.concatenate([Q[:nb // 2], P[:nb - nb // 2]])        # row i overlaps columns i (its partner) and nb // 2 + i (itself)
    out = Guarded((max(na * nb, 1),), torch.float64, fill=SENT)
    ta, tb = _t(corners_of(A)), _t(corners_of(B))
    _call("gencomm_quad_iou_fwd", _p(ta) if na else 0, na, _p(tb) if nb else 0, nb, _p(out.t), _st())
    got = out.get()
    if na * nb == 0:
        assert (got == SENT).all()
        return
    got = got.reshape(na, nb)
    want = R.quad_iou_f64_batch(np.repeat(A, nb, 0), np.tile(B, (na, 1, 1))).reshape(na, nb)
    assert (want > 0).sum() >= min(na, nb - nb // 2)
    np.testing.assert_allclose(got, want, rtol=0, atol=quad_bound("random") + 1e-13)


# ============================================================================================================== rotated NMS
def gpu_nms(corners, scores, thr, top, range6=None, ws=None, n_dev=None):
    n = len(scores)
    c, s = _t(np.asarray(corners, np.float32).reshape(-1)), _t(np.asarray(scores, np.float32))
    ndev = torch.tensor([n if n_dev is None else n_dev], dtype=torch.int32, device=_dev())
    ob, osc = Guarded((top, 8, 3)), Guarded((top,))
    oi, oc = Guarded((top,), torch.int32, fill=-5), Guarded((1,), torch.int32, fill=-5)
    if ws is None:
        ws = torch.empty(_size("gencomm_nms_workspace_bytes"), dtype=torch.uint8, device=_dev())
    r6 = None if range6 is None else _t(np.asarray(range6, np.float32))
    _call("gencomm_nms_rotated_fwd", _p(c), _p(s), _p(ndev), float(np.float32(thr)), top, _p(r6), _p(ob.t), _p(osc.t), _p(oi.t), _p(oc.t),
          _p(ws), ws.numel(), _st())
    return dict(boxes=ob.get(), scores=osc.get(), index=oi.get(), count=int(oc.get()[0]))


def check_nms(corners, scores, thr, top, range6=None, expect=None, margin_free=True, **kw):
    corners, scores = np.asarray(corners, np.float32).reshape(-1, 8, 3), np.asarray(scores, np.float32)
    kept, undecided = R.nms_reference(corners, scores, thr, top, range6, margin=nms_margin())
    if margin_free:
        assert undecided == [], undecided[:5]                 # before the GPU is touched
    if expect is not None:
        assert kept.tolist() == list(expect)
    got = gpu_nms(corners, scores, thr, top, range6, **kw)
    m = len(kept)
    assert got["count"] == m, (got["count"], m)
    assert got["index"][:m].tolist() == kept.tolist()
    assert np.array_equal(_bits(got["scores"][:m]), _bits(scores[kept]))
    assert np.array_equal(_bits(got["boxes"][:m]), _bits(corners[kept]))
    assert (got["index"][m:] == -5).all() and (got["scores"][m:] == SENT).all() and (got["boxes"][m:] == SENT).all()
    return kept, got


@pytest.mark.parametrize("n,top", [(0, 1000), (1, 1000), (2, 1000), (63, 1000), (64, 1000), (65, 1000), (127, 1000), (128, 1000), (129, 1000),
                                   (999, 1000), (1000, 1000), (1001, 1000), (1023, 1024), (1024, 1024), (1025, 1024), (5, 1), (130, 64),
                                   (5000, 1000), (16384, 1000)])
def test_nms_sizes(n, top):
    corners, scores = R.cluster_scene(n, 100 + n)
    kept, _ = check_nms(corners, scores, 0.15, top)
    assert n < 3 or 0 < len(kept) <= min(n, top)
    if n >= 999:
        assert len(kept) < min(n, top)      # something was suppressed


def _row_scene(n, spacing=10.0):
    """n disjoint 4.5 x 2 boxes in a row, scores descending with the index (rank = index)."""
    quads = np.stack([R.bev_quad(spacing * i - 300.0, 7.0, 4.5, 2.0, 0.0) for i in range(n)])
    return corners_of(quads), (0.99 - 5e-4 * np.arange(n)).astype(np.float32)


@pytest.mark.parametrize("r", [62, 63, 64])
def test_nms_greedy_chain_across_mask_words(r):
    """Rank r suppresses r + 1 (IoU 5/13); r + 1 would suppress r + 2 but is gone; r and r + 2 overlap by 1/17 only: r + 2 is kept."""
    corners, scores = _row_scene(130)
    x0 = 10.0 * r - 300.0
    corners[r + 1] = corners_of(R.bev_quad(x0 + 2.0, 7.0, 4.5, 2.0, 0.0)[None])[0]
    corners[r + 2] = corners_of(R.bev_quad(x0 + 4.0, 7.0, 4.5, 2.0, 0.0)[None])[0]
    check_nms(corners, scores, 0.3, 1000, expect=[i for i in range(130) if i != r + 1])


def test_nms_rank_0_suppresses_rank_999_and_the_cut():
    corners, scores = _row_scene(1001, spacing=6.0)
    corners[999] = corners_of(R.bev_quad(-300.0 + 0.5, 7.0, 4.5, 2.0, 0.0)[None])[0]
    check_nms(corners, scores, 0.3, 1000, expect=list(range(999)))       # 999 suppressed by 0, 1000 beyond the cut


def test_nms_all_identical_and_all_disjoint():
    one = corners_of(R.bev_quad(120.0, -30.0, 4.5, 2.0, 0.7)[None])
    corners = np.repeat(one, 300, 0)
    scores = np.random.RandomState(3).permutation(np.linspace(0.3, 0.9, 300)).astype(np.float32)
    check_nms(corners, scores, 0.15, 1000, expect=[int(np.argmax(scores))])
    check_nms(corners, np.full(300, 0.5, np.float32), 0.15, 1000, expect=[299])          # all tied: the largest index
    corners, scores = _row_scene(1500, spacing=6.0)
    check_nms(corners, scores, 0.15, 1000, expect=list(range(1000)))


def test_nms_tie_order():
    """Blocks of equal scores (many at exactly 1.0f, as saturated sigmoids are) among distinct ones; the tied boxes 3g, 3g + 1 overlap, so
    the order among ties decides which one survives: the larger index."""
    n = 600
    corners, scores = R.cluster_scene(n, 7)
    r = np.random.RandomState(8)
    tied = r.permutation(n // 3)[:120]
    for k, g in enumerate(tied):
        v = np.float32([1.0, 1.0, 0.5, 0.25 + 2.0 ** -24][k % 4])
        scores[3 * g] = scores[3 * g + 1] = v
        if k % 8 == 0:
            scores[3 * g + 2] = v
    assert (scores == 1.0).sum() >= 120
    kept, _ = check_nms(corners, scores, 0.15, 1000)
    kept = set(kept.tolist())
    assert all((3 * g + 1 in kept) and (3 * g not in kept) for g in tied)


def test_nms_exact_threshold():
    """IoU exactly 1/3 (half-shifted box on exact coordinates at 128 m): float32(1/3) is not above the threshold float32(1/3); it is above the
    next float32 below."""
    quads = np.stack([R.bev_quad(128.5, 32.25, 4.5, 2.0, 0.0), R.bev_quad(128.5 + 2.25, 32.25, 4.5, 2.0, 0.0)])
    assert R.quad_iou_exact(quads[0], quads[1]) == Fraction(1, 3)
    corners, scores = corners_of(quads), np.array([0.9, 0.8], np.float32)
    third = np.float32(1.0 / 3.0)
    check_nms(corners, scores, third, 1000, expect=[0, 1], margin_free=False)
    check_nms(corners, scores, np.nextafter(third, np.float32(0)), 1000, expect=[0], margin_free=False)


def _axis_box(x0, x1, y0, y1, z0=-1.8, z1=-0.2):
    q = np.array([[x1, y0], [x1, y1], [x0, y1], [x0, y0]], np.float32)
    c = corners_of(q[None])[0]
    c[:4, 2], c[4:, 2] = z0, z1
    return c


def _range_scene():
    r6 = np.array([-140.8, -40.0, -3.0, 140.8, 40.0, 1.0], np.float32)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))
    boxes = [
        _axis_box(r6[0], r6[0] + 4, -30, -28), _axis_box(dn(r6[0]), r6[0] + 4, -20, -18),          # 0 on x low, 1 outside
        _axis_box(r6[3] - 4, r6[3], -30, -28), _axis_box(r6[3] - 4, up(r6[3]), -20, -18),          # 2 on x high, 3 outside
        _axis_box(-50, -46, r6[1], r6[1] + 2), _axis_box(-40, -36, dn(r6[1]), r6[1] + 2),          # 4 on y low, 5 outside
        _axis_box(-50, -46, r6[4] - 2, r6[4]), _axis_box(-40, -36, r6[4] - 2, up(r6[4])),          # 6 on y high, 7 outside
        _axis_box(0, 4, 0, 2, z0=r6[2]), _axis_box(10, 14, 0, 2, z0=dn(r6[2])),                    # 8 on z low, 9 outside
        _axis_box(20, 24, 0, 2, z1=r6[5]), _axis_box(30, 34, 0, 2, z1=up(r6[5])),                  # 10 on z high, 11 outside
        _axis_box(139, 143, 10, 12), _axis_box(136.5, 140.5, 10, 12),                              # 12 outside, suppresses 13 (IoU 3/13) first
        _axis_box(60, 64, 20, 22),                                                                 # 14 plain
    ]
    scores = (0.95 - 0.01 * np.arange(len(boxes))).astype(np.float32)
    return np.stack(boxes), scores, r6


def test_nms_range_mask_bounds_are_inclusive_and_come_after_the_suppression():
    corners, scores, r6 = _range_scene()
    check_nms(corners, scores, 0.15, 1000, r6, expect=[0, 2, 4, 6, 8, 10, 14])
    check_nms(corners, scores, 0.15, 1000, None, expect=[i for i in range(15) if i != 13])
    inf_z = np.array([r6[0], r6[1], -np.inf, r6[3], r6[4], np.inf], np.float32)                  # as the V2X-Real path passes them
    check_nms(corners, scores, 0.15, 1000, inf_z, expect=[0, 2, 4, 6, 8, 9, 10, 11, 14])


def test_nms_workspace_reuse_large_then_small():
    ws = torch.empty(_size("gencomm_nms_workspace_bytes"), dtype=torch.uint8, device=_dev())
    big_c, big_s = R.cluster_scene(1000, 21)
    small_c, small_s = R.cluster_scene(70, 22)
    check_nms(big_c, big_s, 0.15, 1000, ws=ws)
    _, reused = check_nms(small_c, small_s, 0.15, 1000, ws=ws)
    _, fresh = check_nms(small_c, small_s, 0.15, 1000)
    assert reused["count"] == fresh["count"] and np.array_equal(reused["index"], fresh["index"])


def test_nms_score_domain_negative_zero_and_denormal():
    """The sort key preserves the order of every finite float (include/gencomm_hip.h): negative scores, zero, denormals, the extremes, ties
    among negatives."""
    n = 303
    corners, _ = R.cluster_scene(n, 31)
    r = np.random.RandomState(32)
    scores = r.permutation(np.linspace(-2.0, 2.0, n)).astype(np.float32)
    assert (scores == 0).sum() == 1 and (scores < 0).sum() > 100
    special = np.array([np.finfo(np.float32).max, np.finfo(np.float32).min, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, 1e-40, -1e-40, 0.0,
                        -0.75, -0.75, -0.75, -1e-30, 1e-30], np.float32)
    at = r.permutation(n)[:len(special)]
    scores[at] = special
    assert not np.signbit(scores[scores == 0]).any()
    check_nms(corners, scores, 0.15, 1000)
    check_nms(corners, -np.abs(scores) - np.float32(1e-3), 0.15, 100)
    # all negative and tied in overlapping pairs: the larger index first
    tied = np.repeat(-np.linspace(0.1, 0.9, n // 3), 3).astype(np.float32)
    kept, _ = check_nms(corners, tied, 0.15, 1000)
    assert 1 in kept.tolist() and 0 not in kept.tolist()


# ============================================================================================================== decoding
THR, DIR_OFFSET = 0.2, 0.7853
L, Wd, Hh = 3.9, 1.6, 1.56


def transform(kind):
    def rot(yaw, roll):
        cz, sz, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
        return Rz @ Rx
    T = np.eye(4)
    if kind == "yaw":
        T[:3, :3], T[:3, 3] = rot(0.3, 0.0), [3.0, -2.0, 0.1]
    elif kind == "roll":
        T[:3, :3], T[:3, 3] = rot(-0.2, 0.01), [-1.5, 2.5, -0.05]
    elif kind == "yaw2":
        T[:3, :3], T[:3, 3] = rot(2.1, 0.0), [10.0, 4.0, 0.0]
    else:
        assert kind == "id"
    return T.astype(np.float32)


def make_map(H, W, A, X, seed, hwl=True, nb=2, reg_sigma=0.1):
    """anchors [H, W, A, 7], reg [7A, H, W], dir [A nb, H, W] float32; anchor centres on a grid over +-X m x +-38 m, z = -1."""
    r = np.random.RandomState(seed)
    xs = np.linspace(-X, X, W) if W > 1 else np.zeros(1)
    ys = np.linspace(-38.0, 38.0, H) if H > 1 else np.zeros(1)
    an = np.zeros((H, W, A, 7), np.float32)
    an[..., 0], an[..., 1], an[..., 2] = xs[None, :, None], ys[:, None, None], -1.0
    an[..., 3:6] = [Hh, Wd, L] if hwl else [L, Wd, Hh]
    an[..., 6] = (np.arange(A) * np.pi / A)[None, None, :]
    reg = (r.standard_normal((7 * A, H, W)) * reg_sigma).astype(np.float32)
    dirp = r.standard_normal((A * nb, H, W)).astype(np.float32) if nb else None
    return an, reg, dirp


def logits_from_flat(flat, H, W, A, nc=1):
    """flat [H W A (, nc)] in anchor order (row = pixel * A + anchor) -> cls [A nc, H, W]."""
    return np.ascontiguousarray(flat.reshape(H * W, A * nc).T.reshape(A * nc, H, W)).astype(np.float32)


def survivor_rows(pattern, n, seed):
    r = np.random.RandomState(seed)
    if pattern == "none":
        return np.zeros(0, np.int64)
    if pattern == "all":
        return np.arange(n)
    if pattern == "last":
        return np.array([n - 1])
    if pattern == "one_per_wave":
        w = np.arange((n + 63) // 64)
        rows = w * 64 + (w * 7) % 64
        return rows[rows < n]
    if pattern == "random":
        return np.nonzero(r.rand(n) < 0.03)[0]
    if pattern == "boundary":       # the workgroups around the scan's round of 1024, and the last one
        nwg = (n + 255) // 256
        rows = [5, 300, 1022 * 256 + 17, 1023 * 256, 1023 * 256 + 5, 1023 * 256 + 255, 1024 * 256, 1024 * 256 + 100, (nwg - 1) * 256, n - 1]
        if nwg > 2048:
            rows += [2047 * 256 + 255, 2048 * 256]
        return np.unique([x for x in rows if x < n])
    raise ValueError(pattern)


def flat_logits(n, rows, seed, nc=1):
    r = np.random.RandomState(seed + 1)
    flat = np.full((n, nc), -6.0, np.float32)
    flat[rows, r.randint(0, nc, len(rows))] = r.uniform(1.5, 4.0, len(rows)).astype(np.float32)
    return flat


_R32 = {}


def r32(X, tkind, hwl=True, dirfix=True):
    """Yardstick: worst error of the float32 torch restatement against the float64 reference on a 16 x 32 x 6 map of this range and
    transformation, with or without the direction fix: (score, projected corners, unprojected corners, largest |coordinate| of the map)."""
    key = (X, tkind, hwl, dirfix)
    if key in _R32:
        return _R32[key]
    from oracle import detect_port as D
    H, W, A = 16, 32, 6
    an, reg, dirp = make_map(H, W, A, X, 991, hwl=hwl)
    flat = np.random.RandomState(992).uniform(-4, 4, (H * W * A, 1)).astype(np.float32)
    cls = logits_from_flat(flat, H, W, A)
    T = transform(tkind)
    ref = R.decode_reference(cls, reg, dirp if dirfix else None, an, T, 2, -1.0, DIR_OFFSET, hwl)     # threshold -1: every anchor decoded
    assert ref["dir_dist"].min() > 1e-5
    with torch.no_grad():
        prob = torch.sigmoid(torch.from_numpy(cls)[None].permute(0, 2, 3, 1)).reshape(-1).numpy()
        b = D.delta_to_boxes3d(torch.from_numpy(reg)[None], torch.from_numpy(an))[0]
        dcp = torch.from_numpy(dirp)[None].permute(0, 2, 3, 1).contiguous().reshape(-1, 2)
        if dirfix:
            labels = torch.max(dcp, dim=-1)[1]
            period = 2 * np.pi / 2
            rot = D.limit_period(b[..., 6] - DIR_OFFSET, 0, period)
            b[..., 6] = rot + DIR_OFFSET + period * labels.to(dcp.dtype)
            b[..., 6] = D.limit_period(b[..., 6], 0.5, 2 * np.pi)
        u = D.boxes_to_corners_3d(b, "hwl" if hwl else "lhw")
        p = D.project_box3d(u, torch.from_numpy(T))
    out = (float(np.abs(prob - ref["score"]).max()), float(np.abs(p.numpy() - ref["corners"]).max()), float(np.abs(u.numpy() - ref["unprojected"]).max()),
           float(np.abs(ref["corners"]).max()))
    _R32[key] = out
    return out


def gpu_decode(agents, nb, thr, off, hwl, capacity):
    """agents: [(cls, reg, dirp or None, anchors, T)] appended into one candidate buffer."""
    cor, sco, idx = Guarded((capacity, 8, 3)), Guarded((capacity,)), Guarded((capacity,), torch.int32, fill=-5)
    cnt = torch.zeros(1, dtype=torch.int32, device=_dev())
    for cls, reg, dirp, an, T in agents:
        H, W, A = an.shape[:3]
        ws = torch.empty(_size("gencomm_det_workspace_bytes", H, W, A), dtype=torch.uint8, device=_dev())
        tc, tr, td, ta, tT = _t(cls), _t(reg), (None if dirp is None else _t(dirp)), _t(an), _t(T)
        _call("gencomm_det_decode_fwd", _p(tc), _p(tr), _p(td), _p(ta), _p(tT), H, W, A, nb if dirp is not None else 0, float(thr),
              float(off), int(hwl), _p(cor.t), _p(sco.t), _p(idx.t), _p(cnt), capacity, _p(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    return dict(corners=cor.get(), scores=sco.get(), index=idx.get(), count=int(cnt.item()))


def assert_margins(ref, yard, exact_rows=()):
    """No anchor within 8 r32 of a selection boundary, except the rows that sit on one by construction."""
    free = np.ones(len(ref["score"]), bool)
    free[np.asarray(exact_rows, np.int64)] = False
    sd = ref["score_dist"][free]
    assert np.abs(sd[np.isfinite(sd)]).min(initial=np.inf) > 8 * yard[0]
    rows = ref["rows"]
    sel = free[rows] & ref["above"][rows]
    fd = ref["filter_dist"][sel]
    assert np.abs(fd[np.isfinite(fd)]).min(initial=np.inf) > 16 * yard[1]       # an extent is the difference of two corners
    dd = ref["dir_dist"][ref["above"] & free]
    assert dd[np.isfinite(dd)].min(initial=np.inf) > 1e-5                       # float32 yaw error 2^-23 pi / period < 1e-6


def check_decode(agents, nb, thr, off, hwl, X, tkinds, capacity=None, exact_rows=None, what=""):
    refs = []
    worst = [0.0, 0.0]
    bound = [0.0, 0.0]
    for k, (cls, reg, dirp, an, T) in enumerate(agents):
        ref = R.decode_reference(cls, reg, dirp, an, T, nb, thr, off, hwl, rows="above")
        yard = r32(X[k] if isinstance(X, (list, tuple)) else X, tkinds[k], hwl, dirp is not None)
        assert_margins(ref, yard, () if exact_rows is None else exact_rows[k])
        refs.append((ref, yard))
    total = sum(len(r["candidates"]) for r, _ in refs)
    cap = max(total, 1) if capacity is None else capacity
    got = gpu_decode(agents, nb, thr, off, hwl, cap)
    assert got["count"] == total, (got["count"], total)
    want_idx = np.concatenate([r["candidates"] for r, _ in refs]) if refs else np.zeros(0, np.int64)
    m = min(total, cap)
    assert got["index"][:m].tolist() == want_idx[:m].tolist()
    assert (got["index"][m:] == -5).all() and (got["scores"][m:] == SENT).all() and (got["corners"][m:] == SENT).all()
    assert np.isfinite(got["scores"][:m]).all() and np.isfinite(got["corners"][:m]).all()
    o = 0
    for ref, yard in refs:
        c = len(ref["candidates"])
        lo, hi = min(o, m), min(o + c, m)
        if hi > lo:
            es = np.abs(got["scores"][lo:hi] - ref["score"][ref["candidates"]][:hi - lo]).max()
            ec = np.abs(got["corners"][lo:hi] - ref["corners"][ref["cand_pos"]][:hi - lo]).max()
            assert es <= 4 * yard[0], (es, yard[0])
            assert ec <= 4 * yard[1], (ec, yard[1])
            worst = [max(worst[0], es), max(worst[1], ec)]
            bound = [max(bound[0], yard[0]), max(bound[1], yard[1])]
        o += c
    print(f"decode {what}: {total} survivors, |x| <= {X} m, r32 score {bound[0]:.2e} kernel {worst[0]:.2e}, r32 corners {bound[1]:.2e} kernel {worst[1]:.2e}")
    return got, refs


SMALL = [(1, 1, 1), (3, 5, 2), (7, 37, 2), (16, 32, 6)]
BIG = [(1, 262144, 1), (1, 262145, 1), (1, 524289, 1)]


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("pattern", ["none", "all", "last", "one_per_wave", "random"])
def test_decode_small_shapes(shape, pattern):
    H, W, A = shape
    n = H * W * A
    X = 40.0
    an, reg, dirp = make_map(H, W, A, X, 10 + n)
    cls = logits_from_flat(flat_logits(n, survivor_rows(pattern, n, n), n), H, W, A)
    got, refs = check_decode([(cls, reg, dirp, an, transform("yaw"))], 2, THR, DIR_OFFSET, True, X, ["yaw"], what=f"{shape} {pattern}")
    if pattern == "all":
        assert got["count"] >= 0.9 * n
    if pattern == "none":
        assert got["count"] == 0


@pytest.mark.parametrize("shape", BIG)
@pytest.mark.parametrize("pattern", ["none", "last", "boundary", "one_per_wave", "random"])
def test_decode_scan_rounds(shape, pattern):
    """1024, 1025 and 2049 workgroups: one, two and three rounds of the workgroup-count scan; survivors in workgroups 1023, 1024 and the last
    one, so a lost carry between rounds moves a slot."""
    H, W, A = shape
    n = H * W * A
    X = 140.0
    an, reg, dirp = make_map(H, W, A, X, 20 + (n % 1000))
    rows = survivor_rows(pattern, n, n)
    cls = logits_from_flat(flat_logits(n, rows, n), H, W, A)
    got, refs = check_decode([(cls, reg, dirp, an, transform("id"))], 2, THR, DIR_OFFSET, True, X, ["id"], what=f"{shape} {pattern}")
    assert got["count"] >= 0.9 * len(rows)


def test_decode_all_survive_at_1024_workgroups():
    H, W, A = 1, 262144, 1
    n = H * W * A
    an, reg, dirp = make_map(H, W, A, 140.0, 77)
    cls = logits_from_flat(flat_logits(n, np.arange(n), 78), H, W, A)
    got, _ = check_decode([(cls, reg, dirp, an, transform("id"))], 2, THR, DIR_OFFSET, True, 140.0, ["id"], what="all of 262144")
    assert got["count"] >= 0.99 * n


@pytest.mark.parametrize("kinds", [("yaw", "roll"), ("yaw", "roll", "yaw2"), ("id", "yaw", "roll")])
def test_decode_agents_append_into_one_buffer(kinds):
    H, W, A = 7, 37, 2
    n = H * W * A
    agents = []
    for k, kind in enumerate(kinds):
        an, reg, dirp = make_map(H, W, A, 40.0, 300 + k)
        cls = logits_from_flat(flat_logits(n, survivor_rows("random", n, 310 + k) if k != 1 else np.arange(0, n, 3), 320 + k), H, W, A)
        agents.append((cls, reg, dirp, an, transform(kind)))
    got, refs = check_decode(agents, 2, THR, DIR_OFFSET, True, 40.0, list(kinds), what=f"agents {kinds}")
    assert all(len(r["candidates"]) > 5 for r, _ in refs)
    # the same agents through a 262145-anchor first agent: the second agent's slots start after two scan rounds
    an, reg, dirp = make_map(1, 262145, 1, 140.0, 333)
    cls = logits_from_flat(flat_logits(262145, survivor_rows("boundary", 262145, 1), 334), 1, 262145, 1)
    check_decode([(cls, reg, dirp, an, transform("id"))] + agents[:1], 2, THR, DIR_OFFSET, True, [140.0, 40.0], ["id", kinds[0]], what="big + small agent")


@pytest.mark.parametrize("capacity", [1, 10, 39, 40])
def test_decode_capacity_smaller_than_the_survivors(capacity):
    H, W, A = 7, 37, 2
    n = H * W * A
    an, reg, dirp = make_map(H, W, A, 40.0, 400)
    rows = np.arange(3, n, 13)[:40]
    cls = logits_from_flat(flat_logits(n, rows, 401), H, W, A)
    got, refs = check_decode([(cls, reg, dirp, an, transform("yaw"))], 2, THR, DIR_OFFSET, True, 40.0, ["yaw"], capacity=capacity,
                             what=f"capacity {capacity}")
    assert got["count"] == 40
    # two agents, the capacity runs out inside the first: the second writes nothing
    got, _ = check_decode([(cls, reg, dirp, an, transform("yaw"))] * 2, 2, THR, DIR_OFFSET, True, 40.0, ["yaw", "yaw"], capacity=capacity,
                          what=f"capacity {capacity}, two agents")
    assert got["count"] == 80


@pytest.mark.parametrize("nb,with_dir,hwl", [(2, True, True), (1, True, True), (2, False, True), (2, True, False), (1, False, False)])
def test_decode_option_variants(nb, with_dir, hwl):
    H, W, A = 16, 32, 6
    n = H * W * A
    an, reg, dirp = make_map(H, W, A, 40.0, 500 + nb, hwl=hwl, nb=nb)
    cls = logits_from_flat(flat_logits(n, survivor_rows("random", n, 501), 502), H, W, A)
    tk = "roll"
    check_decode([(cls, reg, dirp if with_dir else None, an, transform(tk))], nb, THR, DIR_OFFSET if with_dir else 0.0, hwl, 40.0, [tk],
                 what=f"bins {nb}, dir {with_dir}, hwl {hwl}")


def test_decode_direction_tie_takes_bin_0():
    H, W, A = 7, 37, 2
    n = H * W * A
    an, reg, dirp = make_map(H, W, A, 40.0, 600)
    dirp[:] = np.float32(0.5)                               # every anchor ties: bin 0
    cls = logits_from_flat(flat_logits(n, np.arange(n), 601), H, W, A)
    got, refs = check_decode([(cls, reg, dirp, an, transform("yaw"))], 2, THR, DIR_OFFSET, True, 40.0, ["yaw"], what="direction tie")
    flipped = dirp.copy()
    flipped.reshape(A, 2, H * W)[:, 1] = 0.75               # bin 1 everywhere: the boxes turn by pi, the corner order changes
    got2, _ = check_decode([(cls, reg, flipped, an, transform("yaw"))], 2, THR, DIR_OFFSET, True, 40.0, ["yaw"], what="direction bin 1")
    assert np.abs(got["corners"] - got2["corners"]).max() > 1.0


def test_decode_zero_y_extent_is_rejected():
    """A width delta of -200 underflows expf to 0.0f; at yaw 0 (no direction fix) and the identity transformation every corner has the same y,
    the y extent is exactly 0 and the reference's size filter, which uses it as a truth value, rejects the box."""
    H, W, A = 3, 5, 2
    n = H * W * A
    an, reg, _ = make_map(H, W, A, 40.0, 700)
    zero = [0, 8, 14, 28]                                   # anchor 0 of its pixel: yaw 0
    for i in zero:
        pix, a = divmod(i, A)
        assert a == 0
        reg.reshape(A, 7, H * W)[a, 4, pix] = -200.0
        reg.reshape(A, 7, H * W)[a, 6, pix] = 0.0
    reg.reshape(A, 7, H * W)[1, 4, 3] = -200.0              # anchor 1 (yaw pi / 2) of pixel 3: its zero extent is x's, which only has to be <= 6
    cls = logits_from_flat(flat_logits(n, np.arange(n), 701), H, W, A)
    got, refs = check_decode([(cls, reg, None, an, transform("id"))], 0, THR, 0.0, True, 40.0, ["id"], exact_rows=[zero + [7]],
                             what="zero y extent")
    assert got["count"] == n - len(zero) and not set(zero) & set(got["index"][:got["count"]].tolist())
    assert 7 in got["index"].tolist()


def test_decode_non_finite_inputs_are_rejected_and_nothing_non_finite_is_stored():
    """NaN and -inf logits never pass the threshold; a +inf logit is sigmoid 1.0 and passes, as in the reference; a box with a NaN or infinite
    delta fails the reference's size / z comparisons (torch's max / min propagate the NaN) and is rejected."""
    H, W, A = 3, 5, 2
    n = H * W * A
    an, reg, dirp = make_map(H, W, A, 40.0, 800)
    flat = flat_logits(n, np.arange(n), 801)
    flat[0], flat[1], flat[2] = np.nan, np.inf, -np.inf
    rv = reg.reshape(A, 7, H * W)
    bad = {3: (0, np.nan), 4: (3, np.inf), 5: (6, np.nan), 6: (2, np.inf), 7: (1, -np.inf), 8: (4, np.nan), 9: (6, np.inf), 10: (5, np.nan),
           11: (0, np.inf), 12: (2, np.nan)}
    for i, (d, v) in bad.items():
        pix, a = divmod(i, A)
        rv[a, d, pix] = v
    cls = logits_from_flat(flat, H, W, A)
    for with_dir in (True, False):
        got, refs = check_decode([(cls, reg, dirp if with_dir else None, an, transform("yaw"))], 2, THR, DIR_OFFSET, True, 40.0, ["yaw"],
                                 what=f"non-finite, dir {with_dir}")
        kept = got["index"][:got["count"]].tolist()
        assert kept[0] == 1 and got["scores"][0] == 1.0 and not set(kept) & ({0, 2} | set(bad)) and len(kept) >= n - 15


# -------------------------------------------------------------------------------------------------------------- multi-class
def gpu_decode_mc(agents, A, nc, thr, hwl, capacity, with_unprojected=True):
    """agents: [(cls [A nc, H, W], reg, anchors, T)]."""
    n = len(agents)
    keep = [[_t(x) for x in ag] for ag in agents]
    PA, IA = C.c_void_p * n, C.c_int * n
    Hs, Ws = IA(*[ag[2].shape[0] for ag in agents]), IA(*[ag[2].shape[1] for ag in agents])
    cor, unp = Guarded((capacity, 8, 3)), Guarded((capacity, 8, 3))
    sco, lab = Guarded((capacity,)), Guarded((capacity,), torch.int32, fill=-5)
    cnt = torch.full((2,), -9, dtype=torch.int32, device=_dev())       # count, violations: the call starts both
    ws = torch.empty(_size("gencomm_det_mc_workspace_bytes", Hs, Ws, n, A), dtype=torch.uint8, device=_dev())
    _call("gencomm_det_mc_decode_fwd", PA(*[_p(k[0]) for k in keep]), PA(*[_p(k[1]) for k in keep]), PA(*[_p(k[2]) for k in keep]),
          PA(*[_p(k[3]) for k in keep]), Hs, Ws, n, A, nc, float(thr), int(hwl), _p(cor.t), _p(unp.t) if with_unprojected else 0, _p(sco.t),
          _p(lab.t), _p(cnt[0:1]), _p(cnt[1:2]), capacity, _p(ws), ws.numel(), _st())
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    return dict(corners=cor.get(), unprojected=unp.get(), scores=sco.get(), labels=lab.get(), count=int(c[0]), violations=int(c[1]))


def check_decode_mc(agents, A, nc, X, tkinds, capacity=None, with_unprojected=True, saturated=None, what=""):
    ref = R.decode_mc_reference(agents, A, nc, THR, True)
    yards = [r32(X, k, True, False) for k in tkinds]
    ys, yc, yu = max(y[0] for y in yards), max(y[1] for y in yards), max(y[2] for y in yards)
    reach = min(y[3] for y in yards)
    free = np.ones(len(ref["score_dist"]), bool)
    if saturated is not None:
        free[saturated] = False
    assert np.abs(ref["score_dist"][free]).min(initial=np.inf) > 8 * ys
    assert ref["class_gap"][free & (ref["score_dist"] > 0)].min(initial=np.inf) > 8 * ys       # the label of a candidate is decided
    fd = ref["filter_dist"]
    assert np.abs(fd[np.isfinite(fd) & (fd != -100.0)]).min(initial=np.inf) > 16 * yc   # -100: the y extent exactly 0 by construction
    total = len(ref["score"])
    cap = max(total, 1) if capacity is None else capacity
    got = gpu_decode_mc(agents, A, nc, THR, True, cap, with_unprojected)
    assert got["count"] == total and got["violations"] == int(ref["violation"].sum()), (got["count"], total, got["violations"])
    m = min(total, cap)
    assert got["labels"][:m].tolist() == ref["label"][:m].tolist()
    assert (got["labels"][m:] == -5).all() and (got["scores"][m:] == SENT).all() and (got["corners"][m:] == SENT).all()
    es = ec = eu = 0.0
    if m:
        es = np.abs(got["scores"][:m] - ref["score"][:m]).max()
        fin = np.isfinite(ref["corners"][:m]).all((1, 2))
        # float32 errors grow with the magnitude: a 213 m box made to violate the size filter reaches further out than the yardstick's map
        scale = np.maximum(1.0, np.abs(ref["corners"][:m][fin]).max((1, 2)) / reach)[:, None, None]
        ec = (np.abs(got["corners"][:m][fin] - ref["corners"][:m][fin]) / scale).max(initial=0.0)
        assert es <= 4 * ys and ec <= 4 * yc, (es, ys, ec, yc)
        if with_unprojected:
            eu = (np.abs(got["unprojected"][:m][fin] - ref["unprojected"][:m][fin]) / scale).max(initial=0.0)
            assert eu <= 4 * yu, (eu, yu)
    if not with_unprojected:
        assert (got["unprojected"] == SENT).all()
    else:
        assert (got["unprojected"][m:] == SENT).all()
    print(f"decode mc {what}: {total} candidates, {got['violations']} violations, r32 {ys:.2e} / {yc:.2e} / {yu:.2e}, kernel {es:.2e} / {ec:.2e} / {eu:.2e}")
    return got, ref


def mc_agent(H, W, A, nc, X, seed, pattern, tkind, violate=0):
    n = H * W * A
    an, reg, _ = make_map(H, W, A, X, seed, nb=0)
    rows = survivor_rows(pattern, n, seed + 1)
    flat = flat_logits(n, rows, seed + 2, nc)
    rv = reg.reshape(A, 7, H * W)
    for i in rows[:violate]:                                # a length of 3.9 e^4 = 213 m: x or y extent above 100 m
        pix, a = divmod(int(i), A)
        rv[a, 5, pix] = 4.0
    return (logits_from_flat(flat, H, W, A, nc), reg, an, transform(tkind))


@pytest.mark.parametrize("shape,nc,pattern", [((1, 1, 1), 1, "all"), ((3, 5, 2), 3, "all"), ((7, 37, 2), 3, "random"), ((7, 37, 2), 1, "one_per_wave"),
                                              ((3, 5, 2), 3, "none"), ((1, 262144, 1), 1, "boundary"), ((1, 262145, 1), 1, "boundary"),
                                              ((1, 262145, 1), 3, "random"), ((1, 524289, 1), 3, "boundary"), ((1, 524289, 1), 1, "one_per_wave"),
                                              ((1, 262145, 1), 1, "last")])
def test_decode_mc_one_agent(shape, nc, pattern):
    H, W, A = shape
    X = 140.0 if W > 1000 else 40.0
    tk = "id" if W > 1000 else "roll"
    ag = mc_agent(H, W, A, nc, X, 900 + nc, pattern, tk, violate=2 if pattern in ("boundary", "random") else 0)
    got, ref = check_decode_mc([ag], A, nc, X, [tk], what=f"{shape} nc {nc} {pattern}")
    if nc == 3 and pattern != "none":
        assert set(ref["label"].tolist()) == {1, 2, 3}


def test_decode_mc_saturated_classes_tie_and_the_first_wins():
    H, W, A, nc = 3, 5, 2, 3
    n = H * W * A
    an, reg, _ = make_map(H, W, A, 40.0, 950, nb=0)
    flat = flat_logits(n, np.arange(0, n, 2), 951, nc)
    sat = [1, 7, 13]
    flat[1] = [20.0, 30.0, -6.0]      # classes 1 and 2 are 1.0f; the second has the larger logit
    flat[7] = [-6.0, 25.0, 40.0]
    flat[13] = [18.0, 18.0, 18.0]
    ag = (logits_from_flat(flat, H, W, A, nc), reg, an, transform("yaw"))
    got, ref = check_decode_mc([ag], A, nc, 40.0, ["yaw"], saturated=sat, what="saturated")
    # candidates are in anchor order: find the saturated ones by their score
    lab = {int(i): int(l) for i, l in zip(np.nonzero(ref["score_dist"] > 0)[0], got["labels"][:got["count"]])}
    assert (lab[1], lab[7], lab[13]) == (1, 2, 1)
    assert all(got["scores"][list(lab).index(i)] == 1.0 for i in sat)


@pytest.mark.parametrize("n_agents", [1, 8, 9, 17])
def test_decode_mc_chunks_carry_count_and_violations(n_agents):
    """Chunks of eight agents: one, two and three launches sets; agents of different H x W in one call; the candidate count and the violation
    counter carry across the chunks; violating candidates are still emitted."""
    shapes = [(3, 5), (7, 37), (1, 300), (2, 129)]
    kinds = ["yaw", "roll", "yaw2", "id"]
    agents, tk = [], []
    for k in range(n_agents):
        H, W = shapes[k % 4]
        pattern = "none" if k == 3 else ("all" if H * W < 100 else "random")
        agents.append(mc_agent(H, W, 2, 3, 40.0, 1000 + 7 * k, pattern, kinds[(k + k // 4) % 4], violate=1 if k % 3 != 1 else 0))
        tk.append(kinds[(k + k // 4) % 4])
    got, ref = check_decode_mc(agents, 2, 3, 40.0, tk, what=f"{n_agents} agents")
    assert got["violations"] >= (n_agents + 1) // 2 and got["count"] > 10 * n_agents
    if n_agents == 9:
        check_decode_mc(agents, 2, 3, 40.0, tk, with_unprojected=False, what="9 agents, no unprojected")
        check_decode_mc(agents, 2, 3, 40.0, tk, capacity=50, what="9 agents, capacity 50")


def test_decode_mc_zero_y_extent_and_non_finite_are_violations():
    H, W, A, nc = 3, 5, 2, 3
    n = H * W * A
    an, reg, _ = make_map(H, W, A, 40.0, 1100, nb=0)
    rv = reg.reshape(A, 7, H * W)
    rv[0, 4, 2], rv[0, 6, 2] = -200.0, 0.0        # anchor row 4: zero y extent
    rv[1, 0, 5] = np.nan                          # row 11
    rv[0, 3, 6] = np.inf                          # row 12
    flat = flat_logits(n, np.arange(n), 1101, nc)
    ag = (logits_from_flat(flat, H, W, A, nc), reg, an, transform("id"))
    got, ref = check_decode_mc([ag], A, nc, 40.0, ["id"], what="zero extent / non-finite")
    assert got["violations"] == 3 and np.nonzero(ref["violation"])[0].tolist() == [4, 11, 12]


def test_det_mc_gather():
    cap, top = 50, 16
    r = np.random.RandomState(5)
    labels = r.randint(1, 4, cap).astype(np.int32)
    unp = r.standard_normal((cap, 8, 3)).astype(np.float32)
    out_scores = r.rand(top).astype(np.float32)
    for count, use_top, with_unp in [(10, 16, True), (16, 16, True), (12, 5, True), (0, 16, True), (10, 16, False), (16, 1, True)]:
        index = r.permutation(cap)[:top].astype(np.int32)
        sl, ou = Guarded((top, 2)), Guarded((top, 8, 3))
        ti, tc, ts, tl, tu = _t(index, torch.int32), _t(np.array([count], np.int32), torch.int32), _t(out_scores), _t(labels, torch.int32), _t(unp)
        _call("gencomm_det_mc_gather_fwd", _p(ti), _p(tc), _p(ts), _p(tl), _p(tu) if with_unp else 0, cap, use_top, _p(sl.t),
              _p(ou.t) if with_unp else 0, _st())
        sl, ou = sl.get(), ou.get()
        m = min(count, use_top)
        assert np.array_equal(_bits(sl[:m, 0]), _bits(out_scores[:m])) and sl[:m, 1].tolist() == labels[index[:m]].astype(np.float32).tolist()
        assert (sl[m:] == SENT).all() and (ou[m:] == SENT).all()
        assert np.array_equal(_bits(ou[:m]), _bits(unp[index[:m]])) if with_unp else (ou == SENT).all()
        assert m == 0 or sl[:m, 1].min() >= 1.0          # labels are 1-based


# ============================================================================================================== iou3d_nms, bbox_overlaps
def _iou3d_families():
    boxes_a, boxes_b, kind = [], [], []
    for cx, cy in [(0.0, 0.0), (35.5, -12.25), (-120.0, 38.0)]:
        for yaw in (0.0, np.pi, -np.pi, 0.3, np.pi / 2):
            a = [cx, cy, -1.0, 4.5, 2.0, 1.6, yaw]
            boxes_a.append(a); boxes_b.append(list(a)); kind.append("identical")
            boxes_a.append(a); boxes_b.append([cx + 0.2, cy - 0.1, -1.0, 2.0, 1.0, 1.6, yaw]); kind.append("inside")
            boxes_a.append([cx + 0.2, cy - 0.1, -1.0, 2.0, 0.8, 1.6, yaw + 0.2]); boxes_b.append([cx, cy, -1.0, 6.0, 4.0, 1.6, yaw]); kind.append("inside")
            boxes_a.append(a); boxes_b.append([cx + 20.0, cy + 9.0, -1.0, 4.5, 2.0, 1.6, yaw + 1.0]); kind.append("disjoint")
            boxes_a.append(a); boxes_b.append([cx + 5.0, cy, -1.0, 4.5, 2.0, 1.6, yaw]); kind.append("disjoint")
            boxes_a.append(a); boxes_b.append([cx, cy, -1.0, 0.0, 0.0, 0.0, yaw]); kind.append("zero")
            boxes_a.append([cx, cy, -1.0, 0.0, 0.0, 1.6, yaw]); boxes_b.append([cx, cy, -1.0, 0.0, 0.0, 1.6, yaw]); kind.append("zero")
            boxes_a.append([cx + 30.0, cy, -1.0, 0.0, 2.0, 1.6, yaw]); boxes_b.append(a); kind.append("disjoint")
    return np.array(boxes_a, np.float32), np.array(boxes_b, np.float32), np.array(kind)


def test_iou3d_pairwise_degenerate_families():
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import native_port as N
    a, b, kind = _iou3d_families()
    ta, tb = _t(a), _t(b)
    for mode, ref, atol in ((0, N.boxes_overlap_bev(a, b), 1e-5), (1, N.boxes_iou_bev(a, b), 1e-6)):
        out = Guarded((len(a), len(b)), fill=SENT)
        _call("gencomm_iou3d_pairwise_fwd", _p(ta), len(a), _p(tb), len(b), mode, _p(out.t), _st())
        got = out.get()
        assert np.isfinite(got).all()
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=atol)
        d = np.diagonal(got)
        assert (d[kind == "disjoint"] == 0.0).all()          # no crossing, no included corner: the centroid division must not leak a NaN
        if mode == 1:
            assert np.abs(d[kind == "identical"] - 1.0).max() < 1e-5
    print(f"iou3d degenerate: {len(a)} x {len(b)} pairs")


def test_iou3d_nms_degenerate_families():
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import native_port as N
    a, b, _ = _iou3d_families()
    boxes = np.concatenate([a, b])
    scores = np.random.RandomState(4).permutation(np.linspace(0.1, 0.9, len(boxes))).astype(np.float32)
    order = np.argsort(-scores, kind="stable")
    sb = boxes[order]
    n = len(sb)
    for thresh, normal in ((0.5, 0), (0.1, 0), (0.5, 1)):
        keep, cnt = Guarded((n,), torch.int64, fill=-5), Guarded((1,), torch.int32, fill=-5)
        ws = torch.empty(max(_size("gencomm_iou3d_nms_workspace_bytes", n), 1), dtype=torch.uint8, device=_dev())
        tb = _t(sb)
        _call("gencomm_iou3d_nms_fwd", _p(tb), n, thresh, normal, _p(keep.t), _p(cnt.t), _p(ws), ws.numel(), _st())
        m = int(cnt.get()[0])
        want = N.nms(boxes, scores, thresh, normal=bool(normal))
        assert order[keep.get()[:m]].tolist() == want.tolist()
        assert (keep.get()[m:] == -5).all()


def _bbox_cases():
    r = np.random.RandomState(6)
    def rnd(n, base=0.0):
        x1, y1 = r.uniform(0, 200, n) + base, r.uniform(0, 200, n) + base
        return np.stack([x1, y1, x1 + r.uniform(1, 60, n), y1 + r.uniform(1, 60, n)], 1).astype(np.float32)
    touch_b = np.array([[10, 10, 20, 20]] * 4, np.float32)
    touch_q = np.array([[21, 10, 30, 20],      # iw = 20 - 21 + 1 = 0: no overlap
                        [20, 10, 30, 20],      # iw = 1
                        [10, 21, 20, 30],      # ih = 0
                        [10, 20, 20, 30]], np.float32)
    inverted = np.array([[30, 30, 10, 10], [5, 5, 4, 4], [0, 0, -1, -1], [10, 10, 20, 20]], np.float32)
    return {"7x37": (rnd(7), rnd(37)), "1x1": (rnd(1), rnd(1)), "300x3": (rnd(300), rnd(3)), "touching": (touch_b, touch_q),
            "inverted": (inverted, np.concatenate([inverted, touch_q])), "near_1e4": (rnd(33, 1e4 - 100), rnd(19, 1e4 - 100)),
            "N0": (np.zeros((0, 4), np.float32), rnd(5)), "K0": (rnd(5), np.zeros((0, 4), np.float32))}


@pytest.mark.parametrize("name", ["7x37", "1x1", "300x3", "touching", "inverted", "near_1e4", "N0", "K0"])
def test_bbox_overlaps_edges_bit_exact(name):
    from oracle import detect_port as D
    b, q = _bbox_cases()[name]
    N, K = len(b), len(q)
    out = Guarded((max(N * K, 1),), fill=SENT)
    tb, tq = _t(b), _t(q)
    _call("gencomm_bbox_overlaps_fwd", _p(tb) if N else 0, _p(tq) if K else 0, _p(out.t), N, K, _st())
    got = out.get()
    if N * K == 0:
        assert (got == SENT).all()
        return
    want = D.bbox_overlaps(b, q)
    assert np.array_equal(_bits(got.reshape(N, K)), _bits(want))
    if name == "touching":
        assert want[0, 0] == 0 and want[1, 1] > 0 and want[2, 2] == 0 and want[3, 3] > 0
    if name == "near_1e4":
        assert (want > 0).sum() > 10
