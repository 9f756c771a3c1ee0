"""Independent references for the detection tail (gencomm_amd/csrc/detect_kernels.h), used by tests/test_detect_reference.py (CPU) and
tests/test_gpu_detect_kernels.py (GPU). Nothing here shares an algorithm with the kernels or with oracle/detect_port.py:

  quad_iou_exact      IoU of two convex quadrilaterals in exact rational arithmetic on the float32 corner values. No clipping: the
                      intersection polygon is the convex hull of {vertices of p inside or on q} + {vertices of q inside or on p} +
                      {proper crossings of the 16 edge pairs}; hull by monotone chain, area by the shoelace formula.
  quad_iou_f64        the same vertex enumeration in numpy float64, batched over pairs, after a bounding-circle rejection (exactly 0).
                      Every orientation predicate is taken on float32 corner values, whose differences and products are exact in
                      float64, so every sign is exact; only the crossing points and the area sums round (coordinates are shifted to
                      p's first corner first, so the sums do not cancel at 140 m).
  nms_reference       greedy rotated NMS over that IoU matrix: score descending then index descending, cut at `top`, suppression when
                      float32(iou) > float32(thr) as the kernel rounds, range mask on all 8 corners (inclusive) after the suppression.
  decode_reference    anchor decoding in float64 from the float32 inputs, single class (direction fix, 6 m / [-3, 1] filters) ...
  decode_mc_reference ... and multi-class (class max over the sigmoids, 100 m filters counted as violations, agents concatenated).
"""
from fractions import Fraction

import numpy as np

F32_TINY_EXP = -150.0 * np.log(2.0)   # expf(d) rounds to 0.0f below this (half the smallest float32 denormal)


# ------------------------------------------------------------------------------------------------------------- exact quad IoU
def _frac_pts(p):
    p = np.asarray(p)
    assert p.shape == (4, 2)
    return [(Fraction(float(x)), Fraction(float(y))) for x, y in p]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _shoelace(pts):
    n = len(pts)
    if n < 3:
        return Fraction(0)
    return sum(pts[i][0] * pts[(i + 1) % n][1] - pts[(i + 1) % n][0] * pts[i][1] for i in range(n)) / 2


def _hull(pts):
    pts = sorted(set(pts))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def _inside_or_on(v, poly):   # poly counter-clockwise, non-degenerate
    return all(_cross(poly[i], poly[(i + 1) % 4], v) >= 0 for i in range(4))


def quad_iou_exact(p, q):
    """Fraction: the IoU of the convex quadrilaterals p, q ((4, 2) float32 values, either orientation); 0 when the union is 0."""
    p, q = _frac_pts(p), _frac_pts(q)
    ap, aq = _shoelace(p), _shoelace(q)
    if ap < 0:
        p, ap = p[::-1], -ap
    if aq < 0:
        q, aq = q[::-1], -aq
    if ap + aq == 0:
        return Fraction(0)
    if ap == 0 or aq == 0:   # a subset of a set without area has no area
        return Fraction(0)
    pts = [v for v in p if _inside_or_on(v, q)] + [v for v in q if _inside_or_on(v, p)]
    for i in range(4):
        a, b = p[i], p[(i + 1) % 4]
        for j in range(4):
            c, d = q[j], q[(j + 1) % 4]
            d1, d2 = _cross(c, d, a), _cross(c, d, b)
            d3, d4 = _cross(a, b, c), _cross(a, b, d)
            if d1 * d2 < 0 and d3 * d4 < 0:
                t = d1 / (d1 - d2)
                pts.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
    inter = abs(_shoelace(_hull(pts)))
    return inter / (ap + aq - inter)


# ------------------------------------------------------------------------------------------------------------- float64 quad IoU
def _area64(P):   # [M, n, 2] -> [M]
    x, y = P[..., 0], P[..., 1]
    return 0.5 * np.sum(x * np.roll(y, -1, axis=-1) - np.roll(x, -1, axis=-1) * y, axis=-1)


def _cross64(o, a, b):
    return (a[..., 0] - o[..., 0]) * (b[..., 1] - o[..., 1]) - (a[..., 1] - o[..., 1]) * (b[..., 0] - o[..., 0])


def circle_reject(P, Q):
    """[M] bool: the bounding circles (centre = corner mean) of the pairs are apart by more than rounding, so the IoU is exactly 0."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    cp, cq = P.mean(-2), Q.mean(-2)
    rp = np.sqrt(((P - cp[..., None, :]) ** 2).sum(-1)).max(-1)
    rq = np.sqrt(((Q - cq[..., None, :]) ** 2).sum(-1)).max(-1)
    d = np.sqrt(((cp - cq) ** 2).sum(-1))
    return d > (rp + rq) * (1 + 1e-9) + 1e-9


def quad_iou_f64_batch(P, Q):
    """P, Q: [M, 4, 2] (float32 values) -> [M] float64 IoU."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 4, 2), np.asarray(Q, np.float64).reshape(-1, 4, 2)
    M = P.shape[0]
    out = np.zeros(M)
    live = np.nonzero(~circle_reject(P, Q))[0]
    if live.size == 0:
        return out
    P, Q = P[live], Q[live]
    org = P[:, :1, :].copy()
    P, Q = P - org, Q - org   # exact: float32 values
    ap, aq = _area64(P), _area64(Q)
    P = np.where((ap < 0)[:, None, None], P[:, ::-1], P)
    Q = np.where((aq < 0)[:, None, None], Q[:, ::-1], Q)
    ap, aq = np.abs(ap), np.abs(aq)
    nxt = [1, 2, 3, 0]
    # vertices of p inside or on q, and of q inside or on p: signs are exact
    sp = np.stack([_cross64(Q[:, None, j], Q[:, None, nxt[j]], P) for j in range(4)], -1)   # [M, 4 (vertex of p), 4 (edge of q)]
    sq = np.stack([_cross64(P[:, None, i], P[:, None, nxt[i]], Q) for i in range(4)], -1)   # [M, 4 (vertex of q), 4 (edge of p)]
    pin, qin = (sp >= 0).all(-1), (sq >= 0).all(-1)
    # proper crossings: edge i of p with edge j of q
    d1 = sp                              # p_i against edge j of q
    d2 = sp[:, nxt, :]                   # p_{i+1} against edge j of q
    d3 = sq.transpose(0, 2, 1)           # q_j against edge i of p  -> [M, i, j]
    d4 = sq[:, nxt, :].transpose(0, 2, 1)
    proper = (((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))) & (((d3 > 0) & (d4 < 0)) | ((d3 < 0) & (d4 > 0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(proper, d1 / (d1 - d2), 0.0)
    A, B = P[:, :, None, :], P[:, nxt][:, :, None, :]
    X = A + t[..., None] * (B - A)       # [M, 4, 4, 2]
    pts = np.concatenate([P, Q, X.reshape(-1, 16, 2)], 1)                # [M, 24, 2]
    ok = np.concatenate([pin, qin, proper.reshape(-1, 16)], 1)           # [M, 24]
    n = ok.sum(-1)
    cen = (pts * ok[..., None]).sum(1) / np.maximum(n, 1)[:, None]
    ang = np.where(ok, np.arctan2(pts[..., 1] - cen[:, None, 1], pts[..., 0] - cen[:, None, 0]), np.inf)
    order = np.argsort(ang, axis=1, kind="stable")
    pts = np.take_along_axis(pts, order[..., None], 1)
    ok = np.take_along_axis(ok, order, 1)
    pts = np.where(ok[..., None], pts, pts[:, :1, :])                    # the invalid slots repeat the first point: no area
    inter = np.where(n >= 3, np.abs(_area64(pts)), 0.0)
    inter = np.where((ap == 0) | (aq == 0), 0.0, inter)
    uni = ap + aq - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        out[live] = np.where(uni > 0, inter / uni, 0.0)
    return out


def quad_iou_f64(p, q):
    return float(quad_iou_f64_batch(np.asarray(p)[None], np.asarray(q)[None])[0])


def quad_iou_matrix_f64(quads):
    """[K, 4, 2] -> [K, K] float64 IoU (upper triangle computed, mirrored), circle-rejected pairs exactly 0."""
    quads = np.asarray(quads, np.float64)
    K = quads.shape[0]
    iou = np.zeros((K, K))
    if K < 2:
        return iou
    i, j = np.triu_indices(K, 1)
    live = ~circle_reject(quads[i], quads[j])
    i, j = i[live], j[live]
    for s in range(0, i.size, 65536):
        v = quad_iou_f64_batch(quads[i[s:s + 65536]], quads[j[s:s + 65536]])
        iou[i[s:s + 65536], j[s:s + 65536]] = v
        iou[j[s:s + 65536], i[s:s + 65536]] = v
    return iou


# ------------------------------------------------------------------------------------------------------------- rotated NMS
def nms_reference(corners, scores, thr, top, range6=None, margin=0.0):
    """corners [n, 8, 3] float32, scores [n] float32 -> (kept indices in output order, [(i, j)] pairs of candidates whose suppression
    decision float32(iou) > float32(thr) changes when the IoU moves by `margin`)."""
    corners = np.asarray(corners, np.float32).reshape(-1, 8, 3)
    scores = np.asarray(scores, np.float32)
    n = scores.shape[0]
    thr = np.float32(thr)
    order = np.lexsort((-np.arange(n), -scores.astype(np.float64)))[:top]
    K = order.shape[0]
    iou = quad_iou_matrix_f64(corners[order][:, :4, :2])
    over = iou.astype(np.float32) > thr
    lo, hi = (iou - margin).astype(np.float32) > thr, (iou + margin).astype(np.float32) > thr
    und = np.argwhere(np.triu(lo != hi, 1))
    undecided = [(int(order[a]), int(order[b])) for a, b in und]
    removed = np.zeros(K, bool)
    kept = []
    for r in range(K):
        if removed[r]:
            continue
        kept.append(r)
        removed[r + 1:] |= over[r, r + 1:]
    kept = order[np.asarray(kept, np.int64)] if kept else np.zeros(0, np.int64)
    if range6 is not None and kept.size:
        r6 = np.asarray(range6, np.float32)
        c = corners[kept]
        inside = ((c >= r6[:3]) & (c <= r6[3:])).all(-1).all(-1)
        kept = kept[inside]
    return kept.astype(np.int64), undecided


# (scene builder shared by the CPU and GPU NMS tests)
def cluster_scene(n, seed, spread=1.0):
    """n car-sized boxes [n, 8, 3] on a 6 m x 3 m grid, in groups of three: a box, a partner shifted / turned onto it (IoU around 0.5) and
    a box of its own; distinct scores in random order."""
    r = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt((n + 1) // 2 + 1)))
    corners = np.zeros((n, 8, 3), np.float32)
    for i in range(n):
        g, k = divmod(i, 3)
        cell = 2 * g + (1 if k == 2 else 0)
        cx, cy = (cell % side - side / 2) * 6.0 * spread, (cell // side - side / 2) * 3.0 * spread
        yaw = 0.0 if k != 1 else r.uniform(0.05, 0.2)
        dx, dy = (0.0, 0.0) if k != 1 else (r.uniform(0.3, 0.9), r.uniform(0.1, 0.3))
        q = bev_quad(cx + dx, cy + dy, 4.5, 2.0, yaw)
        corners[i, :4, :2] = q; corners[i, 4:, :2] = q
        corners[i, :4, 2], corners[i, 4:, 2] = -1.8, -0.2
    scores = r.permutation(np.linspace(0.2, 0.99, n)).astype(np.float32) if n else np.zeros(0, np.float32)
    return corners, scores


# ------------------------------------------------------------------------------------------------------------- decoding
_SX = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64) / 2
_SY = np.array([-1, 1, 1, -1, -1, 1, 1, -1], np.float64) / 2
_SZ = np.array([-1, -1, -1, -1, 1, 1, 1, 1], np.float64) / 2


def _exp_f32(d):
    """exp in float64, but 0 where the float32 result is 0 (and the input is that far down on purpose)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(d < F32_TINY_EXP, 0.0, np.exp(d))


def _sigmoid64(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _boxes7(reg, anchors):
    """reg [7A, H, W], anchors [H, W, A, 7] -> boxes [H W A, 7] float64 (delta_to_boxes3d), row = pixel * A + anchor."""
    H, W, A = anchors.shape[:3]
    an = anchors.astype(np.float64).reshape(-1, 7)
    d = reg.astype(np.float64).reshape(A, 7, H * W).transpose(2, 0, 1).reshape(-1, 7)
    diag = np.sqrt(an[:, 4] ** 2 + an[:, 5] ** 2)
    b = np.empty_like(d)
    with np.errstate(over="ignore", invalid="ignore"):
        b[:, 0] = d[:, 0] * diag + an[:, 0]
        b[:, 1] = d[:, 1] * diag + an[:, 1]
        b[:, 2] = d[:, 2] * an[:, 3] + an[:, 2]
        b[:, 3:6] = _exp_f32(d[:, 3:6]) * an[:, 3:6]
        b[:, 6] = d[:, 6] + an[:, 6]
    return b


def _corners(b, order_hwl, T):
    """boxes [N, 7] -> (unprojected [N, 8, 3], projected [N, 8, 3]) float64."""
    ex, ey, ez = (b[:, 5], b[:, 4], b[:, 3]) if order_hwl else (b[:, 3], b[:, 4], b[:, 5])
    with np.errstate(over="ignore", invalid="ignore"):
        c, s = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
        px, py, pz = ex[:, None] * _SX, ey[:, None] * _SY, ez[:, None] * _SZ
        u = np.stack([px * c - py * s + b[:, 0:1], px * s + py * c + b[:, 1:2], pz + b[:, 2:3]], -1)
        T = np.asarray(T, np.float64)
        p = np.stack([T[r, 0] * u[..., 0] + T[r, 1] * u[..., 1] + T[r, 2] * u[..., 2] + T[r, 3] for r in range(3)], -1)
    return u, p


def _extent(p, limits):
    """projected corners [N, 8, 3] -> (size_ok & z_ok [N], distances of x_len, y_len from the size limit and of zmin, zmax from theirs
    [N, 4]); a non-finite corner fails the filters, as torch's NaN-propagating max / min make it in the reference."""
    size, zlo, zhi = limits
    with np.errstate(over="ignore", invalid="ignore"):
        x_len = p[..., 0].max(1) - p[..., 0].min(1)
        y_len = p[..., 1].max(1) - p[..., 1].min(1)
        zmin, zmax = p[..., 2].min(1), p[..., 2].max(1)
        ok = (x_len <= size) & (y_len <= size) & (y_len != 0) & (zmin >= zlo) & (zmax <= zhi)
        dist = np.stack([x_len - size, y_len - size, zmin - zlo, zmax - zhi], 1)
    return ok, dist


def decode_reference(cls, reg, dirp, anchors, T, num_bins, thr, dir_offset, order_hwl, rows=None):
    """One agent, single class. cls [A, H, W], reg [7A, H, W], dirp [A num_bins, H, W] or None, anchors [H, W, A, 7], T [4, 4], all
    float32. Over all N = H W A anchors (row = pixel * A + anchor): score, above (score > thr), score_dist, dir_dist (distance of the
    direction fix's floor argument from an integer). For the anchors `rows` (None: all; "above": those above the threshold; or an index
    array): corners (projected), unprojected, filter_ok, filter_dist [., 4] (x / y extent - 6, zmin + 3, zmax - 1). keep [N] = above and
    filter_ok (False outside `rows`); candidates = the kept anchors in order, cand_pos = their positions in `rows`."""
    H, W, A = anchors.shape[:3]
    score = _sigmoid64(cls.astype(np.float64).reshape(A, H * W).T.reshape(-1))
    b = _boxes7(reg, anchors)
    N = b.shape[0]
    dir_dist = np.full(N, np.inf)
    if dirp is not None:
        d = dirp.reshape(A, num_bins, H * W).transpose(2, 0, 1).reshape(-1, num_bins)
        label = np.argmax(d, 1)                       # first maximum
        period = 2 * np.pi / num_bins
        with np.errstate(over="ignore", invalid="ignore"):
            v = (b[:, 6] - dir_offset) / period
            dir_dist = np.abs(v - np.round(v))
            rot = (b[:, 6] - dir_offset) - np.floor(v) * period
            yaw = rot + dir_offset + period * label
            b[:, 6] = yaw - np.floor(yaw / (2 * np.pi) + 0.5) * (2 * np.pi)
    t32 = np.float64(np.float32(thr))
    with np.errstate(invalid="ignore"):
        above = score > t32
    if rows is None:
        rows = np.arange(N)
    elif isinstance(rows, str):
        assert rows == "above"
        rows = np.nonzero(above)[0]
    rows = np.asarray(rows, np.int64)
    u, p = _corners(b[rows], order_hwl, T)
    ok, fdist = _extent(p, (6.0, -3.0, 1.0))
    keep = np.zeros(N, bool)
    keep[rows] = above[rows] & ok
    candidates = np.nonzero(keep)[0]
    return dict(score=score, above=above, keep=keep, score_dist=score - t32, dir_dist=dir_dist, rows=rows, corners=p, unprojected=u,
                filter_ok=ok, filter_dist=fdist, candidates=candidates, cand_pos=np.searchsorted(rows, candidates))


def decode_mc_reference(agents, A, nc, thr, order_hwl):
    """agents: list of (cls [A nc, H, W], reg [7A, H, W], anchors [H, W, A, 7], T [4, 4]). Candidates (score > thr) of all agents in
    agent, pixel, anchor order: score, label (1-based; the class sigmoids are compared as float32 values, so saturated classes tie and
    the first wins), corners, unprojected, violation (a size / z filter rejects it), score_dist and class_gap over ALL anchors (for the
    margin assertions) and filter_dist of the candidates."""
    out = dict(score=[], label=[], corners=[], unprojected=[], violation=[], filter_dist=[], score_dist=[], class_gap=[])
    for cls, reg, anchors, T in agents:
        H, W = anchors.shape[:2]
        x = cls.astype(np.float64).reshape(A, nc, H * W).transpose(2, 0, 1).reshape(-1, nc)
        sig = _sigmoid64(x)
        sig32 = sig.astype(np.float32)
        label = np.argmax(sig32, 1)                  # first maximum of the float32 values
        score = sig[np.arange(sig.shape[0]), label]
        if nc > 1:
            srt = np.sort(sig, 1)
            gap = srt[:, -1] - srt[:, -2]
        else:
            gap = np.full(sig.shape[0], np.inf)
        m = score > np.float64(np.float32(thr))
        b = _boxes7(reg, anchors)[m]
        u, p = _corners(b, order_hwl, T)
        ok, fdist = _extent(p, (100.0, -100.0, 100.0))
        out["score"].append(score[m]); out["label"].append(label[m] + 1); out["corners"].append(p); out["unprojected"].append(u)
        out["violation"].append(~ok); out["filter_dist"].append(fdist)
        out["score_dist"].append(score - np.float64(np.float32(thr))); out["class_gap"].append(gap)
    return {k: np.concatenate(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------- quad IoU test families
def bev_quad(cx, cy, l, w, yaw):
    """(4, 2) float32 BEV corners in the corner order of boxes_to_corners_3d (counter-clockwise)."""
    c, s = np.cos(yaw), np.sin(yaw)
    px, py = np.array([1, 1, -1, -1]) * (l / 2), np.array([-1, 1, 1, -1]) * (w / 2)
    return np.stack([px * c - py * s + cx, px * s + py * c + cy], -1).astype(np.float32)


EXACT_FAMILIES = {"identical": 1.0, "shared_edge_corner": 0.0, "degenerate": 0.0, "disjoint": 0.0}
_FAMILY_CACHE = {}


def iou_families(seed=0):
    """name -> (P [n, 4, 2], Q [n, 4, 2]) float32: car-sized boxes with centres out to +-140 m / +-40 m. The families named in
    EXACT_FAMILIES have that IoU exactly (asserted against quad_iou_exact on the CPU); their axis-aligned members sit on multiples of
    1/4 m, so that every product and sum of the area formulas is exact in float64 as well."""
    if seed in _FAMILY_CACHE:
        return _FAMILY_CACHE[seed]
    r = np.random.RandomState(seed)
    fam = {k: ([], []) for k in ("random", "identical", "identical_rolled", "shared_edge_corner", "containment", "crosses",
                                 "near_coincident", "degenerate", "disjoint", "mixed_orientation")}

    def add(name, p, q):
        fam[name][0].append(np.asarray(p, np.float32)); fam[name][1].append(np.asarray(q, np.float32))

    def rand_box():
        return [r.uniform(-140, 140), r.uniform(-40, 40), r.uniform(3.5, 5.5), r.uniform(1.6, 2.2), r.uniform(-np.pi, np.pi)]

    def partner(b):
        return [b[0] + r.normal(0, 1.0), b[1] + r.normal(0, 0.7), b[2] + r.normal(0, 0.2), b[3] + r.normal(0, 0.1), b[4] + r.normal(0, 0.5)]

    far = [(128.5, 32.25), (-139.75, -39.5), (0.0, 0.0), (-64.25, 17.0)]   # exact centres
    for _ in range(200):
        b = rand_box()
        add("random", bev_quad(*b), bev_quad(*partner(b)))
    for _ in range(30):
        b = rand_box()
        add("mixed_orientation", bev_quad(*b)[::-1], bev_quad(*partner(b)))
    for _ in range(10):
        a = bev_quad(*rand_box())
        add("identical", a, a)
        add("identical", a, a[::-1])
        add("identical_rolled", a, np.roll(a, 1, 0))
        add("identical_rolled", a, np.roll(a[::-1], 1, 0))
    for cx, cy in far:
        a = bev_quad(cx, cy, 4.5, 2.0, 0.0)
        add("identical", a, np.roll(a, 1, 0))
        add("identical", a[::-1], np.roll(a, 2, 0))
        for dx, dy in ((4.5, 0), (-4.5, 0), (0, 2.0), (0, -2.0), (4.5, 2.0), (-4.5, 2.0), (4.5, -2.0), (-4.5, -2.0)):
            add("shared_edge_corner", a, bev_quad(cx + dx, cy + dy, 4.5, 2.0, 0.0))
        add("shared_edge_corner", a, bev_quad(cx + 3.25, cy + 1.5, 2.0, 1.0, 0.0)[::-1])     # a smaller box on part of an edge line
        # containment: 2 x 1 in 4 x 2 (1/4), off-centre, rotated inner, both rotated
        big = bev_quad(cx, cy, 4.0, 2.0, 0.0)
        add("containment", big, bev_quad(cx, cy, 2.0, 1.0, 0.0))
        add("containment", bev_quad(cx + 0.75, cy - 0.25, 2.0, 1.0, 0.0), big)
        add("containment", bev_quad(cx + 1.0, cy + 0.5, 2.0, 1.0, 0.0), big)                # inside, touching two edges
        add("containment", big, bev_quad(cx + 0.3, cy - 0.1, 2.0, 1.0, 0.4))
        yaw = r.uniform(-np.pi, np.pi)
        add("containment", bev_quad(cx, cy, 5.0, 2.2, yaw), bev_quad(cx + 0.2, cy + 0.1, 3.0, 1.2, yaw))
        add("containment", bev_quad(cx, cy, 3.0, 1.2, yaw + 0.2), bev_quad(cx, cy, 6.0, 4.0, yaw))
        # crosses
        add("crosses", bev_quad(cx, cy, 4.0, 1.0, 0.0), bev_quad(cx, cy, 1.0, 4.0, 0.0))    # 1/7
        add("crosses", bev_quad(cx, cy, 2.0, 2.0, 0.0), bev_quad(cx, cy, 2.0, 2.0, np.pi / 4))
        add("crosses", bev_quad(cx, cy, 4.5, 2.0, yaw), bev_quad(cx, cy, 4.5, 2.0, yaw + np.pi / 2))
        add("crosses", bev_quad(cx, cy, 2.0, 2.0, yaw), bev_quad(cx, cy, 2.0, 2.0, yaw + np.pi / 4)[::-1])
        # degenerate
        norm = bev_quad(cx, cy, 4.5, 2.0, 0.0)
        for zw in (bev_quad(cx, cy, 4.5, 0.0, 0.0), bev_quad(cx + 0.5, cy, 0.0, 2.0, 0.0), bev_quad(cx, cy, 0.0, 0.0, 0.0)):
            add("degenerate", zw, norm); add("degenerate", norm, zw); add("degenerate", zw, zw)
        # disjoint
        add("disjoint", norm, bev_quad(cx + 4.75, cy, 4.5, 2.0, 0.0))                        # 0.25 m gap
        add("disjoint", norm, bev_quad(cx, cy + 2.25, 4.5, 2.0, 0.0)[::-1])
        add("disjoint", norm, bev_quad(cx + 30.0, cy - 11.0, 4.5, 2.0, 1.0))
        add("disjoint", bev_quad(cx, cy, 4.5, 2.0, 0.5), bev_quad(cx + 4.0 * np.cos(0.5 + np.pi / 2), cy + 4.0 * np.sin(0.5 + np.pi / 2), 4.5, 2.0, 0.5))
        add("disjoint", bev_quad(cx, cy, 4.5, 2.0, 0.5), bev_quad(cx + 3.2, cy - 2.6, 4.5, 2.0, -0.9))
    for k in range(8):
        b = rand_box() if k >= 2 else [far[k][0], far[k][1], 4.5, 2.0, 0.0]
        a = bev_quad(*b)
        for dyaw in (1e-7, 1e-6, 1e-5, 1e-4, 1e-3):
            add("near_coincident", a, bev_quad(b[0], b[1], b[2], b[3], b[4] + dyaw))
        for i, sh in enumerate((1e-5, 1e-4, 1e-3)):
            dx, dy = [(sh, 0), (0, sh), (sh, -sh)][(i + k) % 3]
            add("near_coincident", a, bev_quad(b[0] + dx, b[1] + dy, b[2], b[3], b[4]))
    # rotated degenerate boxes: zero width / zero size at an angle (the two corner pairs coincide in float32)
    for _ in range(4):
        b = rand_box()
        zw, zs, norm = bev_quad(b[0], b[1], b[2], 0.0, b[4]), bev_quad(b[0], b[1], 0.0, 0.0, b[4]), bev_quad(*b)
        for z in (zw, zs):
            add("degenerate", z, norm); add("degenerate", norm, z); add("degenerate", z, z)
    out = {k: (np.stack(p), np.stack(q)) for k, (p, q) in fam.items()}
    _FAMILY_CACHE[seed] = out
    return out


_YARD_CACHE = {}


def iou_yardsticks(seed=0):
    """name -> (exact [n] float64 (rounded once from the Fraction), r64: worst |oracle.detect_port.quad_iou - exact| of the family)."""
    if seed in _YARD_CACHE:
        return _YARD_CACHE[seed]
    from oracle import detect_port as D
    out = {}
    for name, (P, Q) in iou_families(seed).items():
        ex = [quad_iou_exact(p, q) for p, q in zip(P, Q)]
        r64 = max(abs(Fraction(float(D.quad_iou(p, q))) - e) for p, q, e in zip(P, Q, ex))
        out[name] = (np.array([float(e) for e in ex]), float(r64), ex)
    _YARD_CACHE[seed] = out
    return out
