"""Pins tests/detect_reference.py on the CPU: the exact rational quad IoU against closed forms, the float64 vertex enumeration
and the oracle's Sutherland-Hodgman clipping (oracle/detect_port.py quad_iou -- the algorithm the HIP kernel restates) against the exact
one on every family of tests/test_gpu_detect_kernels.py, the NMS reference against the oracle's greedy loop, and the float64 decode
references against the float32 restatements on the committed goldens.

Measured here (worst |error| against quad_iou_exact per family, n pairs):
  family               n    oracle clipping (r64)   float64 enumeration
  random              200   2.2e-13                 3.0e-16
  mixed_orientation    30   2.9e-14                 2.2e-16
  containment          24   6.9e-15                 2.3e-17
  crosses              16   2.3e-13                 1.5e-16
  near_coincident      64   9.0e-14                 4.5e-16
  identical (+rolled)  48   0                       0
  shared_edge_corner   36   0                       0
  disjoint             20   0                       0
  degenerate           60   1.8e-15                 0      (clipping against a ROTATED zero-width box leaves slivers; axis-aligned: 0)
"""
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

import detect_reference as R
from helpers import load_case
from gencomm_amd import synth


def _sq(x0, y0, w, h):
    return np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], np.float32)


def test_quad_iou_exact_closed_forms():
    sq = _sq(0, 0, 2, 2)
    assert R.quad_iou_exact(sq, sq) == 1
    assert R.quad_iou_exact(sq, sq[::-1]) == 1
    assert R.quad_iou_exact(sq, _sq(1, 0, 2, 2)) == Fraction(1, 3)                       # half shift
    assert R.quad_iou_exact(_sq(100, 30, 4, 2), _sq(101, 30.5, 2, 1)) == Fraction(1, 4)  # 2 x 1 inside 4 x 2
    assert R.quad_iou_exact(sq, _sq(2, 0, 2, 2)) == 0                                   # shared edge
    assert R.quad_iou_exact(sq, _sq(2, 2, 2, 2)) == 0                                   # shared corner
    assert R.quad_iou_exact(sq, _sq(0.5, 0.5, 0, 1)) == 0                               # zero width
    assert R.quad_iou_exact(_sq(1, 1, 0, 0), _sq(1, 1, 0, 0)) == 0                      # zero size: the union is 0
    assert R.quad_iou_exact(sq, _sq(5, 5, 2, 2)) == 0
    assert R.quad_iou_exact(_sq(0, 0, 4, 1), _sq(1.5, -1.5, 1, 4)) == Fraction(1, 7)     # 90 degree cross
    # the square against itself turned by 45 degrees: a regular octagon of area 8 (sqrt 2 - 1), up to the float32 corner rounding
    c = np.float64(np.sqrt(2.0))
    diamond = np.array([[1 + c, 1], [1, 1 + c], [1 - c, 1], [1, 1 - c]], np.float32)
    octagon = 8 * (np.sqrt(2.0) - 1)
    assert abs(float(R.quad_iou_exact(sq, diamond)) - octagon / (8 - octagon)) < 4 * 2.0 ** -24
    assert abs(float(R.quad_iou_exact(sq[::-1], np.roll(diamond, 1, 0))) - octagon / (8 - octagon)) < 4 * 2.0 ** -24


def test_quad_iou_f64_matches_exact_on_every_family():
    """Bound: the enumeration shifts the origin to p's first corner, so every shoelace term is at most 8 m x 8 m; at most 24 terms, three
    areas of at least 5.6 m^2 (the smallest box) -> 3 * 24 * 64 * 2^-53 / 5.6 = 1e-13."""
    fam, yard = R.iou_families(), R.iou_yardsticks()
    for name, (P, Q) in fam.items():
        got = R.quad_iou_f64_batch(P, Q)
        err = max(abs(Fraction(float(g)) - e) for g, e in zip(got, yard[name][2]))
        print(f"{name}: float64 enumeration worst error {float(err):.2e}")
        assert err <= 1e-13, name
        if name in R.EXACT_FAMILIES:
            assert (got == R.EXACT_FAMILIES[name]).all(), name
        assert R.quad_iou_f64(P[0], Q[0]) == got[0]


def test_exact_families_are_exact():
    yard = R.iou_yardsticks()
    for name, value in R.EXACT_FAMILIES.items():
        assert all(e == Fraction(value) for e in yard[name][2]), name
    assert all(e == 1 for e in yard["identical_rolled"][2])
    assert yard["containment"][2][0] == Fraction(1, 4) and yard["crosses"][2][0] == Fraction(1, 7)


def test_oracle_quad_iou_against_exact():
    """The yardstick r64 of the GPU test: the clipping algorithm in float64 on unshifted coordinates. Bound from the format: shoelace terms of
    up to 142 m x 42 m, eight per area, relative to 5.6 m^2 -> 8 * 142 * 42 * 2^-53 / 5.6 = 9.5e-13."""
    yard = R.iou_yardsticks()
    for name, (_, r64, _) in yard.items():
        print(f"{name}: r64 {r64:.2e}")
        assert r64 <= 1e-12, name
    for name in ("identical", "identical_rolled", "shared_edge_corner", "disjoint"):
        assert yard[name][1] == 0.0, name
    assert yard["degenerate"][1] <= 1e-14     # slivers of the rotated zero-width clip windows; the exact answer is 0


cluster_scene = R.cluster_scene


@pytest.mark.parametrize("n,thr,top", [(1, 0.15, 1000), (2, 0.15, 1000), (300, 0.15, 1000), (300, 0.6, 1000), (300, 0.15, 100)])
def test_nms_reference_matches_oracle_greedy_loop(n, thr, top):
    from oracle import detect_port as D
    corners, scores = cluster_scene(n, 5 + n)
    kept, undecided = R.nms_reference(corners, scores, thr, top, None, margin=1e-10)
    assert undecided == []
    assert kept.tolist() == D.nms_rotated(corners, scores, thr, top).tolist()
    if n == 300:
        assert 100 <= len(kept) < 300 or top == 100 or thr == 0.6


def test_nms_reference_ties_range_and_margin():
    corners, _ = cluster_scene(6, 1)
    scores = np.array([0.5, 0.5, 0.9, 0.5, 0.5, 0.5], np.float32)       # boxes 0 / 1 and 3 / 4 overlap and tie: the larger index wins
    kept, _ = R.nms_reference(corners, scores, 0.15, 1000)
    assert kept.tolist() == [2, 5, 4, 1]
    hi = corners[..., 0].max()
    r6 = [-1000, -1000, -3, float(corners[4, :, 0].max()), 1000, 1]     # box 4's own x maximum is a bound: inclusive
    kept, _ = R.nms_reference(corners, scores, 0.15, 1000, r6)
    assert 4 in kept.tolist() and all(corners[k, :, 0].max() <= r6[3] for k in kept) and hi > r6[3]
    r6[3] = float(np.nextafter(np.float32(r6[3]), np.float32(-np.inf)))
    kept, _ = R.nms_reference(corners, scores, 0.15, 1000, r6)
    assert 4 not in kept.tolist() and 3 not in kept.tolist()             # the mask comes after the suppression: 4 still removed 3
    # a pair at IoU 1/3 is undecided around float32(1/3)'s rounding boundary only when the margin reaches it
    pair = np.zeros((2, 8, 3), np.float32)
    pair[0, :4, :2] = pair[0, 4:, :2] = _sq(128, 32, 2, 2); pair[1, :4, :2] = pair[1, 4:, :2] = _sq(129, 32, 2, 2)
    third = np.float32(1 / 3)
    assert R.nms_reference(pair, np.array([0.9, 0.8], np.float32), third, 10)[0].tolist() == [0, 1]
    assert R.nms_reference(pair, np.array([0.9, 0.8], np.float32), np.nextafter(third, np.float32(0)), 10)[0].tolist() == [0]
    assert R.nms_reference(pair, np.array([0.9, 0.8], np.float32), third, 10, margin=1e-10)[1] == []
    assert R.nms_reference(pair, np.array([0.9, 0.8], np.float32), third, 10, margin=3e-8)[1] == [(0, 1)]


# ------------------------------------------------------------------------------------------------------------- decoding vs the goldens
def _tail_from_reference(dec, params, mc_range=False):
    """Candidates of a decode reference -> NMS reference -> range mask: what the whole tail returns."""
    g = params["gt_range"]
    r6 = [g[0], g[1], -np.inf, g[3], g[4], np.inf] if mc_range else g
    kept, undecided = R.nms_reference(dec["corners"].astype(np.float32), dec["score"].astype(np.float32), params["nms_thresh"], 1000, r6,
                                      margin=1e-6)
    assert undecided == []   # no decision of these goldens hangs on the float32 corner rounding
    return kept


@pytest.mark.parametrize("tag", ["a", "b"])
def test_decode_reference_matches_oracle_post_process_on_golden(tag):
    from oracle import detect_port as D
    g = load_case("postproc")
    params = json.loads(str(g["params"]))
    H, W, A = int(g["H"]), int(g["W"]), int(g["A"])
    cls, reg, dirp = synth.make_detection_maps(H, W, A, int(g[f"seed_{tag}"]))
    anchors = g["anchors"].astype(np.float32)
    T = g[f"T_{tag}"].astype(np.float32)
    ref = R.decode_reference(cls[0], reg[0], dirp[0], anchors, T, params["dir_args"]["num_bins"], params["target_args"]["score_threshold"],
                             params["dir_args"]["dir_offset"], params["order"] == "hwl")
    assert np.abs(ref["score_dist"]).min() > 1e-6 and ref["dir_dist"][ref["above"]].min() > 1e-5
    assert np.abs(ref["filter_dist"][ref["above"]]).min() > 1e-3
    dec = dict(corners=ref["corners"][ref["cand_pos"]], score=ref["score"][ref["candidates"]])
    kept = _tail_from_reference(dec, params)
    boxes, scores = D.post_process(torch.from_numpy(cls), torch.from_numpy(reg), torch.from_numpy(dirp), torch.from_numpy(g["anchors"]),
                                   torch.from_numpy(g[f"T_{tag}"]), params)
    assert boxes.shape[0] == len(kept) > 5
    np.testing.assert_allclose(dec["score"][kept], scores.numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(dec["corners"][kept], boxes.numpy(), rtol=0, atol=3e-5)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_decode_mc_reference_matches_restatement_on_golden(tag):
    import v2xreal_restatement as V
    g = load_case("postproc_v2xreal")
    params, data, out, projection = V.case_dicts(g, tag)
    agents = []
    for cav_id, cav in data.items():
        if cav_id not in out:
            continue
        an = np.stack([np.asarray(a) for a in cav["anchor_box"]])
        nc, H, W, Rr = an.shape[:4]
        an = an.transpose(1, 2, 0, 3, 4).reshape(H, W, nc * Rr, 7).astype(np.float32)
        agents.append((out[cav_id]["cls_preds"][0].numpy(), out[cav_id]["reg_preds"][0].numpy(), an,
                       cav["transformation_matrix"].numpy().astype(np.float32)))
    A = agents[0][2].shape[2]
    nc = agents[0][0].shape[0] // A
    ref = R.decode_mc_reference(agents, A, nc, params["target_args"]["score_threshold"], params["order"] == "hwl")
    assert not ref["violation"].any() and np.abs(ref["score_dist"]).min() > 1e-6
    kept = _tail_from_reference(ref, params, mc_range=True)
    boxes, sl = V.post_process_v2xreal(params, data, out, projection)
    assert boxes.shape[0] == len(kept) > 5
    np.testing.assert_array_equal(ref["label"][kept], sl[:, 1].numpy())
    np.testing.assert_allclose(ref["score"][kept], sl[:, 0].numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose((ref["corners"] if projection else ref["unprojected"])[kept], boxes.numpy(), rtol=0, atol=3e-5)
    if tag == "c":   # two classes saturated to 1.0f: the first wins
        assert ((ref["score"][kept] >= 1 - 2.0 ** -25) & (ref["label"][kept] == 1)).sum() >= 1
