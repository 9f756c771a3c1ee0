"""V2X-Real multi-class detection tail, CPU side: anchors against the reference's generate_anchor_box_v2xreal
(tests/golden/postproc_v2xreal.npz, written by tools/make_golden_postproc_v2xreal.py), and the torch-CPU restatement the GPU tests
use (tests/v2xreal_restatement.py) against the reference's post_process_v2xreal outputs."""
import copy
import hashlib
import json

import numpy as np
import pytest

import v2xreal_restatement as R
from helpers import load_case


def _pp(params):
    from gencomm_amd.postprocess import VoxelPostprocessor
    return VoxelPostprocessor(params, train=False, class_names=R.CLASS_NAMES)


def test_anchor_boxes_v2xreal_match_reference():
    g = load_case("postproc_v2xreal")
    anchors, napl = _pp(json.loads(str(g["params"]))).generate_anchor_box_v2xreal()
    assert napl == [2, 2, 2]
    assert len(anchors) == 3 and all(a.dtype == np.float64 for a in anchors)
    np.testing.assert_array_equal(np.stack(anchors), g["anchors"])


def test_anchor_boxes_v2xreal_at_the_shipped_grid_match_reference_hash():
    g = load_case("postproc_v2xreal")
    params = copy.deepcopy(json.loads(str(g["params"])))
    rng = [-102.4, -51.2, -15.0, 102.4, 51.2, 15.0]   # hypes_yaml/v2xreal: 0.4 m voxels (512 x 256), feature_map_stride 4
    params["gt_range"] = rng
    params["anchor_args"].update(cav_lidar_range=rng, W=512, H=256)
    anchors, napl = _pp(params).generate_anchor_box_v2xreal()
    assert napl == [2, 2, 2] and [a.shape for a in anchors] == [(64, 128, 2, 7)] * 3
    h = hashlib.sha256()
    for a in anchors:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    assert h.hexdigest() == str(g["anchors_sha256_shipped"])


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_restatement_matches_reference(tag):
    g = load_case("postproc_v2xreal")
    params, data, out, projection = R.case_dicts(g, tag)
    boxes, score_labels = R.post_process_v2xreal(params, data, out, projection)
    np.testing.assert_array_equal(score_labels.numpy(), g[f"score_labels_{tag}"])
    np.testing.assert_allclose(boxes.numpy(), g[f"boxes_{tag}"], rtol=0, atol=1e-5)


def test_restatement_assert_and_empty_cases():
    g = load_case("postproc_v2xreal")
    assert bool(g["raises_e"]) and bool(g["none_f"])
    params, data, out, projection = R.case_dicts(g, "e")
    with pytest.raises(AssertionError):
        R.post_process_v2xreal(params, data, out, projection)
    params, data, out, projection = R.case_dicts(g, "f")
    assert R.post_process_v2xreal(params, data, out, projection) == (None, None)
