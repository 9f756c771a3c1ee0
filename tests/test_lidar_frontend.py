"""Batched lidar front end (``SpVoxelPreprocessor.preprocess_batch_device``): the parts that need no GPU -- the ABI carries the two
entry points, arguments are checked before anything touches a device, and the numpy restatement the GPU test compares with reproduces
the reference's results in ``tests/golden/lidar_frontend.npz`` exactly."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_frontend_restatement as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gencomm_voxelize_batch_workspace_bytes", "gencomm_voxelize_batch_fwd")
PARAMS = {"cav_lidar_range": [-12.8, -6.4, -3, 12.8, 6.4, 1],
          "args": {"voxel_size": [0.4, 0.4, 4], "max_points_per_voxel": 32, "max_voxel_train": 100, "max_voxel_test": 100}}


def _pp(params=PARAMS):
    from gencomm_amd.sp_voxel_preprocessor import SpVoxelPreprocessor
    return SpVoxelPreprocessor(params, train=False)


def test_header_bindings_and_library_carry_the_entry_points():
    import ctypes
    from gencomm_amd import _lib
    header = open(os.path.join(REPO, "include", "gencomm_hip.h")).read()
    _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for sym in SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(raw, sym), sym
    assert _lib.lib().gencomm_abi_version() == 12
    assert hasattr(_pp(), "preprocess_batch_device")


def test_cpu_tensors_are_refused():
    from gencomm_amd import _lib
    pts = torch.zeros(10, 4)
    with pytest.raises(_lib.GenCommHipError):
        _pp().preprocess_batch_device([pts[:6], pts[6:]])
    with pytest.raises(_lib.GenCommHipError):
        _pp().preprocess_batch_device(pts, offsets=[0, 6, 10], transforms=torch.eye(4).repeat(2, 1, 1), return_padded=True)


@pytest.mark.parametrize("kwargs, names", [
    (dict(offsets=[0, 6, 9]), "offsets"),                 # does not end at N
    (dict(offsets=[1, 6, 10]), "offsets"),                # does not start at 0
    (dict(offsets=[0, 7, 6, 10]), "offsets"),             # descending
    (dict(offsets=[10]), "offsets"),                      # no agent
    (dict(), "offsets"),                                  # concatenated points without offsets
    (dict(offsets=[0, 6, 10], transforms=torch.zeros(3, 4, 4)), "transforms"),
    (dict(offsets=[0, 6, 10], transforms=torch.zeros(2, 3, 4)), "transforms"),
    (dict(offsets=[0, 6, 10], perm=torch.arange(9)), "perm"),
])
def test_inconsistent_arguments_name_the_argument(kwargs, names):
    with pytest.raises(ValueError, match=names):
        _pp().preprocess_batch_device(torch.zeros(10, 4), **kwargs)


def test_inconsistent_agent_list_names_the_argument():
    with pytest.raises(ValueError, match="points"):
        _pp().preprocess_batch_device([torch.zeros(3, 4), torch.zeros(3, 5)])
    with pytest.raises(ValueError, match="offsets"):
        _pp().preprocess_batch_device([torch.zeros(3, 4)], offsets=[0, 3])


def test_key_limit_is_a_named_status_error():
    """A * cells at or beyond 2^63 cannot be keyed: a status error that names the limit, raised before any pointer is used."""
    import ctypes as C
    from gencomm_amd import _lib
    l = _lib.lib()
    vs, rg = (C.c_float * 3)(1e-3, 1e-3, 1e-3), (C.c_float * 6)(-1e6, -1e6, -1e3, 1e6, 1e6, 1e3)       # 2e9 x 2e9 x 2e6 cells
    assert l.gencomm_voxelize_batch_fwd(None, 8, 4, None, 2, None, None, 1, vs, rg, 32, 100, 8, None, None, None, None, None, None, 0, None) == 1
    assert b"64-bit keys" in l.gencomm_last_error() and b"2^63" in l.gencomm_last_error()
    assert l.gencomm_voxelize_batch_workspace_bytes(-1, 2, 10) == -1
    assert l.gencomm_voxelize_batch_workspace_bytes(1000, 2, 10) > 0


def test_restatement_reproduces_the_fixture():
    cases = R.load_cases()
    assert len(cases) >= 12
    seen = set()
    for c in cases:
        got = c.restated_agent_points()
        assert [len(g) for g in got] == list(np.diff(c.ref_offsets)), c.name
        np.testing.assert_array_equal(np.concatenate(got).view(np.uint32), c.ref_points.view(np.uint32), err_msg=c.name)
        assert c.ref_coords.shape == (c.meta["voxels"], 4) and c.ref_coords.dtype == np.int32
        for a in range(c.A):                                     # collate layout: agents back to back, index in column 0
            lo = sum(c.meta["voxels_per_agent"][:a])
            assert np.all(c.ref_coords[lo:lo + c.meta["voxels_per_agent"][a], 0] == a), c.name
        seen.add((c.meta["transforms"], c.meta["perm"], c.meta["mask_ego"]))
    assert {(True, True, True), (True, False, True), (False, True, False), (False, False, False)} <= seen


def test_restated_collate_and_dict_voxeliser_agree_with_the_oracle():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import native_port as N
    if N.build(verbose=False) is None:
        pytest.fail("the C oracle could not be built")
    c = next(c for c in R.load_cases() if c.name == "cap_points")
    m, batch = c.meta, []
    for p in c.restated_agent_points():
        v, co, k = N.points_to_voxel(p, m["voxel_size"], m["range"], m["max_points"], m["max_voxels"])
        v2, co2, k2 = R.points_to_voxel_dict(p, m["voxel_size"], m["range"], m["max_points"], m["max_voxels"])
        np.testing.assert_array_equal(co, co2); np.testing.assert_array_equal(k, k2); np.testing.assert_array_equal(v, v2)
        batch.append({"voxel_features": v, "voxel_coords": co, "voxel_num_points": k})
    col = R.collate(batch)
    np.testing.assert_array_equal(col["voxel_coords"], c.ref_coords)
    np.testing.assert_array_equal(col["voxel_num_points"], c.ref_num_points)
    assert int(c.ref_num_points.max()) == 3                       # cells of 5 points cut to max_points = 3
