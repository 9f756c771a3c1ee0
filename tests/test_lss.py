"""Lift-Splat-Shoot camera encoder (gencomm_amd.lift_splat_shoot), CPU side: parameter tree against the reference's state_dict keys,
frustum and depth bins, the refusals, float64 restatements against tests/golden/lss.npz (made by tools/make_golden_lss.py from the
reference's own code), and the ABI v12 entries' argument checks. No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from lss_restatement import cells64, depth_targets32, geometry64, m4_args, small_args

from gencomm_amd import _lib
from gencomm_amd.lift_splat_shoot import LiftSplatShoot

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSS_ENTRIES = ("gencomm_lss_workspace_bytes", "gencomm_lss_splat_fwd", "gencomm_lss_depth_target_fwd", "gencomm_maxpool3x3s2_fwd")


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "lss.npz"))


def test_state_dict_keys_and_shapes_match_reference(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "lss_state_dict_keys.json")))
    got = [[k, list(v.shape)] for k, v in LiftSplatShoot(m4_args()).state_dict().items()]
    assert got == want


def test_reference_checkpoint_loads_strict(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "lss_state_dict_keys.json")))
    sd = {k: torch.zeros(shape, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, shape in want}
    LiftSplatShoot(m4_args()).load_state_dict(sd, strict=True)


def test_construction_is_device_agnostic():
    m = LiftSplatShoot(m4_args())
    assert all(p.device.type == "cpu" for p in m.parameters())
    assert m.frustum.device.type == "cpu" and tuple(m.frustum.shape) == (48, 42, 56, 3)


def test_frustum_and_depth_bins_equal_fixture(g):
    m = LiftSplatShoot(small_args())
    assert m.frustum.dtype == torch.float32
    assert np.array_equal(m.frustum.numpy(), g["frustum"])
    assert np.array_equal(m.frustum[:, 0, 0, 2].numpy(), g["depth_bins"])
    assert m.D == 48 and [int(v) for v in m.nx] == [256, 256, 1]


def test_refusals_name_their_cause():
    a = m4_args()
    a["camera_encoder"] = "EfficientNet"
    with pytest.raises(NotImplementedError, match="camera_encoder: EfficientNet"):
        LiftSplatShoot(a)
    a = m4_args()
    a["use_depth_gt"] = True
    with pytest.raises(NotImplementedError, match="use_depth_gt"):
        LiftSplatShoot(a)


def test_grad_enabled_forward_is_refused(g):
    m = LiftSplatShoot(small_args())
    inp = {k: torch.from_numpy(g[k].astype(np.float32)) for k in ("imgs", "rots", "trans", "intrins", "post_rots", "post_trans")}
    with pytest.raises(NotImplementedError, match="encoder_"):
        m({"inputs_m4": inp}, "m4")


def test_float64_geometry_reproduces_fixture_cells(g):
    """The float64 restatement of get_geometry + voxel_pooling's truncation and rank gives the fixture's (fp32 reference) cell of every
    frustum point, except points that sit within rounding distance of a cell boundary."""
    geom = geometry64(g["frustum"], g["rots"], g["trans"], g["intrins"], g["post_rots"], g["post_trans"])
    cell, v = cells64(geom, small_args()["grid_conf"])
    want = g["cell"].astype(np.int64)
    diff = cell != want
    assert diff.sum() <= max(1, int(1e-4 * cell.size)), int(diff.sum())
    if diff.any():
        frac = np.abs(v[diff] - np.round(v[diff]))
        assert (frac.min(axis=1) < 1e-4).all(), frac
    # the fixture exercises both sides: points outside the grid, and the truncation edge (-1, 0) that .long() keeps in cell 0
    assert (want < 0).sum() > 1000 and (want >= 0).sum() > 1000
    assert (((v > -1) & (v < 0)).any(axis=1) & (want >= 0)).sum() > 100


def test_depth_targets_restatement_equals_fixture(g):
    imgs = g["imgs"]
    B, N = imgs.shape[:2]
    got = depth_targets32(imgs[:, :, 3].reshape(B * N, *imgs.shape[3:]), 2, 50, 48, "LID", 8)
    assert np.array_equal(got, g["depth_gt_indices"])


def test_lss_entries_in_header_binding_and_library():
    txt = open(os.path.join(REPO, "include", "gencomm_hip.h")).read()
    raw = ctypes.CDLL(_lib.build())
    for name in LSS_ENTRIES:
        assert name + "(" in txt and name in _lib.EXPORTED_SYMBOLS and hasattr(raw, name), name
    assert "#define GENCOMM_ABI_VERSION 12" in txt and _lib.ABI_VERSION == 12


def test_lss_entries_reject_bad_arguments_with_status_codes():
    _lib.build()
    l = _lib.lib()
    nx = (ctypes.c_int * 3)(256, 256, 1)
    lo = (ctypes.c_float * 3)(-51.2, -51.2, -10.0)
    dx = (ctypes.c_float * 3)(0.4, 0.4, 20.0)
    assert l.gencomm_lss_workspace_bytes(4, 4, 48, 42, 56, 128, nx) > 4 * 4 * 48 * 42 * 56 * 20
    assert l.gencomm_lss_workspace_bytes(0, 4, 48, 42, 56, 128, nx) == -1
    assert l.gencomm_lss_workspace_bytes(4, 4, 48, 42, 56, 128, None) == -1
    assert b"null pointer" in l.gencomm_last_error()
    bad_nx = (ctypes.c_int * 3)(256, 0, 1)
    assert l.gencomm_lss_workspace_bytes(4, 4, 48, 42, 56, 128, bad_nx) == -1
    assert b"bad grid" in l.gencomm_last_error()
    args = [None] * 8 + [lo, dx, nx, 1, 1, 48, 8, 16, 16, None, None, None, 1 << 30, None]
    assert l.gencomm_lss_splat_fwd(*args) == 1
    assert b"null pointer" in l.gencomm_last_error()
    args[11] = 0   # B = 0
    assert l.gencomm_lss_splat_fwd(*args) == 1
    assert b"bad B" in l.gencomm_last_error()
    zero_dx = (ctypes.c_float * 3)(0.4, 0.0, 20.0)
    args[11], args[9] = 1, zero_dx
    assert l.gencomm_lss_splat_fwd(*args) == 1
    assert l.gencomm_lss_depth_target_fwd(None, 4, 4, 64, 128, 8, 1, 2.0, 50.0, 48, None, None, None) == 1
    assert b"null pointer" in l.gencomm_last_error()
    p = ctypes.c_void_p(16)   # never dereferenced: the argument checks fail first
    assert l.gencomm_lss_depth_target_fwd(p, 4, 3, 64, 128, 8, 1, 2.0, 50.0, 48, p, None, None) == 1   # no depth channel
    assert l.gencomm_lss_depth_target_fwd(p, 4, 4, 64, 128, 8, 2, 2.0, 50.0, 48, p, None, None) == 1   # mode
    assert l.gencomm_maxpool3x3s2_fwd(None, None, 1, 64, 32, 32, None) == 1
    assert l.gencomm_maxpool3x3s2_fwd(p, p, 1, 0, 32, 32, None) == 1
    assert b"bad dims" in l.gencomm_last_error()
