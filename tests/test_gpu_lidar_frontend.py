"""``SpVoxelPreprocessor.preprocess_batch_device`` on the GPU: every comparison is bit-exact (the operations are copies and one
float32 projection). Per agent against the single-agent ``preprocess_device`` on the restated masked / projected points, against the C
oracle ``gc_oracle_points_to_voxel``, and against the reference's results in ``tests/golden/lidar_frontend.npz``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import lidar_frontend_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = R.load_cases()
DEV = "cuda:0"


def _pp(params):
    from gencomm_amd.sp_voxel_preprocessor import SpVoxelPreprocessor
    return SpVoxelPreprocessor(params, train=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(c, as_list=False, **kw):
    pts = torch.from_numpy(c.points).to(DEV)
    tfm = None if c.transforms is None else torch.from_numpy(c.transforms).to(DEV)
    perm = None if c.perm is None else torch.from_numpy(c.perm).to(DEV)
    if as_list:
        assert perm is None
        return _pp(c.params()).preprocess_batch_device([pts[lo:hi] for lo, hi in zip(c.offsets, c.offsets[1:])], transforms=tfm,
                                                       mask_ego=c.mask_ego, **kw)
    return _pp(c.params()).preprocess_batch_device(pts, offsets=c.offsets, transforms=tfm, mask_ego=c.mask_ego, perm=perm, **kw)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    for k in ("voxel_coords", "voxel_num_points", "voxel_features"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what} {k}")


@pytest.fixture(scope="module")
def results():
    """The batched result of every fixture case, computed once."""
    return {c.name: _host(_run(c)) for c in CASES}


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_single_agent_path_per_agent(c, results):
    pp, batch = _pp(c.params()), []
    for p in c.restated_agent_points():
        v, co, k = pp.preprocess_device(torch.from_numpy(p).to(DEV))
        batch.append({"voxel_features": v.cpu().numpy(), "voxel_coords": co.cpu().numpy(), "voxel_num_points": k.cpu().numpy()})
    assert [len(b["voxel_coords"]) for b in batch] == c.meta["voxels_per_agent"]
    _assert_same(results[c.name], R.collate(batch), c.name)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_equals_c_oracle_and_fixture(c, results):
    import native_port as N
    m, got = c.meta, results[c.name]
    batch = []
    for p in c.restated_agent_points():
        v, co, k = N.points_to_voxel(p, m["voxel_size"], m["range"], m["max_points"], m["max_voxels"])
        batch.append({"voxel_features": v, "voxel_coords": co, "voxel_num_points": k})
    _assert_same(got, R.collate(batch), c.name)
    # the reference's collate layout, and its projection: the first point of every voxel is one of the reference's projected points
    np.testing.assert_array_equal(got["voxel_coords"], c.ref_coords)
    np.testing.assert_array_equal(got["voxel_num_points"], c.ref_num_points)
    ref_rows = {r.tobytes() for r in c.ref_points}
    filled = got["voxel_features"][np.arange(m["max_points"])[None, :] < got["voxel_num_points"][:, None]]
    assert len(filled) == int(got["voxel_num_points"].sum()) and all(r.tobytes() in ref_rows for r in filled)


def test_fixture_covers_the_issue_table():
    by = {c.name: c for c in CASES}
    assert by["single"].A == 1 and by["ragged5"].A == 5 and len(set(np.diff(by["ragged5"].offsets))) == 5
    assert 0 in np.diff(by["empty_agent"].offsets)
    assert by["ego_only_agent"].meta["voxels_per_agent"][1] == 0 and by["out_of_range_agent"].meta["voxels_per_agent"][0] == 0
    assert by["cap_voxels"].meta["voxels_per_agent"] == [4, 7, 3] and by["cap_voxels"].meta["max_voxels"] == 7
    assert by["cap_points"].meta["max_points"] == 3
    assert by["five_features"].meta["F"] == 5 and by["several_z"].ref_coords[:, 1].max() > 0
    assert len(by["ego_edges"].ref_points) == 2 * 4                     # of 14 edge points per agent only those one ulp outside stay


def test_list_input_equals_concatenated_input(results):
    for c in CASES:
        if c.perm is None:
            _assert_same(_host(_run(c, as_list=True)), results[c.name], c.name)


def test_device_offsets_and_int64_perm(results):
    c = next(c for c in CASES if c.name == "ragged5")
    pts = torch.from_numpy(c.points).to(DEV)
    out = _pp(c.params()).preprocess_batch_device(pts, offsets=torch.tensor(c.offsets, device=DEV), transforms=torch.from_numpy(c.transforms).to(DEV),
                                                  perm=torch.from_numpy(c.perm).to(DEV).long())
    _assert_same(_host(out), results[c.name], c.name)


def test_workspace_reuse_five_calls_in_a_row(results):
    """Different A and n one after the other on the same workspace (it only grows): nothing of an earlier call leaks into a later one."""
    order = ["ragged5", "cap_voxels", "several_z", "empty_agent", "single", "ego_edges", "ragged5"]
    by = {c.name: c for c in CASES}
    outs = [_run(by[n]) for n in order]                                  # no synchronisation in between but the count read
    for n, o in zip(order, outs):
        _assert_same(_host(o), results[n], n)


def test_two_runs_are_bit_identical():
    c = next(c for c in CASES if c.name == "ragged5")
    a, b = _host(_run(c)), _host(_run(c))
    _assert_same(a, b, "determinism")
    big = _big_case()
    a, b = _host(big()), _host(big())
    _assert_same(a, b, "determinism, many blocks")


def _big_case(n=(30011, 17, 25013), seed=5):
    """More than one block per kernel and more than one radix pass: three agents on the OPV2V pillar grid."""
    rng = np.random.default_rng(seed)
    params = {"cav_lidar_range": [-102.4, -51.2, -3, 102.4, 51.2, 1],
              "args": {"voxel_size": [0.4, 0.4, 4], "max_points_per_voxel": 8, "max_voxel_train": 6000, "max_voxel_test": 6000}}
    agents = [np.concatenate([rng.normal(0, (35, 20, 1), size=(k, 3)) + (0, 0, -1), rng.uniform(0, 1, size=(k, 1))], axis=1).astype(np.float32) for k in n]
    tfm = np.stack([np.eye(4, dtype=np.float32)] * len(n))
    tfm[1, :3, 3], tfm[2, :2, :2] = (3.5, -2.25, 0.1), [[0.6, -0.8], [0.8, 0.6]]
    big = lambda **kw: _pp(params).preprocess_batch_device([torch.from_numpy(a).to(DEV) for a in agents], transforms=torch.from_numpy(tfm).to(DEV), **kw)
    big.params, big.agents, big.tfm = params, agents, tfm
    return big


def test_many_blocks_and_voxel_cap_against_single_agent_path():
    big = _big_case()
    got, pp, batch = _host(big()), _pp(big.params), []
    for p, t in zip(big.agents, big.tfm):
        v, co, k = pp.preprocess_device(torch.from_numpy(R.agent_points(p, t, True)).to(DEV))
        batch.append({"voxel_features": v.cpu().numpy(), "voxel_coords": co.cpu().numpy(), "voxel_num_points": k.cpu().numpy()})
    assert len(batch[0]["voxel_coords"]) == 6000 and len(batch[1]["voxel_coords"]) < 20          # the cap bites for the large agents only
    _assert_same(got, R.collate(batch), "big")


def test_return_padded_makes_no_host_read_and_has_equal_prefix(results):
    for name in ("ragged5", "cap_voxels", "out_of_range_agent"):
        c = next(c for c in CASES if c.name == name)
        out = _run(c, return_padded=True)
        cap = min(c.A * c.meta["max_voxels"], len(c.points))
        assert out["voxel_features"].shape[0] == cap and out["voxel_coords"].shape == (cap, 4) and out["counts"].is_cuda
        counts = out["counts"].cpu().numpy()
        assert counts.tolist() == c.meta["voxels_per_agent"]
        m = int(counts.sum())
        _assert_same({k: v[:m] for k, v in _host(out).items() if k != "counts"}, results[name], name)


def test_empty_call():
    pp = _pp(CASES[0].params())
    out = pp.preprocess_batch_device([torch.zeros(0, 4, device=DEV), torch.zeros(0, 4, device=DEV)], return_padded=True)
    assert out["counts"].cpu().tolist() == [0, 0] and out["voxel_features"].shape == (0, 32, 4)
    assert pp.preprocess_batch_device([torch.zeros(0, 4, device=DEV)])["voxel_coords"].shape == (0, 4)


def test_sixty_four_bit_keys_on_a_grid_too_large_for_32():
    """A * cells = 2 * 70 000^2 = 9.8e9 > 2^32: the call switches to 64-bit keys (the single-agent path refuses this grid). Only the grid's
    sizes are large -- keys are computed, never stored per cell. Compared with the sequential definition on a dictionary."""
    from gencomm_amd import _lib
    rng = np.random.default_rng(11)
    params = {"cav_lidar_range": [0, 0, -2, 700, 700, 2],
              "args": {"voxel_size": [0.01, 0.01, 4], "max_points_per_voxel": 3, "max_voxel_train": 150, "max_voxel_test": 150}}
    agents = []
    for k in (260, 190):
        base = rng.uniform((0, 0, -2.5), (701, 701, 2.5), size=(k // 2, 3))          # far apart, and some outside
        agents.append(np.concatenate([np.concatenate([base, base + rng.uniform(0, 0.004, size=base.shape)]),     # pairs that mostly share a cell
                                      rng.uniform(0, 1, size=(2 * len(base), 1))], axis=1).astype(np.float32))
    pp = _pp(params)
    with pytest.raises(_lib.GenCommHipError, match="32-bit"):
        pp.preprocess_device(torch.from_numpy(agents[0]).to(DEV))
    got = _host(pp.preprocess_batch_device([torch.from_numpy(a).to(DEV) for a in agents], mask_ego=False))
    batch = []
    for a in agents:
        v, co, k = R.points_to_voxel_dict(a, params["args"]["voxel_size"], params["cav_lidar_range"], 3, 150)
        batch.append({"voxel_features": v, "voxel_coords": co, "voxel_num_points": k})
    assert len(batch[0]["voxel_coords"]) > 100 and batch[0]["voxel_num_points"].max() >= 2 and batch[0]["voxel_coords"][:, 1:].max() > 65536
    _assert_same(got, R.collate(batch), "64-bit keys")
