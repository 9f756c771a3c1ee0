#!/usr/bin/env python3
"""Golden fixture of the batched lidar front end, from the reference's own code (run on the CPU).

Runs only where the reference checkout is mounted (build container), never on the GPU machine:

    python tools/make_golden_lidar_frontend.py      # writes tests/golden/lidar_frontend.npz

Per agent the reference's dataset does shuffle_points -> mask_ego_points -> project_points_by_matrix_torch -> preprocess
(opencood/data_utils/datasets/intermediate_heter_fusion_dataset.py:443-471) and ``SpVoxelPreprocessor.collate_batch`` pads the agent
index in front of (z, y, x). This script runs the reference's ``mask_ego_points`` (pcd_utils.py:70), ``project_points_by_matrix_torch``
(box_utils.py:1169) and ``SpVoxelPreprocessor.collate_batch_list`` / ``collate_batch_dict`` (sp_voxel_preprocessor.py:110-174) with the
import route of oracle/make_golden.py (``_install_stubs``). spconv is absent, so the voxeliser between the projection and the collate is
the C restatement ``gc_oracle_points_to_voxel`` (oracle/csrc/detect_port.c), as in tests/test_iou3d_voxel.py. ``mask_points_by_range``
(pcd_utils.py:41) is used as a cross-check: every point strictly inside the range lands in a voxel row or is cut by a cap.

The shuffle is a stored permutation (the reference draws it with np.random.permutation). Stored per case: points [N, F], offsets [A + 1],
transforms [A, 4, 4] float32, perm [N]; the reference's masked and projected points per agent (ref_points, ref_offsets) and the collated
voxel_coords [M, 4] / voxel_num_points [M]. The voxel features are not stored (they are the oracle's, which the GPU test calls itself).

torch's CPU matmul evaluates the projection of MORE THAN 16 points as a fused multiply-add chain over k and of fewer points with
separate multiplies and adds; real clouds have tens of thousands of points, so every projected agent here keeps more than 16 points
(asserted), and tests/lidar_frontend_restatement.py restates the fused chain (asserted bit-equal here).
"""
from __future__ import annotations

import json
import os
import sys

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import numpy as np

import lidar_frontend_restatement as R

OUT = os.path.join(REPO, "tests", "golden", "lidar_frontend.npz")
SEED = 7100
PILLAR = {"range": [-12.8, -6.4, -3.0, 12.8, 6.4, 1.0], "voxel_size": [0.4, 0.4, 4.0], "max_points": 32, "max_voxels": 4000}   # 64 x 32 x 1
SECOND = {"range": [-12.8, -6.4, -3.0, 12.8, 6.4, 1.0], "voxel_size": [0.4, 0.4, 0.5], "max_points": 5, "max_voxels": 4000}    # 64 x 32 x 8


def cloud(rng, n, F, lo=(-14.0, -7.5, -3.5), hi=(14.0, 7.5, 1.5), near=0.15):
    """n points over slightly more than the range; a share `near` of them around the ego vehicle so that the ego mask bites."""
    p = rng.uniform(lo, hi, size=(n, 3))
    k = int(n * near)
    p[:k] = rng.uniform((-3.0, -1.8, -2.0), (4.0, 1.8, 0.5), size=(k, 3))
    rng.shuffle(p)
    return np.concatenate([p, rng.uniform(0, 1, size=(n, F - 3))], axis=1).astype(np.float32)


def pose(rng, shift=3.0, tilt=0.02):
    yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rot = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    t = np.eye(4)
    t[:3, :3], t[:3, 3] = rot, rng.uniform(-shift, shift, size=3) * (1, 1, 0.05)
    return t.astype(np.float32)


def cells(rng, centres, per_cell, F, jitter=0.15):
    """`per_cell` points around each cell centre, interleaved so that the cells' first points come in the order of `centres`."""
    c = np.asarray(centres, np.float64)
    p = np.repeat(c[None], per_cell, axis=0) + rng.uniform(-jitter, jitter, size=(per_cell, len(c), 3)) * (1, 1, 3)
    p = p.reshape(-1, 3)
    return np.concatenate([p, rng.uniform(0, 1, size=(len(p), F - 3))], axis=1).astype(np.float32)


def centre(ix, iy, cfg=PILLAR):
    r, v = cfg["range"], cfg["voxel_size"]
    return (r[0] + (ix + 0.5) * v[0], r[1] + (iy + 0.5) * v[1], -1.0)


def make_cases():
    rng = np.random.default_rng(SEED)
    f32, nx = np.float32, np.nextafter
    cases = {}

    def add(name, cfg, agents, transforms=False, perm=False, mask_ego=True, **over):
        meta = dict(cfg, **over)
        meta.update(transforms=bool(transforms), perm=bool(perm), mask_ego=bool(mask_ego), F=int(agents[0].shape[1]))
        offs = np.cumsum([0] + [len(a) for a in agents]).astype(np.int32)
        arrays = {"points": np.concatenate(agents).astype(np.float32), "offsets": offs,
                  "transforms": np.stack([pose(rng) for _ in agents]) if transforms else np.zeros((0, 4, 4), np.float32),
                  "perm": np.concatenate([offs[i] + rng.permutation(len(a)) for i, a in enumerate(agents)]).astype(np.int32) if perm
                  else np.zeros(0, np.int32)}
        cases[name] = (meta, arrays)

    add("single", PILLAR, [cloud(rng, 700, 4)], transforms=True, perm=True)
    add("ragged5", PILLAR, [cloud(rng, n, 4) for n in (400, 130, 257, 64, 513)], transforms=True, perm=True)
    add("empty_agent", PILLAR, [cloud(rng, 200, 4), np.zeros((0, 4), np.float32), cloud(rng, 150, 4)], transforms=True)
    inside = np.concatenate([rng.uniform((-1.9, -1.0, -2), (2.9, 1.0, 0), size=(80, 3)), rng.uniform(0, 1, size=(80, 1))], axis=1).astype(np.float32)
    add("ego_only_agent", PILLAR, [cloud(rng, 150, 4), inside, cloud(rng, 120, 4)], perm=True)
    outside = cloud(rng, 90, 4, lo=(13.0, 6.5, -3.5), hi=(20.0, 9.0, 1.5), near=0.0)
    add("out_of_range_agent", PILLAR, [outside, cloud(rng, 140, 4)], mask_ego=False)
    few = [centre(40 + i, 5) for i in range(4)]
    many = [centre(int(ix), int(iy)) for ix, iy in zip(rng.permutation(20) + 40, rng.integers(0, 32, 20))]
    add("cap_voxels", PILLAR, [cells(rng, few, 3, 4), cells(rng, many, 2, 4), cells(rng, few[:3], 4, 4)], max_voxels=7)
    add("cap_points", PILLAR, [cells(rng, many[:6], 5, 4), cells(rng, few, 5, 4)], max_points=3)
    ex, ey = (f32(-1.95), f32(2.95)), (f32(-1.1), f32(1.1))
    edge = [(ex[0], 0.3), (ex[1], -0.3), (0.5, ey[0]), (0.5, ey[1]), (ex[0], ey[0]), (ex[1], ey[1]),                       # on the box: removed
            (nx(ex[0], f32(-9)), 0.3), (nx(ex[1], f32(9)), -0.3), (0.5, nx(ey[0], f32(-9))), (0.5, nx(ey[1], f32(9))),    # one ulp outside: kept
            (nx(ex[0], f32(9)), 0.3), (nx(ex[1], f32(-9)), -0.3), (0.5, nx(ey[0], f32(9))), (0.5, nx(ey[1], f32(-9)))]    # one ulp inside: removed
    edge = np.array([(x, y, -1.0, 0.5) for x, y in edge], np.float32)
    add("ego_edges", PILLAR, [edge, edge[::-1].copy()])
    r = [f32(v) for v in PILLAR["range"]]
    border = [(r[0], 0.1, -1), (nx(r[0], f32(-99)), 0.1, -1), (r[3], 0.1, -1), (nx(r[3], f32(-99)), 0.1, -1),              # the floor rule decides
              (5.1, r[1], -1), (5.1, nx(r[1], f32(-99)), -1), (5.1, r[4], -1), (5.1, nx(r[4], f32(-99)), -1),
              (7.3, 2.2, r[2]), (7.3, 2.2, nx(r[2], f32(-99))), (7.3, 2.2, r[5]), (7.3, 2.2, nx(r[5], f32(-99))),
              (f32(-12.4), f32(-6.0), -1), (f32(0.4) * f32(3), f32(0.4) * f32(7), -1)]                                     # interior cell borders
    border = np.array([p + (0.25,) for p in border], np.float32)
    add("range_edges", PILLAR, [border, border[::-1].copy()], mask_ego=False)
    add("five_features", PILLAR, [cloud(rng, 300, 5), cloud(rng, 200, 5)], transforms=True, perm=True)
    add("several_z", SECOND, [cloud(rng, 500, 4), cloud(rng, 350, 4)], transforms=True)
    add("perm_only", PILLAR, [cloud(rng, 180, 4), cloud(rng, 90, 4)], perm=True, mask_ego=False)
    add("plain", PILLAR, [cloud(rng, 160, 4), cloud(rng, 110, 4)], mask_ego=False)
    return cases


def load_reference():
    from make_golden import _install_stubs
    _install_stubs()
    import types
    for name in ("pypcd", "open3d"):                       # imported by pcd_utils.py for file reading only
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["pypcd"], "pypcd"):
        sys.modules["pypcd"].pypcd = sys.modules["pypcd.pypcd"] = types.ModuleType("pypcd.pypcd")
    sys.path.insert(0, REF)
    from opencood.data_utils.pre_processor.sp_voxel_preprocessor import SpVoxelPreprocessor
    from opencood.utils.box_utils import project_points_by_matrix_torch
    from opencood.utils.pcd_utils import mask_ego_points, mask_points_by_range
    return SpVoxelPreprocessor, project_points_by_matrix_torch, mask_ego_points, mask_points_by_range


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not mounted; the fixture can only be regenerated in the build container")
    import native_port as N
    SP, project, mask_ego_points, mask_points_by_range = load_reference()
    out, meta = {}, {"seed": SEED, "cases": {}}
    worst32 = 0.0
    for name, (m, arr) in make_cases().items():
        pts, offs = arr["points"], arr["offsets"]
        batch, ref_pts = [], []
        for a in range(len(offs) - 1):
            p = pts[offs[a]:offs[a + 1]].copy()
            if m["perm"]:
                p = pts[arr["perm"][offs[a]:offs[a + 1]]].copy()      # shuffle_points with the stored draw
            if m["mask_ego"]:
                p = mask_ego_points(p)
            if m["transforms"]:
                assert len(p) == 0 or len(p) > 16, (name, a, len(p))
                proj = project(p[:, :3], arr["transforms"][a])
                assert proj.dtype == np.float32
                exact = p[:, :3].astype(np.float64) @ arr["transforms"][a].astype(np.float64)[:3, :3].T + arr["transforms"][a].astype(np.float64)[:3, 3]
                if len(p):
                    worst32 = max(worst32, float(np.abs(proj - exact).max()))
                p[:, :3] = proj
            ref_pts.append(p)
            v, c, k = N.points_to_voxel(p, m["voxel_size"], m["range"], m["max_points"], m["max_voxels"])
            strictly_inside = len(mask_points_by_range(p, m["range"]))
            if len(c) < m["max_voxels"] and int(k.max(initial=0)) < m["max_points"]:      # no cap hit: nothing strictly inside is lost
                assert int(k.sum()) >= strictly_inside, name
            batch.append({"voxel_features": v, "voxel_coords": c, "voxel_num_points": k})
        col = SP.collate_batch_list(batch)
        col_d = SP.collate_batch_dict({k: [b[k] for b in batch] for k in batch[0]})
        for k in col:
            assert np.array_equal(col[k].numpy(), col_d[k].numpy()), (name, k)
        mine = R.collate(batch)
        for k in col:
            assert np.array_equal(col[k].numpy(), mine[k]) and col[k].numpy().dtype == mine[k].dtype, (name, k)
        m = dict(m, voxels=int(len(col["voxel_coords"])), voxels_per_agent=[int(len(b["voxel_coords"])) for b in batch])
        meta["cases"][name] = m
        for k, v in arr.items():
            out[f"{name}/{k}"] = v
        out[f"{name}/ref_points"] = np.concatenate(ref_pts).astype(np.float32)
        out[f"{name}/ref_offsets"] = np.cumsum([0] + [len(p) for p in ref_pts]).astype(np.int32)
        out[f"{name}/ref_coords"] = col["voxel_coords"].numpy().astype(np.int32)
        out[f"{name}/ref_num_points"] = col["voxel_num_points"].numpy().astype(np.int32)
    meta["projection_fp32_max_abs_error"] = worst32     # the reference's own float32 error against float64, over every projected point
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **out)
    # the restatement the tests use reproduces what was just written
    for c in R.load_cases():
        got = c.restated_agent_points()
        assert [len(g) for g in got] == list(np.diff(c.ref_offsets)), c.name
        assert np.array_equal(np.concatenate(got).view(np.uint32), c.ref_points.view(np.uint32)), c.name
    n_pts = sum(len(a["points"]) for _, a in make_cases().values())
    print(f"wrote {OUT}: {len(meta['cases'])} cases, {n_pts} points, {os.path.getsize(OUT)} bytes; reference fp32 projection error {worst32:.3e}")
    for name, m in meta["cases"].items():
        print(f"  {name}: voxels per agent {m['voxels_per_agent']}")


if __name__ == "__main__":
    main()
