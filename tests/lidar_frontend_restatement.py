"""numpy restatement of the reference's per-agent lidar front end (intermediate_heter_fusion_dataset.py:443-471) and of
``SpVoxelPreprocessor.collate_batch``, for the tests of ``SpVoxelPreprocessor.preprocess_batch_device``. Pinned to the reference's own
functions by ``tests/golden/lidar_frontend.npz`` (``tools/make_golden_lidar_frontend.py``; ``tests/test_lidar_frontend.py`` checks that
this file reproduces the fixture exactly). Shared by the CPU and the GPU test; nothing here touches a GPU."""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar_frontend.npz")


def mask_ego_points(points: np.ndarray) -> np.ndarray:
    """pcd_utils.py:84-86 -- the closed box is removed; float32 points against float32-rounded bounds, as numpy compares them."""
    lo_x, hi_x, lo_y, hi_y = np.float32(-1.95), np.float32(2.95), np.float32(-1.1), np.float32(1.1)
    mask = (points[:, 0] >= lo_x) & (points[:, 0] <= hi_x) & (points[:, 1] >= lo_y) & (points[:, 1] <= hi_y)
    return points[np.logical_not(mask)]


def _fma(a, b, c):
    """fused multiply-add of float32 operands: the product is exact in float64; the sum is rounded to float64 and then to float32
    (a double rounding that differs from the fused result only when the float64 sum lands on a float32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def project_points(xyz: np.ndarray, tfm: np.ndarray) -> np.ndarray:
    """box_utils.py:1169 ``project_points_by_matrix_torch`` on float32 points and a float32 4x4 matrix: ``einsum('ik,jk->ij')`` over
    (x, y, z, 1), which torch's CPU matmul evaluates, for more than 16 points, as acc = 0; acc = fma(p_k, T[j][k], acc), k = 0..3."""
    xyz = np.asarray(xyz, dtype=np.float32)
    t = np.asarray(tfm, dtype=np.float32)
    out = np.empty_like(xyz)
    for j in range(3):
        acc = _fma(xyz[:, 0], t[j, 0], np.zeros(len(xyz), np.float32))
        acc = _fma(xyz[:, 1], t[j, 1], acc)
        acc = _fma(xyz[:, 2], t[j, 2], acc)
        out[:, j] = _fma(np.ones(len(xyz), np.float32), t[j, 3], acc)
    return out


def agent_points(points: np.ndarray, tfm, mask_ego: bool, perm=None) -> np.ndarray:
    """shuffle (a given permutation) -> mask_ego_points -> projection of x, y, z: what the dataset hands to ``preprocess``."""
    p = np.array(points, dtype=np.float32, copy=True)
    if perm is not None:
        p = p[perm]
    if mask_ego:
        p = mask_ego_points(p)
    if tfm is not None:
        p = p.copy()
        p[:, :3] = project_points(p[:, :3], tfm)
    return p


def collate(batch: list) -> dict:
    """sp_voxel_preprocessor.py:110-142 ``collate_batch_list``: the agent index in front of (z, y, x), everything concatenated."""
    coords = [np.pad(b["voxel_coords"], ((0, 0), (1, 0)), mode="constant", constant_values=i) for i, b in enumerate(batch)]
    return {"voxel_features": np.concatenate([b["voxel_features"] for b in batch]),
            "voxel_coords": np.concatenate(coords),
            "voxel_num_points": np.concatenate([b["voxel_num_points"] for b in batch])}


def points_to_voxel_dict(points: np.ndarray, voxel_size, lidar_range, max_points: int, max_voxels: int):
    """The voxeliser's sequential definition with a dictionary instead of a dense grid (for grids too large to allocate): voxels in
    order of their first point, points in input order, cell = floor((p - range_min) / voxel_size) in float32."""
    vs, r0 = np.asarray(voxel_size, np.float32), np.asarray(lidar_range[:3], np.float32)
    grid = np.round((np.asarray(lidar_range[3:6], np.float32) - r0) / vs).astype(np.int64)
    F = points.shape[1]
    cells = np.floor((points[:, :3].astype(np.float32) - r0) / vs)
    index, voxels, coords, num = {}, [], [], []
    for i in range(len(points)):
        c = cells[i]
        if not (np.all(c >= 0) and np.all(c < grid.astype(np.float32))):
            continue
        key = (int(c[2]), int(c[1]), int(c[0]))
        v = index.get(key)
        if v is None:
            if len(voxels) >= max_voxels:
                continue
            v = index[key] = len(voxels)
            voxels.append(np.zeros((max_points, F), np.float32)); coords.append(key); num.append(0)
        if num[v] < max_points:
            voxels[v][num[v]] = points[i]
            num[v] += 1
    return (np.stack(voxels) if voxels else np.zeros((0, max_points, F), np.float32),
            np.asarray(coords, np.int32).reshape(-1, 3), np.asarray(num, np.int32))


class Case:
    """One case of the fixture: configuration, inputs and the reference's results."""

    def __init__(self, name: str, meta: dict, z):
        self.name, self.meta = name, meta
        g = lambda k: z[f"{name}/{k}"]
        self.points, self.offsets = g("points"), [int(v) for v in g("offsets")]
        self.A = len(self.offsets) - 1
        self.transforms = g("transforms") if meta["transforms"] else None      # [A, 4, 4] float32
        self.perm = g("perm").astype(np.int64) if meta["perm"] else None       # [N] rows of `points`
        self.mask_ego = bool(meta["mask_ego"])
        self.ref_points, self.ref_offsets = g("ref_points"), [int(v) for v in g("ref_offsets")]
        self.ref_coords, self.ref_num_points = g("ref_coords"), g("ref_num_points")

    def params(self) -> dict:
        m = self.meta
        return {"cav_lidar_range": m["range"], "args": {"voxel_size": m["voxel_size"], "max_points_per_voxel": m["max_points"],
                                                         "max_voxel_train": m["max_voxels"], "max_voxel_test": m["max_voxels"]}}

    def restated_agent_points(self) -> list:
        out = []
        for a in range(self.A):
            lo, hi = self.offsets[a], self.offsets[a + 1]
            rows = self.points[lo:hi] if self.perm is None else self.points[self.perm[lo:hi]]
            out.append(agent_points(rows, None if self.transforms is None else self.transforms[a], self.mask_ego))
        return out


def load_cases() -> list:
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    return [Case(name, m, z) for name, m in meta["cases"].items()]
