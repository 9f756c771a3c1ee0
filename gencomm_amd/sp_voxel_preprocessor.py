"""``SpVoxelPreprocessor`` -- the reference's point-cloud voxeliser
(``opencood/data_utils/pre_processor/sp_voxel_preprocessor.py:18-85``) without spconv: same constructor arguments
(``preprocess_params`` with ``cav_lidar_range`` and ``args.{voxel_size, max_points_per_voxel, max_voxel_train, max_voxel_test}``,
``train``), same ``preprocess(pcd_np)`` result (``voxel_features [M, max_points, 4]``, ``voxel_coords [M, 3] (z, y, x)``,
``voxel_num_points [M]`` as numpy arrays) and ``grid_size``, on the HIP voxeliser (``csrc/voxel_kernels.h``).
``preprocess_device`` keeps the result on the GPU (no host copy) for callers that feed the PointPillars encoder directly;
``preprocess_batch_device`` takes the raw clouds of all agents of a call (ego mask, optional projection, voxeliser, ``collate_batch``)
and returns ``inputs_m<k>`` on the GPU after one host read (``csrc/voxel_batch_kernels.h``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .runtime import dev_ints, ptr, stream_ptr, workspaces


class SpVoxelPreprocessor:
    def __init__(self, preprocess_params: dict, train: bool, device="cuda:0"):
        self.params = preprocess_params
        self.train = train
        self.device = torch.device(device)
        self.lidar_range = self.params['cav_lidar_range']
        self.voxel_size = self.params['args']['voxel_size']
        self.max_points_per_voxel = self.params['args']['max_points_per_voxel']
        self.max_voxels = self.params['args']['max_voxel_train'] if train else self.params['args']['max_voxel_test']
        grid_size = (np.array(self.lidar_range[3:6]) - np.array(self.lidar_range[0:3])) / np.array(self.voxel_size)
        self.grid_size = np.round(grid_size).astype(np.int64)

    def preprocess_device(self, points: torch.Tensor):
        """points [n, F] float32 on the GPU -> (voxels [M, max_points, F], coords [M, 3] int32 (z, y, x), num_points [M] int32)."""
        if not points.is_cuda:
            raise _lib.GenCommHipError("SpVoxelPreprocessor.preprocess_device needs a device tensor (no CPU fallback)")
        pts = points.contiguous().float()
        n, F = pts.shape
        l = _lib.lib()
        dev = pts.device
        voxels = torch.empty(self.max_voxels, self.max_points_per_voxel, F, dtype=torch.float32, device=dev)
        coords = torch.empty(self.max_voxels, 3, dtype=torch.int32, device=dev)
        npts = torch.empty(self.max_voxels, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = workspaces.get(dev, _lib.check_size(l.gencomm_voxelize_workspace_bytes(n), "gencomm_voxelize_workspace_bytes"), "voxelize")
        vs = (C.c_float * 3)(*[float(v) for v in self.voxel_size])
        rg = (C.c_float * 6)(*[float(v) for v in self.lidar_range])
        _lib.check(l.gencomm_voxelize_fwd(ptr(pts), n, F, vs, rg, int(self.max_points_per_voxel), int(self.max_voxels), ptr(voxels),
                                          ptr(coords), ptr(npts), ptr(count), ptr(ws), ws.numel(), stream_ptr(dev)), "gencomm_voxelize_fwd")
        m = int(count.item())
        return voxels[:m], coords[:m], npts[:m]

    def preprocess_batch_device(self, points, offsets=None, transforms=None, mask_ego=True, perm=None, return_padded=False) -> dict:
        """The lidar front end of all agents of a call in one launch sequence (``csrc/voxel_batch_kernels.h``): per agent the
        reference's ``shuffle_points`` (``perm``, drawn by the caller) -> ``mask_ego_points`` -> ``project_points_by_matrix_torch``
        (``transforms``, the ``proj_first`` case) -> ``preprocess``, then ``collate_batch``.

        ``points``: a list of per-agent ``[n_a, F]`` float32 device tensors, or one concatenated ``[N, F]`` tensor with ``offsets``
        (``A + 1`` ascending integers from 0 to N: a list, or a CPU / device tensor). ``transforms``: ``[A, 4, 4]`` or None.
        ``perm``: ``[N]`` integers or None; logical point ``i`` (the one ``offsets`` speaks of) is row ``perm[i]`` of the
        concatenated points, so agent ``a``'s shuffle is ``offsets[a] + np.random.permutation(n_a)``.

        Returns ``{'voxel_features' [M, max_points, F], 'voxel_coords' [M, 4] int32 (agent, z, y, x), 'voxel_num_points' [M]}`` on
        the device after ONE host read (the total count). ``return_padded=True`` makes no host read: the three tensors keep their
        capacity ``min(A * max_voxels, N)`` (rows past the total are unspecified) and ``'counts'`` ``[A]`` (device int32) is added."""
        if isinstance(points, (list, tuple)):
            if offsets is not None:
                raise ValueError("offsets: not accepted together with a list of per-agent points (the list gives them)")
            if len(points) == 0:
                raise ValueError("points: the list of agents is empty")
            for p in points:
                if p.dim() != 2 or p.shape[1] != points[0].shape[1]:
                    raise ValueError("points: every agent needs a [n, F] tensor with the same F")
            offs = [0]
            for p in points:
                offs.append(offs[-1] + int(p.shape[0]))
            pts_in, off_dev = None, None
        else:
            if points.dim() != 2:
                raise ValueError("points: expected a [N, F] tensor or a list of per-agent [n, F] tensors")
            if offsets is None:
                raise ValueError("offsets: needed with concatenated points")
            pts_in = points
            if isinstance(offsets, torch.Tensor) and offsets.is_cuda:   # stays on the device: only its shape can be checked here
                if offsets.dim() != 1 or offsets.numel() < 2:
                    raise ValueError("offsets: expected A + 1 entries")
                offs, off_dev = None, offsets.to(torch.int32).contiguous()
            else:
                offs = [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
                off_dev = None
                if len(offs) < 2 or offs[0] != 0 or offs[-1] != int(points.shape[0]) or any(b < a for a, b in zip(offs, offs[1:])):
                    raise ValueError(f"offsets: expected A + 1 ascending entries from 0 to N = {int(points.shape[0])}, got {offs}")
        A = len(offs) - 1 if offs is not None else off_dev.numel() - 1
        N = offs[-1] if offs is not None else int(pts_in.shape[0])
        F = int(points[0].shape[1]) if pts_in is None else int(pts_in.shape[1])
        if F < 3:
            raise ValueError("points: rows need at least x, y, z")
        if transforms is not None and tuple(transforms.shape) not in ((A, 4, 4), (A, 16)):
            raise ValueError(f"transforms: expected [{A}, 4, 4], got {list(transforms.shape)}")
        if perm is not None and (perm.dim() != 1 or perm.numel() != N):
            raise ValueError(f"perm: expected [{N}] entries, got {list(perm.shape)}")
        tensors = list(points) if pts_in is None else [pts_in]
        tensors += [t for t in (transforms, perm) if t is not None]
        if not all(t.is_cuda for t in tensors):
            raise _lib.GenCommHipError("SpVoxelPreprocessor.preprocess_batch_device needs device tensors (no CPU fallback)")
        pts = (torch.cat([p.float() for p in points]) if pts_in is None else pts_in.float()).contiguous()
        dev = pts.device
        if off_dev is None:
            off_dev = dev_ints(offs, dev)
        tfm = None if transforms is None else transforms.to(torch.float32).reshape(A, 16).contiguous()
        prm = None if perm is None else perm.to(torch.int32).contiguous()
        l = _lib.lib()
        cap = min(A * int(self.max_voxels), N)
        voxels = torch.empty(cap, self.max_points_per_voxel, F, dtype=torch.float32, device=dev)
        coords = torch.empty(cap, 4, dtype=torch.int32, device=dev)
        npts = torch.empty(cap, dtype=torch.int32, device=dev)
        counts = torch.empty(A + 1, dtype=torch.int32, device=dev)   # [A] per agent, then the total
        ws = workspaces.get(dev, _lib.check_size(l.gencomm_voxelize_batch_workspace_bytes(N, A, int(self.max_voxels)),
                                                 "gencomm_voxelize_batch_workspace_bytes"), "voxelize_batch")
        vs = (C.c_float * 3)(*[float(v) for v in self.voxel_size])
        rg = (C.c_float * 6)(*[float(v) for v in self.lidar_range])
        _lib.check(l.gencomm_voxelize_batch_fwd(ptr(pts), N, F, ptr(off_dev), A, ptr(tfm), ptr(prm), int(bool(mask_ego)), vs, rg,
                                                int(self.max_points_per_voxel), int(self.max_voxels), cap, ptr(voxels), ptr(coords), ptr(npts),
                                                ptr(counts), counts.data_ptr() + 4 * A, ptr(ws), ws.numel(), stream_ptr(dev)),
                   "gencomm_voxelize_batch_fwd")
        if return_padded:
            return {'voxel_features': voxels, 'voxel_coords': coords, 'voxel_num_points': npts, 'counts': counts[:A]}
        m = int(counts[A].item())
        return {'voxel_features': voxels[:m], 'voxel_coords': coords[:m], 'voxel_num_points': npts[:m]}

    def preprocess(self, pcd_np: np.ndarray) -> dict:
        v, c, k = self.preprocess_device(torch.from_numpy(np.ascontiguousarray(pcd_np, dtype=np.float32)).to(self.device))
        return {'voxel_features': v.cpu().numpy(), 'voxel_coords': c.cpu().numpy(), 'voxel_num_points': k.cpu().numpy()}
