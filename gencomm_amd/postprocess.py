"""``VoxelPostprocessor`` -- host-side mirror of the reference's detection tail for inference
(opencood/data_utils/post_processor/voxel_postprocessor.py: ``generate_anchor_box`` :68-121, ``post_process``
:1084-1244) and ``bbox_overlaps`` (opencood/utils/box_overlaps.pyx:17-57). SURVEY.md 8f rank 3.

``post_process(data_dict, output_dict)`` takes the reference's dictionaries -- per agent id:
``data_dict[cav]['transformation_matrix']`` (4x4), ``['anchor_box']`` ([H, W, A, 7]);
``output_dict[cav]['cls_preds' | 'reg_preds' | 'dir_preds']`` (also the ``psm / rm / dm`` spellings) -- and returns
``(pred_box3d_tensor [M, 8, 3], scores [M])`` or ``(None, None)``. Sigmoid, score filter, box decoding, direction fix,
corners, projection, the size and z filters, the score sort, the rotated IoU (float64), the greedy suppression and the
range mask all run in the HIP library; the only host round trip is the final read of M (the reference goes through numpy
three times on the same path). Anchor generation is constructor-time numpy, as in the reference.

The V2X-Real multi-class heads (``VoxelPostprocessor(params, class_names=[...])``; ``generate_anchor_box_v2xreal`` :123-186,
``post_process_v2xreal`` :787-943): ``data_dict[cav]['anchor_box']`` is the list of per-class anchor arrays ([H, W, R, 7] each,
or one [nc, H, W, R, 7] array), ``cls_preds`` has A * nc channels (A = nc * R anchors per location, class k of anchor j in
channel j * nc + k), ``reg_preds`` 7 A; the result is ``(pred_box3d [M, 8, 3], score_labels [M, 2])`` (score, 1-based class)
or ``(None, None)``. Class max over the sigmoids, score filter, decoding (no direction fix), corners, projection, the size / z
checks, the class-agnostic rotated NMS and the x/y range mask run in the HIP library, every agent of a call in the same
launches; the only host round trip reads the candidate, kept and filter-violation counts together.

Training side (``generate_label`` :188-310, ``generate_label_v2xreal`` :312-463, ``collate_batch`` / ``collate_batch_v2xreal`` :577-655):
``generate_label_batch(object_bbx_center [B, max_num, 7 | 8], object_bbx_mask [B, max_num], anchors)`` makes ``pos_equal_one``,
``neg_equal_one`` and ``targets`` on the device from the boxes the batch already carries, every sample (and, for V2X-Real, every class)
in two launches of the library (``gencomm_target_assign_fwd``, csrc/target_kernels.h); the anchors' stand-up boxes are prepared once
per anchor array and device. ``generate_label`` / ``generate_label_v2xreal`` are the per-sample calls with the reference's keywords.
Not mirrored: ``iou_preds``, ``generate_pos_region_ranges``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import GenCommHipError
from .runtime import f32c, ptr, require_gpu, stream_ptr


class VoxelPostprocessor:
    def __init__(self, anchor_params: dict, train: bool = False, class_names=None):
        self.params = anchor_params
        self.train = train
        self.anchor_num = self.params["anchor_args"]["num"]
        self._cache = {}
        self._anchor_cache = None
        self._target_cache = []
        if class_names is not None:  # voxel_postprocessor.py:32-66
            cfg = anchor_params["anchor_args"]["anchor_generator_config"]
            self.order = anchor_params["order"]
            self.anchor_generator_config = cfg
            self.anchor_sizes = [c["anchor_sizes"] for c in cfg]
            self.anchor_rotations = [c["anchor_rotations"] for c in cfg]
            self.anchor_heights = [c["anchor_bottom_heights"] for c in cfg]
            self.align_center = [c.get("align_center", False) for c in cfg]
            self.anchor_class_names = [c["class_name"] for c in cfg]
            self.matched_thresholds = {c["class_name"]: c["matched_threshold"] for c in cfg}
            self.unmatched_thresholds = {c["class_name"]: c["unmatched_threshold"] for c in cfg}
            assert len(self.anchor_sizes) == len(self.anchor_rotations) == len(self.anchor_heights)
            self.num_of_anchor_sets = len(self.anchor_sizes)
            self.grid_size = np.array([anchor_params["anchor_args"]["W"], anchor_params["anchor_args"]["H"]])
            self.cav_lidar_range = anchor_params["anchor_args"]["cav_lidar_range"]

    # ------------------------------------------------------------------ anchors (numpy, constructor-time)
    def generate_anchor_box(self) -> np.ndarray:
        a = self.params["anchor_args"]
        W, H = a["W"], a["H"]
        r = [math.radians(e) for e in a["r"]]
        assert self.anchor_num == len(r)
        vh, vw = a["vh"], a["vw"]
        xrange = [a["cav_lidar_range"][0], a["cav_lidar_range"][3]]
        yrange = [a["cav_lidar_range"][1], a["cav_lidar_range"][4]]
        fs = a["feature_stride"] if "feature_stride" in a else 2
        x = np.linspace(xrange[0] + vw, xrange[1] - vw, W // fs)
        y = np.linspace(yrange[0] + vh, yrange[1] - vh, H // fs)
        cx, cy = np.meshgrid(x, y)
        cx = np.tile(cx[..., np.newaxis], self.anchor_num)
        cy = np.tile(cy[..., np.newaxis], self.anchor_num)
        cz = np.ones_like(cx) * -1.0
        w, l, h = np.ones_like(cx) * a["w"], np.ones_like(cx) * a["l"], np.ones_like(cx) * a["h"]
        r_ = np.ones_like(cx)
        for i in range(self.anchor_num):
            r_[..., i] = r[i]
        if self.params["order"] == "hwl":
            return np.stack([cx, cy, cz, h, w, l, r_], axis=-1)
        if self.params["order"] == "lhw":
            return np.stack([cx, cy, cz, l, h, w, r_], axis=-1)
        raise ValueError("Unknown bbx order.")

    def generate_anchor_box_v2xreal(self):
        """Per-class anchors ([ny, nx, R, 7] float64 each) and the anchors per location of each class, as the reference builds
        them (voxel_postprocessor.py:123-186): np.arange with the `+ 1e-5` stop, meshgrid in xy order, `align_center`, sizes
        given as l, w, h and reordered for `order`; rotations are used as given."""
        grid_sizes = [self.grid_size[:2] // c["feature_map_stride"] for c in self.anchor_generator_config]
        all_anchors, num_anchors_per_location = [], []
        rng = self.cav_lidar_range
        for grid_size, anchor_size, anchor_rotation, anchor_height, align_center in zip(
                grid_sizes, self.anchor_sizes, self.anchor_rotations, self.anchor_heights, self.align_center):
            num_anchors_per_location.append(len(anchor_rotation) * len(anchor_size) * len(anchor_height))
            if align_center:
                x_stride = (rng[3] - rng[0]) / grid_size[0]
                y_stride = (rng[4] - rng[1]) / grid_size[1]
                x_offset, y_offset = x_stride / 2, y_stride / 2
            else:
                x_stride = (rng[3] - rng[0]) / (grid_size[0] - 1)
                y_stride = (rng[4] - rng[1]) / (grid_size[1] - 1)
                x_offset, y_offset = 0, 0
            x_shifts = np.arange(rng[0] + x_offset, rng[3] + 1e-5, step=x_stride)
            y_shifts = np.arange(rng[1] + y_offset, rng[4] + 1e-5, step=y_stride)
            z_shifts = np.array(anchor_height)
            num_anchor_size, num_anchor_rotation = len(anchor_size), len(anchor_rotation)
            anchor_rotation = np.array(anchor_rotation)
            anchor_size = np.array(anchor_size)
            x_shifts, y_shifts, z_shifts = np.meshgrid(x_shifts, y_shifts, z_shifts)
            anchors = np.concatenate([x_shifts, y_shifts, z_shifts], axis=-1)
            anchor_size = np.tile(anchor_size.reshape(1, -1, 3), (*anchors.shape[0:2], 1))
            if self.order == "hwl":
                anchor_size = anchor_size[..., [2, 1, 0]]
            elif self.order == "lhw":
                anchor_size = anchor_size[..., [0, 2, 1]]
            else:
                raise ValueError("Unknown bbx order.")
            anchors = np.concatenate((anchors, anchor_size), axis=-1)
            anchors = np.tile(anchors[:, :, None, :], (1, 1, num_anchor_rotation, 1))
            anchor_rotation = np.tile(anchor_rotation.reshape(1, 1, -1, 1), (*anchors.shape[0:2], num_anchor_size, 1))
            all_anchors.append(np.concatenate([anchors, anchor_rotation], axis=-1))
        return all_anchors, num_anchors_per_location

    # ------------------------------------------------------------------ inference tail
    def _buffers(self, device, H, W, A):
        key = (str(device), H, W, A)
        if key not in self._cache:
            l = _lib.lib()
            # every agent of a late-fusion call appends into these buffers: sized for the sort's limit, not for one agent's map
            cap = l.gencomm_nms_max_candidates()
            top = 1000
            ws = max(_lib.check_size(l.gencomm_det_workspace_bytes(H, W, A), "gencomm_det_workspace_bytes"),
                     _lib.check_size(l.gencomm_nms_workspace_bytes(), "gencomm_nms_workspace_bytes"))
            self._cache[key] = dict(
                cap=cap, top=top,
                corners=torch.empty(cap, 8, 3, dtype=torch.float32, device=device), scores=torch.empty(cap, dtype=torch.float32, device=device),
                aidx=torch.empty(cap, dtype=torch.int32, device=device), counts=torch.zeros(2, dtype=torch.int32, device=device),
                out_boxes=torch.empty(top, 8, 3, dtype=torch.float32, device=device), out_scores=torch.empty(top, dtype=torch.float32, device=device),
                out_index=torch.empty(top, dtype=torch.int32, device=device), ws=torch.empty(ws, dtype=torch.uint8, device=device),
                range6=torch.tensor([float(v) for v in self.params["gt_range"]], dtype=torch.float32, device=device))
        return self._cache[key]

    def post_process(self, data_dict, output_dict) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        l = _lib.lib()
        buf = None
        for cav_id in output_dict.keys():
            assert cav_id in data_dict
            cav, out = data_dict[cav_id], output_dict[cav_id]
            cls = out["psm"] if "psm" in out else out["cls_preds"]
            reg = out["rm"] if "rm" in out else out["reg_preds"]
            dirp = out["dm"] if "dm" in out else out.get("dir_preds")
            if "iou_preds" in out:
                raise NotImplementedError("iou_preds rescoring is not part of this build")
            require_gpu(cls, "VoxelPostprocessor.post_process")
            if reg.dim() != 4 or cls.shape[0] != 1:
                raise NotImplementedError("anchor-based heads with batch size 1 (as the reference asserts, :1153)")
            dev = cls.device
            anchors = cav["anchor_box"]
            anchors = torch.as_tensor(anchors).to(device=dev, dtype=torch.float32).contiguous()
            H, W, A = anchors.shape[:3]
            if tuple(cls.shape) != (1, A, H, W) or tuple(reg.shape) != (1, 7 * A, H, W):
                raise ValueError(f"head shapes {tuple(cls.shape)} / {tuple(reg.shape)} do not match anchors {tuple(anchors.shape)}")
            nb = int(self.params["dir_args"]["num_bins"]) if dirp is not None else 0
            T = torch.as_tensor(cav["transformation_matrix"]).to(device=dev, dtype=torch.float32).contiguous()
            st = stream_ptr(dev)
            if buf is None:
                buf = self._buffers(dev, H, W, A)
                buf["counts"].zero_()
            elif buf["corners"].device != dev:
                raise ValueError("all agents of one call must live on the same device")
            cls, reg = f32c(cls), f32c(reg)
            dirp = f32c(dirp) if dirp is not None else None
            _lib.check(l.gencomm_det_decode_fwd(
                ptr(cls), ptr(reg), ptr(dirp), ptr(anchors), ptr(T), H, W, A, nb,
                float(self.params["target_args"]["score_threshold"]),
                float(self.params["dir_args"]["dir_offset"]) if dirp is not None else 0.0,
                1 if self.params["order"] == "hwl" else 0,
                ptr(buf["corners"]), ptr(buf["scores"]), ptr(buf["aidx"]), ptr(buf["counts"][0:1]), buf["cap"],
                ptr(buf["ws"]), buf["ws"].numel(), st), "gencomm_det_decode_fwd")
        if buf is None:
            return None, None
        st = stream_ptr(buf["corners"].device)
        _lib.check(l.gencomm_nms_rotated_fwd(
            ptr(buf["corners"]), ptr(buf["scores"]), ptr(buf["counts"][0:1]), float(self.params["nms_thresh"]), buf["top"],
            ptr(buf["range6"]), ptr(buf["out_boxes"]), ptr(buf["out_scores"]), ptr(buf["out_index"]), ptr(buf["counts"][1:2]),
            ptr(buf["ws"]), buf["ws"].numel(), st), "gencomm_nms_rotated_fwd")
        n_cand, m = (int(v) for v in buf["counts"].tolist())  # the one host synchronisation of the tail
        if n_cand > buf["cap"]:
            raise RuntimeError(f"{n_cand} candidates above the score threshold exceed the capacity {buf['cap']} of the device sort")
        if n_cand == 0:
            return None, None
        return buf["out_boxes"][:m].clone(), buf["out_scores"][:m].clone()

    # ------------------------------------------------------------------ V2X-Real multi-class tail
    def _device_anchors_v2xreal(self, anchor_box, dev) -> torch.Tensor:
        """[H, W, nc * R, 7] float32 on `dev` (the reference's stack -> permute(1, 2, 0, 3, 4) -> view -> .float()). The dataset
        hands the same anchor arrays to every agent of every sample (generated once, intermediate_heter_v2xreal_fusion_dataset.py:59),
        so the device copy of the last arrays seen is kept and reused while the same objects come back; the arrays are treated as
        constants, like the reference's own anchors."""
        parts = list(anchor_box) if isinstance(anchor_box, (list, tuple)) else [anchor_box]
        c = self._anchor_cache
        if c is not None and c[1] == dev and len(c[0]) == len(parts) and all(x is y for x, y in zip(c[0], parts)):
            return c[2]
        if isinstance(anchor_box, (list, tuple)):
            a = torch.stack([torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x.cpu() for x in parts], dim=0)
        else:
            a = torch.as_tensor(anchor_box).cpu()
        if a.dim() != 5 or a.shape[-1] != 7:
            raise ValueError(f"anchor_box: expected per-class [H, W, R, 7] arrays, got a stack of shape {tuple(a.shape)}")
        nc, H, W, R = a.shape[:4]
        t = a.permute(1, 2, 0, 3, 4).reshape(H, W, nc * R, 7).float().contiguous().to(dev)
        self._anchor_cache = (parts, dev, t)
        return t

    def _buffers_v2xreal(self, device):
        key = ("v2xreal", str(device))
        if key not in self._cache:
            l = _lib.lib()
            cap, top = l.gencomm_nms_max_candidates(), 1000
            g = [float(v) for v in self.params["gt_range"]]
            f32 = dict(dtype=torch.float32, device=device)
            self._cache[key] = dict(
                cap=cap, top=top,
                corners=torch.empty(cap, 8, 3, **f32), unprojected=torch.empty(cap, 8, 3, **f32), scores=torch.empty(cap, **f32),
                labels=torch.empty(cap, dtype=torch.int32, device=device),
                counts=torch.zeros(3, dtype=torch.int32, device=device),   # candidates, kept, filter violations
                out_boxes=torch.empty(top, 8, 3, **f32), out_scores=torch.empty(top, **f32),
                out_index=torch.empty(top, dtype=torch.int32, device=device), out_unprojected=torch.empty(top, 8, 3, **f32),
                score_labels=torch.empty(top, 2, **f32),
                ws=torch.empty(_lib.check_size(l.gencomm_nms_workspace_bytes(), "gencomm_nms_workspace_bytes"), dtype=torch.uint8, device=device),
                # get_mask_for_boxes_within_range_torch checks x and y only (box_utils.py:348-380)
                range6=torch.tensor([g[0], g[1], -math.inf, g[3], g[4], math.inf], **f32))
        return self._cache[key]

    def post_process_v2xreal(self, data_dict, output_dict, projection: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        l = _lib.lib()
        agents = []
        dev = None
        A = nc = None
        for cav_id, cav in data_dict.items():
            if cav_id not in output_dict:
                continue
            out = output_dict[cav_id]
            cls = out["psm"] if "psm" in out else out["cls_preds"]
            reg = out["rm"] if "rm" in out else out["reg_preds"]
            require_gpu(cls, "VoxelPostprocessor.post_process_v2xreal")
            if cls.dim() != 4 or reg.dim() != 4 or cls.shape[0] != 1:
                raise NotImplementedError("anchor-based heads with batch size 1 (as the reference asserts, :862)")
            if dev is None:
                dev = cls.device
            elif cls.device != dev or reg.device != dev:
                raise ValueError("all agents of one call must live on the same device")
            anchors = self._device_anchors_v2xreal(cav["anchor_box"], dev)
            H, W, a_loc = anchors.shape[:3]
            k = cls.shape[1] // a_loc
            if A is None:
                A, nc = a_loc, k
            if (a_loc, k) != (A, nc) or tuple(cls.shape) != (1, A * nc, H, W) or tuple(reg.shape) != (1, 7 * A, H, W):
                raise ValueError(f"head shapes {tuple(cls.shape)} / {tuple(reg.shape)} do not match anchors {tuple(anchors.shape)} "
                                 f"with {nc} classes")
            T = torch.as_tensor(cav["transformation_matrix"]).to(device=dev, dtype=torch.float32).contiguous()
            agents.append((f32c(cls), f32c(reg), anchors, T, H, W))
        if not agents:
            return None, None
        n = len(agents)
        P, I = ctypes.c_void_p * n, ctypes.c_int * n
        Hs, Ws = I(*[a[4] for a in agents]), I(*[a[5] for a in agents])
        buf = self._buffers_v2xreal(dev)
        ws_bytes = _lib.check_size(l.gencomm_det_mc_workspace_bytes(Hs, Ws, n, A), "gencomm_det_mc_workspace_bytes")
        if ws_bytes > buf["ws"].numel():
            buf["ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = stream_ptr(dev)
        counts = buf["counts"]
        unproj, out_unproj = (None, None) if projection else (buf["unprojected"], buf["out_unprojected"])
        _lib.check(l.gencomm_det_mc_decode_fwd(
            P(*[ptr(a[0]) for a in agents]), P(*[ptr(a[1]) for a in agents]), P(*[ptr(a[2]) for a in agents]),
            P(*[ptr(a[3]) for a in agents]), Hs, Ws, n, A, nc, float(self.params["target_args"]["score_threshold"]),
            1 if self.params["order"] == "hwl" else 0, ptr(buf["corners"]), ptr(unproj), ptr(buf["scores"]), ptr(buf["labels"]),
            ptr(counts[0:1]), ptr(counts[2:3]), buf["cap"], ptr(buf["ws"]), buf["ws"].numel(), st), "gencomm_det_mc_decode_fwd")
        _lib.check(l.gencomm_nms_rotated_fwd(
            ptr(buf["corners"]), ptr(buf["scores"]), ptr(counts[0:1]), float(self.params["nms_thresh"]), buf["top"],
            ptr(buf["range6"]), ptr(buf["out_boxes"]), ptr(buf["out_scores"]), ptr(buf["out_index"]), ptr(counts[1:2]),
            ptr(buf["ws"]), buf["ws"].numel(), st), "gencomm_nms_rotated_fwd")
        _lib.check(l.gencomm_det_mc_gather_fwd(
            ptr(buf["out_index"]), ptr(counts[1:2]), ptr(buf["out_scores"]), ptr(buf["labels"]), ptr(unproj), buf["cap"], buf["top"],
            ptr(buf["score_labels"]), ptr(out_unproj), st), "gencomm_det_mc_gather_fwd")
        n_cand, m, bad = (int(v) for v in counts.tolist())  # the one host synchronisation of the tail
        if n_cand > buf["cap"]:
            raise RuntimeError(f"{n_cand} candidates above the score threshold exceed the capacity {buf['cap']} of the device sort")
        if n_cand == 0:
            return None, None
        if bad:  # the reference asserts that the size / z filters keep every candidate (voxel_postprocessor.py:908)
            raise AssertionError(f"{bad} of {n_cand} candidates fail remove_large_pred_bbx_v2xreal / remove_bbx_abnormal_z_v2xreal")
        boxes = buf["out_boxes"] if projection else buf["out_unprojected"]
        return boxes[:m].clone(), buf["score_labels"][:m].clone()


    # ------------------------------------------------------------------ training-time target assignment
    _MASK_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3, torch.uint8: 4, torch.bool: 4}

    def _target_anchors(self, anchors, dev):
        """Per class: the float64 anchors [H W R, 7] on `dev` and their float32 stand-up boxes (``gencomm_target_standup_fwd``), made once
        per anchor array (or list of arrays) and device and kept while the same objects come back, as `_device_anchors_v2xreal` keeps its
        upload; the arrays are treated as constants. Returns (anchor tensors, stand-up tensors, H, W, R)."""
        parts = list(anchors) if isinstance(anchors, (list, tuple)) else [anchors]
        for c in self._target_cache:
            if c[1] == dev and len(c[0]) == len(parts) and all(x is y for x, y in zip(c[0], parts)):
                return c[2]
        l = _lib.lib()
        a64, sup, shape = [], [], None
        for x in parts:
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            if t.dim() != 4 or t.shape[-1] != 7:
                raise ValueError(f"anchors: expected [H, W, A, 7] (per class for the multi-class heads), got {tuple(t.shape)}")
            if shape is None:
                shape = tuple(t.shape[:3])
            elif tuple(t.shape[:3]) != shape:
                raise ValueError("every class must have the same [H, W, R] anchor grid")
            t = t.to(device=dev, dtype=torch.float64).contiguous().reshape(-1, 7)
            s = torch.empty(t.shape[0], 4, dtype=torch.float32, device=dev)
            _lib.check(l.gencomm_target_standup_fwd(ptr(t), t.shape[0], 1, ptr(s), stream_ptr(dev)), "gencomm_target_standup_fwd")
            a64.append(t)
            sup.append(s)
        entry = (a64, sup) + shape
        self._target_cache = [(parts, dev, entry)] + self._target_cache[:3]
        return entry

    def _assign_targets(self, boxes, mask, anchors, multiclass, dtype):
        assert self.params["order"] == "hwl", "Currently Voxel only support hwl bbx order."
        if not (torch.is_tensor(boxes) and torch.is_tensor(mask) and boxes.is_cuda and mask.is_cuda):
            raise GenCommHipError("target assignment: gt_box_center and mask must be tensors on the GPU (there is no CPU fallback)")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype: torch.float32 or torch.float64")
        dev = boxes.device
        if mask.device != dev:
            raise ValueError("boxes and mask must live on the same device")
        if boxes.dtype not in (torch.float32, torch.float64):
            boxes = boxes.to(torch.float64)
        if mask.dtype not in self._MASK_DTYPES:
            mask = mask.to(torch.float64)
        boxes, mask = boxes.contiguous(), mask.contiguous()
        if boxes.dim() != 3 or boxes.shape[2] not in (7, 8) or tuple(mask.shape) != tuple(boxes.shape[:2]):
            raise ValueError(f"expected boxes [B, max_num, 7 | 8] and mask [B, max_num], got {tuple(boxes.shape)} / {tuple(mask.shape)}")
        B, max_num, width = boxes.shape
        a64, sup, H, W, R = self._target_anchors(anchors, dev)
        nc = len(a64)
        if multiclass:
            if nc != len(self.anchor_class_names):
                raise ValueError(f"{nc} anchor arrays for {len(self.anchor_class_names)} classes")
            pos_thr = [float(self.matched_thresholds[n]) for n in self.anchor_class_names]
            neg_thr = [float(self.unmatched_thresholds[n]) for n in self.anchor_class_names]
        else:
            if nc != 1:
                raise ValueError("the single-class head takes one [H, W, A, 7] anchor array")
            pos_thr = [float(self.params["target_args"]["pos_threshold"])]
            neg_thr = [float(self.params["target_args"]["neg_threshold"])]
        l = _lib.lib()
        key = ("target_ws", str(dev), B, nc, max_num)
        if key not in self._cache:   # zeroed once here; every call leaves it zeroed
            nbytes = _lib.check_size(l.gencomm_target_assign_workspace_bytes(B, nc, max_num), "gencomm_target_assign_workspace_bytes")
            self._cache[key] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        ws = self._cache[key]
        S = nc * R
        pos = torch.empty(B, H, W, S, dtype=dtype, device=dev)
        neg = torch.empty(B, H, W, R, dtype=dtype, device=dev)
        tgt = torch.empty((B, H, W, S, 7) if multiclass else (B, H, W, 7 * S), dtype=dtype, device=dev)
        P, Dbl = ctypes.c_void_p * nc, ctypes.c_double * nc
        _lib.check(l.gencomm_target_assign_fwd(
            ptr(boxes), int(boxes.dtype == torch.float64), width, ptr(mask), self._MASK_DTYPES[mask.dtype],
            P(*[ptr(t) for t in a64]), P(*[ptr(t) for t in sup]), Dbl(*pos_thr), Dbl(*neg_thr), B, nc, max_num, H * W * R, R,
            int(multiclass), ptr(pos), ptr(neg), ptr(tgt), int(dtype == torch.float64), ptr(ws), ws.numel(), stream_ptr(dev)),
            "gencomm_target_assign_fwd")
        return {"targets": tgt, "pos_equal_one": pos, "neg_equal_one": neg}

    def generate_label_batch(self, object_bbx_center, object_bbx_mask, anchors, num_anchors_per_location=None, dtype=torch.float32):
        """What ``collate_batch`` / ``collate_batch_v2xreal`` return for the B samples of a batch, made on the device:
        ``generate_label_batch(batch['ego']['object_bbx_center'], batch['ego']['object_bbx_mask'], anchors)``. The V2X-Real layout
        (label map [B, H, W, S], targets [B, H, W, S, 7], neg_equal_one [B, H, W, R] of the last class) is chosen when the post-processor
        was built with ``class_names``; otherwise [B, H, W, A], [B, H, W, 7A], [B, H, W, A]."""
        multiclass = hasattr(self, "anchor_class_names")
        if multiclass and num_anchors_per_location is not None:
            parts = list(anchors) if isinstance(anchors, (list, tuple)) else [anchors]
            if [int(x.shape[2]) for x in parts] != [int(v) for v in num_anchors_per_location]:
                raise ValueError("num_anchors_per_location does not match the anchor arrays")
        return self._assign_targets(object_bbx_center, object_bbx_mask, anchors, multiclass, dtype)

    def generate_label(self, **kwargs):
        """generate_label(gt_box_center=[max_num, 7], anchors=[H, W, A, 7], mask=[max_num], dtype=torch.float32) -> pos_equal_one,
        neg_equal_one [H, W, A] and targets [H, W, 7A] on the device (voxel_postprocessor.py:188-310)."""
        assert self.params["order"] == "hwl", "Currently Voxel only support hwl bbx order."
        gt, mask = kwargs["gt_box_center"], kwargs["mask"]
        if torch.is_tensor(gt) and torch.is_tensor(mask):
            gt, mask = gt[None], mask[None]
        out = self._assign_targets(gt, mask, kwargs["anchors"], False, kwargs.get("dtype", torch.float32))
        return {"pos_equal_one": out["pos_equal_one"][0], "neg_equal_one": out["neg_equal_one"][0], "targets": out["targets"][0]}

    def generate_label_v2xreal(self, **kwargs):
        """generate_label_v2xreal(gt_box_center=[max_num, 8], anchors=per-class [H, W, R, 7], num_anchors_per_location=, mask=[max_num],
        dtype=torch.float32) -> the label map pos_equal_one [H, W, S], targets [H, W, S, 7], neg_equal_one [H, W, R] of the last class
        (voxel_postprocessor.py:312-463)."""
        assert self.params["order"] == "hwl", "Currently Voxel only support hwl bbx order."
        gt, mask = kwargs["gt_box_center"], kwargs["mask"]
        if torch.is_tensor(gt) and torch.is_tensor(mask):
            gt, mask = gt[None], mask[None]
        out = self.generate_label_batch(gt, mask, kwargs["anchors"], kwargs.get("num_anchors_per_location"), kwargs.get("dtype", torch.float32))
        return {"pos_equal_one": out["pos_equal_one"][0], "targets": out["targets"][0], "neg_equal_one": out["neg_equal_one"][0]}

    @staticmethod
    def collate_batch(label_batch_list):
        """Stack per-sample label dictionaries of tensors (voxel_postprocessor.py:577-619)."""
        return {k: torch.stack([d[k] for d in label_batch_list]) for k in ("targets", "pos_equal_one", "neg_equal_one")}

    @staticmethod
    def collate_batch_v2xreal(label_batch_list):
        """Stack per-sample label dictionaries of tensors (voxel_postprocessor.py:621-655)."""
        return {k: torch.stack([d[k] for d in label_batch_list]) for k in ("targets", "pos_equal_one", "neg_equal_one")}


def bbox_overlaps(boxes: torch.Tensor, query_boxes: torch.Tensor) -> torch.Tensor:
    """(N, 4), (K, 4) float32 [x1, y1, x2, y2] on the GPU -> (N, K) overlaps, box_overlaps.pyx:17-57."""
    require_gpu(boxes, "bbox_overlaps")
    b, q = f32c(boxes), f32c(query_boxes)
    if b.dim() != 2 or q.dim() != 2 or b.shape[1] != 4 or q.shape[1] != 4:
        raise ValueError("expected (N, 4) and (K, 4)")
    out = torch.zeros(b.shape[0], q.shape[0], dtype=torch.float32, device=b.device)
    _lib.check(_lib.lib().gencomm_bbox_overlaps_fwd(ptr(b), ptr(q), ptr(out), b.shape[0], q.shape[0], stream_ptr(b.device)),
               "gencomm_bbox_overlaps_fwd")
    return out
