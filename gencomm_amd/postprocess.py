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
Not mirrored: the training-time target assignment (``generate_label``, ``generate_label_v2xreal``), ``iou_preds``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .runtime import f32c, ptr, require_gpu, stream_ptr


class VoxelPostprocessor:
    def __init__(self, anchor_params: dict, train: bool = False, class_names=None):
        self.params = anchor_params
        self.train = train
        self.anchor_num = self.params["anchor_args"]["num"]
        self._cache = {}
        self._anchor_cache = None
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
            cap = min(H * W * A, l.gencomm_nms_max_candidates())
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
