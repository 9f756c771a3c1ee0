"""torch-CPU restatement of the reference's V2X-Real detection tail (VoxelPostprocessor.post_process_v2xreal,
opencood/data_utils/post_processor/voxel_postprocessor.py:787-943, steps 1-8 of the issue that added it), with the oracle's quad
IoU inside the rotated NMS (oracle/detect_port.py), and the case table of tests/golden/postproc_v2xreal.npz
(tools/make_golden_postproc_v2xreal.py). Written from the formulas; never reads the reference."""
import json

import numpy as np
import torch

from gencomm_amd import synth

CLASS_NAMES = ["vehicle", "pedestrian", "truck"]
VARIANT = {"a": "plain", "b": "plain", "c": "saturate", "d": "plain", "e": "oversize", "f": "empty"}
# tag -> (agents of data_dict, agents of output_dict in its own order, projection)
CASES = {"a": ([0], [0], True), "b": ([0, 1, 2], [2, 0], True), "c": ([1], [1], True), "d": ([1], [1], False),
         "e": ([0], [0], True), "f": ([0], [0], True)}


def case_dicts(g, tag, device="cpu"):
    """(params, data_dict, output_dict, projection) of fixture case `tag`, head maps rebuilt from the stored seed."""
    params = json.loads(str(g["params"]))
    anchors = [a for a in g["anchors"]]
    nc = len(anchors)
    H, W, R = anchors[0].shape[:3]
    in_data, in_out, projection = CASES[tag]
    data, out = {}, {}
    for k in in_data:
        data[f"cav{k}"] = {"transformation_matrix": torch.from_numpy(g["T"][k]).to(device), "anchor_box": anchors,
                           "num_anchors_per_location": [R] * nc}
    for k in in_out:
        cls, reg = synth.make_detection_maps_v2xreal(H, W, nc * R, nc, int(g[f"seed_{tag}"]) + k, variant=VARIANT[tag])
        out[f"cav{k}"] = {"cls_preds": torch.from_numpy(cls).to(device), "reg_preds": torch.from_numpy(reg).to(device)}
    return params, data, out, projection


def post_process_v2xreal(params, data_dict, output_dict, projection=True):
    """(boxes [M, 8, 3], score_labels [M, 2]) or (None, None); AssertionError when the size / z filters would drop a candidate."""
    from oracle import detect_port as D
    thr = params["target_args"]["score_threshold"]
    boxes_l, unproj_l, scores_l, labels_l = [], [], [], []
    for cav_id, cav in data_dict.items():
        if cav_id not in output_dict:
            continue
        out = output_dict[cav_id]
        cls, reg = out["cls_preds"].detach().cpu().float(), out["reg_preds"].detach().cpu().float()
        ab = cav["anchor_box"]
        an = torch.stack([torch.as_tensor(np.asarray(a)) for a in ab]) if isinstance(ab, (list, tuple)) else torch.as_tensor(ab)
        an = an.permute(1, 2, 0, 3, 4).reshape(-1, 7).float()                         # 1. anchor j = class set * R + rotation
        N = an.shape[0]
        prob = torch.sigmoid(cls.permute(0, 2, 3, 1)).reshape(1, N, -1)              # 2. class k of anchor j: channel j nc + k
        score, label = torch.max(prob, dim=-1)
        label = label + 1
        d = reg.permute(0, 2, 3, 1).reshape(1, N, 7)[0]                               # 4. regression channel 7 j + d
        diag = torch.sqrt(an[:, 4] ** 2 + an[:, 5] ** 2)
        b = torch.zeros_like(d)
        b[:, 0:2] = d[:, 0:2] * diag[:, None] + an[:, 0:2]
        b[:, 2] = d[:, 2] * an[:, 3] + an[:, 2]
        b[:, 3:6] = torch.exp(d[:, 3:6]) * an[:, 3:6]
        b[:, 6] = d[:, 6] + an[:, 6]
        m = torch.gt(score[0], thr)                                                   # 3. strict, fp32
        if not bool(m.any()):
            continue
        corners = D.boxes_to_corners_3d(b[m], params["order"])                        # 5.
        T = torch.as_tensor(cav["transformation_matrix"]).detach().cpu().float()
        unproj_l.append(corners.clone())
        boxes_l.append(D.project_box3d(corners, T))
        scores_l.append(score[0][m])
        labels_l.append(label[0][m])
    if not boxes_l:
        return None, None
    boxes, unproj, scores, labels = torch.cat(boxes_l), torch.cat(unproj_l), torch.cat(scores_l), torch.cat(labels_l)
    x_len = boxes[:, :, 0].max(1)[0] - boxes[:, :, 0].min(1)[0]                       # 6. the "z extent" is y's again
    y_len = boxes[:, :, 1].max(1)[0] - boxes[:, :, 1].min(1)[0]
    keep = (x_len <= 100) & (y_len <= 100) & (y_len != 0)
    keep &= (boxes[:, :, 2].min(1)[0] >= -100) & (boxes[:, :, 2].max(1)[0] <= 100)
    assert int(keep.sum()) == boxes.shape[0]
    k = torch.from_numpy(D.nms_rotated(boxes.numpy(), scores.numpy(), params["nms_thresh"]).astype(np.int64))  # 7. top 1000
    boxes, unproj, scores, labels = boxes[k], unproj[k], scores[k], labels[k]
    g = params["gt_range"]
    lo, hi = torch.tensor(g[:2], dtype=torch.float32), torch.tensor(g[3:5], dtype=torch.float32)
    inside = ((boxes[:, :, :2] >= lo) & (boxes[:, :, :2] <= hi)).all(-1).all(-1)     # x and y only
    out_boxes = boxes if projection else unproj                                      # 8.
    return out_boxes[inside], torch.stack([scores[inside], labels[inside].float()], 1)
