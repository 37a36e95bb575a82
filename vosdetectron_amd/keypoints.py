"""Keypoint utilities under the reference's names (lib/utils/keypoints.py).

heatmaps_to_keypoints is the device kernel (ops.heatmaps_to_keypoints ->
vd_heatmaps_to_keypoints): the reference copies every detection's heatmaps to the
host, cv2.resize's them bicubically to the box's pixel size, softmaxes and
argmaxes them in a Python loop; here one launch decodes all of them and the
resized maps are never written.  OKS NMS (nms_oks) is not built
(config.UNSUPPORTED: KRCNN.NMS_OKS)."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .config import cfg

_KEYPOINTS = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder",
              "right_shoulder", "left_elbow", "right_elbow", "left_wrist", "right_wrist",
              "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle")


def get_keypoints():
    """keypoints.py:30-63: the 17 COCO keypoint names and the left -> right flip map."""
    names = list(_KEYPOINTS)
    flip = {n: "right_" + n[len("left_"):] for n in names if n.startswith("left_")}
    return names, flip


def get_person_class_index():
    """keypoints.py:66-68: index of the person class in COCO."""
    return 1


def heatmaps_to_keypoints(maps, rois, device="cuda"):
    """keypoints.py:103-157: maps [R,K,M,M] logits, rois [R,>=4] (x1, y1, x2, y2 in
    image coordinates) -> xy_preds [R,4,K] float32, rows (x, y, logit, prob).  Reads
    cfg.KRCNN.INFERENCE_MIN_SIZE like the reference.  Tensors in, tensor out (on the
    maps' device, no host read); numpy in, numpy out."""
    as_numpy = not isinstance(maps, torch.Tensor)
    m = torch.as_tensor(np.ascontiguousarray(maps, np.float32)) if as_numpy else maps
    r = rois if isinstance(rois, torch.Tensor) else \
        torch.as_tensor(np.ascontiguousarray(rois, np.float32))
    if not m.is_cuda:
        m = m.to(device)
    r = r.to(m.device, torch.float32)
    out = ops.heatmaps_to_keypoints(m.float(), r, int(cfg.KRCNN.INFERENCE_MIN_SIZE))
    return out.cpu().numpy() if as_numpy else out
