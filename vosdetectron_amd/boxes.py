"""Drop-ins for the reference's ``utils.boxes`` NMS entry points (lib/utils/boxes.py:
277-355: nms, soft_nms, box_voting).

``nms(dets, thresh)`` keeps the reference's host signature -- dets an (N, >=5)
float32 ndarray ``[x1, y1, x2, y2, score]``, thresh a float -- and returns the
kept row indices as an int64 ndarray in ascending order (``[]`` for no rows),
with cython_nms.nms semantics (``+1`` areas, fp32 IoU, suppress on
``>= thresh``; lib/utils/cython_nms.pyx:37-87).  The suppression runs on the
device (vd_nms: wave-ballot bitmask + single-wave resolve, nms.hip); the rows go
up and the indices come back because the reference's callers hold ndarrays.
Device tensors are accepted as well and stay on the device.

``soft_nms`` (vd_soft_nms) and ``box_voting`` (vd_box_voting) keep the
reference's signatures and return ndarrays the same way.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def nms(dets, thresh):
    """Apply classic DPM-style greedy NMS (cython_nms semantics) on the device."""
    if isinstance(dets, torch.Tensor):
        if not dets.is_cuda:
            raise NotImplementedError("nms: CPU tensors have no path; pass an ndarray "
                                      "or a device tensor")
        return ops.nms(dets.float().contiguous(), thresh)
    d = np.asarray(dets)
    if d.shape[0] == 0:
        return []
    if d.ndim != 2 or d.shape[1] < 5:
        raise ValueError("dets must be N x >=5, got %s" % (d.shape,))
    t = torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(
        torch.device("cuda", torch.cuda.current_device()))
    return ops.nms(t, thresh).cpu().numpy()


def flip_boxes(boxes, im_width):
    """Flip boxes horizontally (lib/utils/boxes.py:261-266): an (N, 4k) ndarray, or a
    tensor on any device; the arithmetic stays in the boxes' dtype (float32 boxes:
    x1' = (W - x2) - 1 in float32, what the device kernels of the test-time
    augmentation compute)."""
    flipped = boxes.clone() if isinstance(boxes, torch.Tensor) else boxes.copy()
    flipped[:, 0::4] = im_width - boxes[:, 2::4] - 1
    flipped[:, 2::4] = im_width - boxes[:, 0::4] - 1
    return flipped


def aspect_ratio(boxes, aspect_ratio):
    """Perform width-relative aspect ratio transformation (lib/utils/boxes.py:269-274):
    x1, x2 of an (N, 4k) ndarray, or a tensor on any device, times aspect_ratio.  The
    product stays in the boxes' dtype: float32 boxes are multiplied by
    float32(aspect_ratio), what numpy computes for a float32 array times a Python float
    and what the union's aspect-ratio views compute on the device."""
    boxes_ar = boxes.clone() if isinstance(boxes, torch.Tensor) else boxes.copy()
    boxes_ar[:, 0::4] = aspect_ratio * boxes[:, 0::4]
    boxes_ar[:, 2::4] = aspect_ratio * boxes[:, 2::4]
    return boxes_ar


def _dev(d):
    return torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(
        torch.device("cuda", torch.cuda.current_device()))


def soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=0.001, method="linear"):
    """Apply the soft NMS algorithm from https://arxiv.org/abs/1704.04503 (device)."""
    d = np.asarray(dets)
    if d.shape[0] == 0:
        return dets, []
    rows, keep = ops.soft_nms(_dev(d), sigma, overlap_thresh, score_thresh, method)
    return rows.cpu().numpy(), keep.cpu().numpy()


def box_voting(top_dets, all_dets, thresh, scoring_method="ID", beta=1.0):
    """Refine top_dets by voting with all_dets (https://arxiv.org/abs/1505.01749)."""
    t = np.asarray(top_dets)
    if t.shape[0] == 0:
        return t.copy()
    return ops.box_voting(_dev(t), _dev(all_dets), thresh, scoring_method, beta).cpu().numpy()


def dedup_boxes(rois, dedup=0.0625):
    """The DEDUP_BOXES step of im_detect_bbox (lib/core/test.py:132-139) on the device
    (vd_rois_from_boxes): rois an (N, 5) float32 ndarray (column 0 the level, 0 in the
    reference's RoI blob, the box already at the blob's scale) -> (rois[index], index,
    inv_index) as np.unique(hashes, return_index=True, return_inverse=True) gives them:
    the distinct hashes ascending, each by its first row.  dedup == 0 returns the rows
    unchanged with index = inv_index = arange(N).  A restriction against the reference's
    lines: column 0 must be 0 in every row, which is all _get_rois_blob ever writes; the
    kernel takes that column from the frame a row belongs to, so another value raises
    ValueError instead of being hashed."""
    r = np.ascontiguousarray(rois, np.float32)
    if r.ndim != 2 or r.shape[1] != 5:
        raise ValueError("rois must be N x 5, got %s" % (r.shape,))
    N = r.shape[0]
    if N == 0:
        return r.copy(), np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    if np.any(r[:, 0] != 0):
        raise ValueError("dedup_boxes: column 0 (the blob level) must be 0, as _get_rois_blob "
                         "writes it")
    if N > ops.GIVEN_BOXES_CAP:
        raise ValueError("dedup_boxes: %d rows exceed %d per call" % (N, ops.GIVEN_BOXES_CAP))
    dev = torch.device("cuda", torch.cuda.current_device())
    out, ucounts, index, inv_index = ops.rois_from_boxes(
        _dev(r[:, 1:5]).view(1, N, 4), torch.full((1,), N, dtype=torch.int32, device=dev),
        torch.ones((1,), dtype=torch.float64, device=dev), dedup)
    u = int(ucounts.item())
    return (out[0, :u].cpu().numpy(), index[0, :u].cpu().numpy().astype(np.int64),
            inv_index[0, :N].cpu().numpy().astype(np.int64))
