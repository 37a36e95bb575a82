"""Keypoint utilities under the reference's names (lib/utils/keypoints.py).

heatmaps_to_keypoints is the device kernel (ops.heatmaps_to_keypoints ->
vd_heatmaps_to_keypoints): the reference copies every detection's heatmaps to the
host, cv2.resize's them bicubically to the box's pixel size, softmaxes and
argmaxes them in a Python loop; here one launch decodes all of them and the
resized maps are never written.

nms_oks / compute_oks (keypoints.py:225-266) are device kernels too
(ops.nms_oks_frames -> vd_nms_oks_frames, ops.compute_oks -> vd_compute_oks): the
reference's per-frame numpy loop becomes a score, a rank, a suppression bitmask
and a greedy pass in one workgroup per frame.  Rows are processed in descending
mean logit, the higher index first among equal scores; NaN logits are unsupported.
The pipeline's switch is KeypointFramePipeline(nms_oks=...): the config key
KRCNN.NMS_OKS itself is still rejected by load_cfg (config.UNSUPPORTED).

flip_heatmaps (keypoints.py:90-100) is the one-view case of the kernel that combines
the TEST.KPS_AUG views inside the decode (ops.heatmaps_to_keypoints_aug ->
vd_heatmaps_to_keypoints_aug, engine.KeypointAugFramePipeline)."""
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


def flip_permutation():
    """get_keypoints()'s flip map as channel indices: flipped channel k is channel
    perm[k] (each left keypoint swapped with its right one, the nose kept)."""
    names, flip = get_keypoints()
    perm = list(range(len(names)))
    for left, right in flip.items():
        l, r = names.index(left), names.index(right)
        perm[l], perm[r] = r, l
    return perm


def flip_heatmaps(heatmaps, device="cuda"):
    """keypoints.py:90-100: heatmaps [R,17,M,M] flipped horizontally -- the left/right
    channels swapped and the last axis reversed -- by the device kernel
    (vd_heatmaps_to_keypoints_aug with the one view flipped; its combined map is the
    result).  Tensors in, tensor out; numpy in, numpy out."""
    h, as_numpy = _as_f32(heatmaps, "heatmaps",
                          lambda t: t.dim() == 4 and t.shape[1] == len(_KEYPOINTS)
                          and t.shape[2] == t.shape[3], "R x %d x M x M" % len(_KEYPOINTS))
    h = _on_device(h, device)
    boxes = torch.zeros((h.shape[0], 4), dtype=torch.float32, device=h.device)
    _, flipped = ops.heatmaps_to_keypoints_aug([h], [True], [False], [False], boxes,
                                               heur="HM_MAX", want_combined=True)
    return flipped.cpu().numpy() if as_numpy else flipped


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


def _as_f32(a, name, shape_ok, shape_text):
    """(float32 tensor, whether the input was not a tensor); ValueError naming the
    argument when its shape is not `shape_text` -- checked before any device work."""
    as_numpy = not isinstance(a, torch.Tensor)
    t = torch.as_tensor(np.ascontiguousarray(a, np.float32)) if as_numpy else a
    if not shape_ok(t):
        raise ValueError("%s must be %s, got %s" % (name, shape_text, tuple(t.shape)))
    return t, as_numpy


def _on_device(t, device):
    return (t if t.is_cuda else t.to(device)).float().contiguous()


def nms_oks(kp_predictions, rois, thresh, device="cuda"):
    """keypoints.py:225-240: kp_predictions [n,4,17] rows (x, y, logit, prob), rois
    [n,>=4] -> the kept row indices in descending mean logit (ties: the higher index
    first).  numpy in, a Python list of ints out; tensors in, an int64 tensor on the
    device with no host read.  n <= 512."""
    kp, as_numpy = _as_f32(kp_predictions, "kp_predictions",
                           lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (4, ops.OKS_K),
                           "n x 4 x %d" % ops.OKS_K)
    n = kp.shape[0]
    r, _ = _as_f32(rois, "rois", lambda t: t.dim() == 2 and t.shape[0] == n and t.shape[1] >= 4,
                   "%d x >=4" % n)
    if n > ops.OKS_MAX_D:
        raise ValueError("kp_predictions: n = %d, OKS NMS supports n <= %d" % (n, ops.OKS_MAX_D))
    kp = _on_device(kp, device)
    r = _on_device(r, kp.device)
    if n == 0:
        return [] if as_numpy else torch.empty((0,), dtype=torch.int64, device=kp.device)
    dets = torch.zeros((1, n, 5), dtype=torch.float32, device=kp.device)
    dets[0, :, :4] = r[:, :4]
    res = ops.nms_oks_frames(
        kp, dets, torch.ones((1, n), dtype=torch.int32, device=kp.device),
        torch.full((1,), n, dtype=torch.int32, device=kp.device), float(thresh))
    if as_numpy:
        return [int(i) for i in res.keep[0, :int(res.counts[0])].cpu()]
    # tensors in: the kept indices are keep's entries >= 0, already in kept order --
    # selected by a mask on the device, the count is not read here
    k = res.keep[0]
    return k[k >= 0].to(torch.int64)


def compute_oks(src_keypoints, src_roi, dst_keypoints, dst_roi=None, device="cuda"):
    """keypoints.py:243-266: src_keypoints [4,17], src_roi [>=4], dst_keypoints
    [N,4,17] -> the N OKS values in float64 (dst_roi is unused, as in the reference).
    numpy in, numpy out; tensors in, a device tensor out."""
    s, as_numpy = _as_f32(src_keypoints, "src_keypoints",
                          lambda t: tuple(t.shape) == (4, ops.OKS_K), "4 x %d" % ops.OKS_K)
    b, _ = _as_f32(src_roi, "src_roi", lambda t: t.numel() >= 4 and t.numel() == t.shape[-1],
                   "a vector of >= 4")
    d, _ = _as_f32(dst_keypoints, "dst_keypoints",
                   lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (4, ops.OKS_K),
                   "N x 4 x %d" % ops.OKS_K)
    s = _on_device(s, device)
    out = ops.compute_oks(s, _on_device(b, s.device).reshape(-1), _on_device(d, s.device))
    return out.cpu().numpy() if as_numpy else out
