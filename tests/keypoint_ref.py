"""Restatements the keypoint tests compare against (a helper, not a conftest).

heatmaps_to_keypoints: lib/utils/keypoints.py:103-157 in numpy with the resized
map materialised.  The resize is cv2.resize INTER_CUBIC on float32 as the C ABI
documents it (include/vosdet.h, csrc/keypoints.hip): destination index d reads
f = float32((d + 0.5) * (M / dst) - 0.5) with the scale and the product in float64,
s = floor(f), t = f - s, taps s-1 .. s+2 clamped to the map, the A = -0.75 cubic
weights in float32, rows first and then columns, each tap sum left to right.  All
array arithmetic below is float32 (numpy keeps float32 op float32 in float32).

keypoint_head_outputs: keypoint_rcnn_heads.roi_pose_head_v1convX + keypoint_outputs
(:17-88, :129-179) on the CPU with torch, in a chosen dtype, from a state_dict with
the reference's names."""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


def cubic_taps(dst: int, src: int):
    """(index [dst, 4] int64, weight [dst, 4] float32) of the four taps of every
    destination index."""
    scale = np.float64(src) / np.float64(dst)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(f)
    t = f - s
    A, one = f32(-0.75), f32(1)
    t1, u = t + one, one - t
    c0 = ((A * t1 - f32(5) * A) * t1 + f32(8) * A) * t1 - f32(4) * A
    c1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + one
    c2 = ((A + f32(2)) * u - (A + f32(3))) * u * u + one
    c3 = one - c0 - c1 - c2
    s = s.astype(np.int64)
    idx = np.clip(np.stack([s - 1, s, s + 1, s + 2], 1), 0, src - 1)
    w = np.stack([c0, c1, c2, c3], 1)
    assert w.dtype == f32
    return idx, w


def resize_cubic(m: np.ndarray, Hm: int, Wm: int) -> np.ndarray:
    """m [M, M] float32 -> [Hm, Wm] float32."""
    assert m.dtype == f32
    M = m.shape[0]
    ix, cx = cubic_taps(Wm, M)
    hz = m[:, ix[:, 0]] * cx[:, 0] + m[:, ix[:, 1]] * cx[:, 1] + m[:, ix[:, 2]] * cx[:, 2] \
        + m[:, ix[:, 3]] * cx[:, 3]  # [M, Wm]
    iy, cy = cubic_taps(Hm, M)
    out = hz[iy[:, 0]] * cy[:, 0, None] + hz[iy[:, 1]] * cy[:, 1, None] \
        + hz[iy[:, 2]] * cy[:, 2, None] + hz[iy[:, 3]] * cy[:, 3, None]
    assert out.dtype == f32 and out.shape == (Hm, Wm)
    return out


def map_size(box, min_size: int = 0):
    """(w, h float32, Wm, Hm int) of one box."""
    x1, y1, x2, y2 = (f32(v) for v in box[:4])
    w, h = np.maximum(x2 - x1, f32(1)), np.maximum(y2 - y1, f32(1))
    Wm, Hm = int(np.ceil(w)), int(np.ceil(h))
    if min_size > 0:
        Wm, Hm = max(Wm, int(min_size)), max(Hm, int(min_size))
    return w, h, Wm, Hm


def heatmaps_to_keypoints(maps: np.ndarray, boxes: np.ndarray, min_size: int = 0) -> np.ndarray:
    """maps [R, K, M, M], boxes [R, >= 4] -> xy_preds [R, 4, K] float32."""
    maps = np.ascontiguousarray(maps, f32)
    boxes = np.asarray(boxes, f32)
    R, K = maps.shape[:2]
    out = np.zeros((R, 4, K), f32)
    for i in range(R):
        w, h, Wm, Hm = map_size(boxes[i], min_size)
        wc, hc = w / f32(Wm), h / f32(Hm)
        assert wc.dtype == f32
        for k in range(K):
            rm = resize_cubic(maps[i, k], Hm, Wm)
            pos = int(rm.argmax())
            yi, xi = divmod(pos, Wm)
            e = np.exp(rm - rm.max())
            out[i, 0, k] = (np.float64(xi) + 0.5) * np.float64(wc) + np.float64(boxes[i, 0])
            out[i, 1, k] = (np.float64(yi) + 0.5) * np.float64(hc) + np.float64(boxes[i, 1])
            out[i, 2, k] = rm[yi, xi]
            out[i, 3, k] = e[yi, xi] / np.sum(e)
    return out


def keypoint_head_outputs(sd: dict, x: torch.Tensor, cfg, dtype=torch.float64) -> torch.Tensor:
    """x [R, C, P, P] RoI features -> [R, K, S, S] heatmap logits on the CPU in `dtype`."""
    kc = cfg.KRCNN
    g = lambda k: sd[k].detach().cpu().to(dtype)  # noqa: E731
    y = x.detach().cpu().to(dtype)
    pad = kc.CONV_HEAD_KERNEL // 2
    for i in range(kc.NUM_STACKED_CONVS):
        n = "Keypoint_Head.conv_fcn.%d" % (2 * i)
        y = F.relu(F.conv2d(y, g(n + ".weight"), g(n + ".bias"), 1, pad))
    dpad = kc.DECONV_KERNEL // 2 - 1
    if kc.USE_DECONV:
        y = F.relu(F.conv_transpose2d(y, g("Keypoint_Outs.deconv.weight"),
                                      g("Keypoint_Outs.deconv.bias"), 2, dpad))
    if kc.USE_DECONV_OUTPUT:
        y = F.conv_transpose2d(y, g("Keypoint_Outs.classify.weight"),
                               g("Keypoint_Outs.classify.bias"), 2, dpad)
    else:
        y = F.conv2d(y, g("Keypoint_Outs.classify.weight"), g("Keypoint_Outs.classify.bias"))
    if kc.UP_SCALE > 1:
        y = F.conv_transpose2d(y, g("Keypoint_Outs.upsample.upconv.weight"),
                               g("Keypoint_Outs.upsample.upconv.bias"), kc.UP_SCALE,
                               kc.UP_SCALE // 2)
    return y
