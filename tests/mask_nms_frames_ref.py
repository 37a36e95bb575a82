"""Inputs and the per-frame reference of vd_mask_iou_nms_frames, shared by
tests/test_mask_nms_frames_cpu.py and tests/test_mask_nms_frames_gpu.py.

The reference is the oracle alone, frame by frame: orc.paste_masks (segm_results'
expand_boxes + cv2.resize + threshold + paste) then orc.nms_with_mask_iou
(lib_vos/tools/vos_test.py:985-1029).  Both are pure numpy.  A box entirely outside
the frame, which the reference's paste cannot take, gets an empty plane (paste())."""
import functools

import numpy as np

from oracle import oracle as orc

R = 28
CAP = 32
# (im_h, im_w, n): an odd size below one word, one above one word, a width that is a
# multiple of 64 (no partial last word)
SIZES = ((37, 45, 24), (70, 100, 32), (64, 128, 32))
# the CPU test also checks the generator on the sizes its statistics were taken at
CPU_SIZES = SIZES + ((64, 96, 32),)
SEEDS = (0, 1, 2, 3)
# (iou_th, max_per_class): cap 1 and 2 remove rows, 100 removes none, 0 keeps nothing
SETTINGS = ((0.5, 1), (0.9, 2), (0.3, 100), (0.5, 0))
COUNT_PREV_BOXES = -2


def gen_frame(rng, n, H, W, r=R):
    """n detections of one frame: (masks [n,r,r], dets [n,5], classes [n] sorted)."""
    nc = max(2, n // 4)
    x0 = rng.uniform(-6, 0.6 * W, nc)
    y0 = rng.uniform(-6, 0.6 * H, nc)
    w = rng.uniform(6, 0.5 * W, nc)
    h = rng.uniform(6, 0.5 * H, nc)
    cl = rng.integers(0, nc, n)
    jit = rng.integers(-3, 4, (n, 4))
    box = np.stack([x0[cl], y0[cl], x0[cl] + w[cl], y0[cl] + h[cl]], 1) + jit
    score = np.round(rng.uniform(0, 1, n) * 16) / 16  # sixteenths: ties
    dets = np.hstack([box, score[:, None]]).astype(np.float32)
    rad = rng.uniform(0.25 * r, 0.5 * r, n)
    cx = rng.uniform(0.4 * r, 0.6 * r, n)
    cy = rng.uniform(0.4 * r, 0.6 * r, n)
    yy, xx = np.mgrid[0:r, 0:r].astype(np.float64)
    dist = np.sqrt((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2)
    masks = (1.0 / (1.0 + np.exp((dist - rad[:, None, None]) / 1.5))).astype(np.float32)
    classes = np.sort(rng.integers(1, 5, n)).astype(np.int32)
    return masks, dets, classes


def gen_step(seed, H, W, counts, cap=CAP, r=R):
    """A step of len(counts) frames: masks [sum(counts),r,r] in (frame, detection)
    order, dets [F,cap,5], classes [F,cap], counts [F] int32.  Rows past a frame's
    count hold a full frame's worth of other detections (never to be read as kept)."""
    rng = np.random.default_rng(seed)
    F = len(counts)
    dets = np.zeros((F, cap, 5), np.float32)
    classes = np.zeros((F, cap), np.int32)
    masks = []
    for f, k in enumerate(counts):
        m, d, c = gen_frame(rng, cap, H, W, r)
        k = max(int(k), 0)
        dets[f], classes[f] = d, c
        masks.append(m[:k])
    return np.concatenate(masks), dets, classes, np.asarray(counts, np.int32)


def step_counts(n):
    return (n, 0, n - 5, 1)


@functools.lru_cache(maxsize=None)
def step(seed, H, W, n):
    """The oracle test's step for one frame size; the arrays are shared: do not write."""
    out = gen_step(seed, H, W, step_counts(n))
    for a in out:
        a.setflags(write=False)
    return out


def frame_rows(counts, cap, M):
    """(first mask row, count) per frame as the kernel forms them: counts clamped to
    [0, cap], summed, and cut to the M rows masks holds (ops.label_maps' rule)."""
    c = np.clip(np.asarray(counts, np.int64), 0, cap)
    end = np.cumsum(c)
    beg = end - c
    return np.minimum(beg, M), np.minimum(end, M) - np.minimum(beg, M)


def paste(masks, boxes, H, W, thresh=0.5):
    """orc.paste_masks, with an all-zero plane for a box whose clipped rectangle is
    empty (entirely outside the frame): the reference's slice assignment raises on
    such a box -- its own boxes are clipped to the frame -- while vd_paste_masks
    writes the empty plane, which the planes-route test holds this to."""
    r = masks.shape[-1]
    eb = orc.expand_boxes(np.asarray(boxes, np.float32)[:, :4], (r + 2.0) / r).astype(np.int32)
    inside = (np.maximum(eb[:, 0], 0) < np.minimum(eb[:, 2] + 1, W)) & \
        (np.maximum(eb[:, 1], 0) < np.minimum(eb[:, 3] + 1, H))
    out = np.zeros((len(masks), H, W), np.uint8)
    if inside.any():
        out[inside] = orc.paste_masks(masks[inside], boxes[inside], H, W, thresh)
    return out


def reference(masks, dets, classes, counts, H, W, iou_th, max_per_class, thresh=0.5,
              planes_out=None):
    """-> (keep lists per frame, keep_counts [F]).  A negative count is returned as it
    is with an empty list.  planes_out: a list that receives each frame's planes."""
    F, cap = dets.shape[:2]
    base, n = frame_rows(counts, cap, len(masks))
    keeps, kc = [], []
    for f in range(F):
        if counts[f] < 0:
            keeps.append([])
            kc.append(int(counts[f]))
            continue
        k, b = int(n[f]), int(base[f])
        planes = paste(masks[b:b + k], dets[f, :k], H, W, thresh)
        if planes_out is not None:
            planes_out.append(planes)
        keep = orc.nms_with_mask_iou(dets[f, :k], classes[f, :k], planes, iou_th, max_per_class)
        keeps.append([int(i) for i in keep])
        kc.append(len(keep))
    return keeps, np.asarray(kc, np.int32)


@functools.lru_cache(maxsize=None)
def step_reference(seed, H, W, n, iou_th, max_per_class):
    m, d, c, k = step(seed, H, W, n)
    return reference(m, d, c, k, H, W, iou_th, max_per_class)


def frame_stats(masks, dets, classes, H, W, iou_th, max_per_class):
    """(detections, kept by the NMS alone, kept after the cap) of one frame."""
    planes = paste(masks, dets, H, W, 0.5)
    nms = orc.nms_with_mask_iou(dets, classes, planes, iou_th, 1 << 20)
    capped = orc.nms_with_mask_iou(dets, classes, planes, iou_th, max_per_class)
    return len(dets), len(nms), len(capped)
