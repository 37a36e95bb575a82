"""viz_mask_result (lib/utils/vis.py:119-157) restated in numpy, and the inputs of the
label-map tests.

paint(): the reference's loop on oracle.paste_masks planes -- ascending score order,
`score < thresh` skipped, outImg[mask > 0] = id, rtv_gt likewise for score >
rvt_cls_threshold -- with the two rules DESIGN.md writes down: thresholds are compared in
float32 (NumPy >= 2 evaluates `np.float32 < python float` that way), and equal scores are
painted in ascending row order (a stable sort), so the higher row wins.
first_hit(): the form the kernel computes -- per pixel the covering painted detection of
highest (score, row) -- which must equal paint() on both maps.

inputs(): one 37 x 83 frame (odd width; more than one 64 x 32 tile in both directions,
a multiple of none) with 24 detections; the conditions a pass depends on are asserted
here on the reference alone.
"""
import functools

import numpy as np

from oracle import oracle as orc

H, W, R, N = 37, 83, 28, 24
THRESH, GT_THRESH = 0.25, 0.6
TIE = (5, 6, 7)  # rows of equal score 0.5; 5 and 6 on identical boxes, 7 shifted by one pixel

_FIXED = [  # (box, score): rows 0..7
    ((-5, -4, 90, 41), 0.30),            # the whole frame and beyond, constant 0.9 mask
    ((5.2, 6.1, 5.9, 6.3), 0.95),        # sub-pixel
    ((20, 10, 33, 23), 0.70),            # expanded integer box 15 x 15: the exact-2x path
    ((-10, 5, 15, 30), 0.65),            # partly left of the frame
    ((40, -8, 70, 12), 0.55),            # partly above it
    ((30, 12, 62, 34), 0.50),            # the tied pair ...
    ((30, 12, 62, 34), 0.50),
    ((31, 13, 63, 35), 0.50),            # ... and the third, one pixel on
]


def blob(rng, r):
    """A smooth bump in (0.05, 0.95): above 0.5 inside an ellipse around the middle."""
    yy, xx = np.mgrid[0:r, 0:r].astype(np.float64)
    cx, cy = rng.uniform(0.35 * r, 0.65 * r, 2)
    sx, sy = rng.uniform(0.25 * r, 0.5 * r, 2)
    g = np.exp(-(((xx - cx) / sx) ** 2 + ((yy - cy) / sy) ** 2) / 2)
    return (0.05 + 0.9 * g).astype(np.float32)


def make(seed=0, r=R, h=H, w=W, distinct=False):
    """(masks [24,r,r], dets [24,5], classes [24] int32), classes nondecreasing (the
    reference takes detections grouped by class).  distinct: the three tied scores pulled
    apart (0.5, 0.51, 0.49), every score a different float32 -- the golden's inputs."""
    rng = np.random.default_rng(20261021 + seed)
    masks = np.stack([blob(rng, r) for _ in range(N)])
    masks[0] = 0.9
    masks[1] = 0.9
    dets = np.zeros((N, 5), np.float32)
    for i, (b, s) in enumerate(_FIXED):
        dets[i] = b + (s,)
    k = N - len(_FIXED)
    c = np.stack([rng.uniform(0, w, k), rng.uniform(0, h, k)], 1)
    wh = rng.uniform(4, 40, (k, 2))
    dets[len(_FIXED):, :4] = np.hstack([c - wh / 2, c + wh / 2])
    # 16 distinct scores, three of them under THRESH, none equal to a fixed one
    dets[len(_FIXED):, 4] = rng.permutation(np.linspace(0.12, 0.98, k) + 0.003)
    if distinct:
        dets[TIE, 4] = (0.5, 0.51, 0.49)
        assert np.unique(dets[:, 4]).size == N
    classes = (1 + np.arange(N) * 3 // 4).astype(np.int32)
    return masks, dets, classes


def ids_of(classes, lut=None):
    c = np.asarray(classes, np.int64)
    if lut is None:
        return np.where((c >= 0) & (c <= 255), c, 0).astype(np.uint8)
    lut = np.asarray(lut, np.uint8)
    ok = (c >= 0) & (c < lut.size)
    return np.where(ok, lut[np.clip(c, 0, lut.size - 1)], 0).astype(np.uint8)


def order_of(scores, thresh, valid=None):
    """Painting order: stable ascending float32 score; score < float32(thresh) and rows
    the filter dropped left out."""
    s = np.asarray(scores, np.float32)
    o = np.argsort(s, kind="stable")
    keep = ~(s[o] < np.float32(thresh))
    if valid is not None:
        keep &= np.asarray(valid)[o] != 0
    return o[keep]


def paint(planes, scores, classes, thresh, gt_thresh, lut=None, valid=None):
    """(label, gt) of one frame from its n x H x W binary planes, the reference's way."""
    n, h, w = planes.shape
    ids = ids_of(classes, lut)
    s = np.asarray(scores, np.float32)
    label, gt = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for i in order_of(s, thresh, valid):
        label[planes[i] > 0] = ids[i]
        if s[i] > np.float32(gt_thresh):
            gt[planes[i] > 0] = ids[i]
    return label, gt


def first_hit(planes, scores, classes, thresh, gt_thresh, lut=None, valid=None):
    """(label, gt) per pixel from the covering painted detection of highest (score, row)."""
    n, h, w = planes.shape
    ids = ids_of(classes, lut)
    s = np.asarray(scores, np.float32)
    label, gt = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    undecided = np.ones((h, w), bool)
    for i in order_of(s, thresh, valid)[::-1]:
        hit = undecided & (planes[i] > 0)
        label[hit] = ids[i]
        if s[i] > np.float32(gt_thresh):
            gt[hit] = ids[i]
        undecided &= ~hit
    return label, gt


def bboxs(dets, classes, thresh, gt_thresh):
    """rtv_bboxs: per class the boxes painted into rtv_gt, in painting order."""
    out = [[] for _ in range(256)]
    for i in order_of(dets[:, 4], thresh):
        if dets[i, 4] > np.float32(gt_thresh):
            out[int(classes[i])].append(dets[i, :4])
    return out


def planes_of(masks, dets, h=H, w=W, bin_thresh=0.5):
    if len(masks) == 0:
        return np.zeros((0, h, w), np.uint8)
    return orc.paste_masks(masks, dets, h, w, bin_thresh)


@functools.lru_cache(maxsize=None)
def inputs(r=R):
    """The tie inputs and their planes; the conditions asserted on the reference alone."""
    masks, dets, classes = make(0, r)
    planes = planes_of(masks, dets)
    label, gt = paint(planes, dets[:, 4], classes, THRESH, GT_THRESH)
    painted = order_of(dets[:, 4], THRESH)
    assert len(painted) < N, "no detection under the threshold"
    cover = (planes[painted] > 0).sum(0)
    stats = dict(nonzero=float((label != 0).mean()), triple=int((cover >= 3).sum()),
                 gt_differs=int((gt != label).sum()),
                 tie_overlap=int(((planes[TIE[0]] > 0) & (planes[TIE[1]] > 0)).sum()))
    assert stats["nonzero"] >= 0.30, stats
    assert stats["triple"] >= 100, stats
    assert stats["gt_differs"] >= 1, stats
    assert stats["tie_overlap"] >= 50, stats
    assert dets[TIE[0], 4] == dets[TIE[1], 4] == dets[TIE[2], 4]
    assert classes[TIE[0]] != classes[TIE[1]] != classes[TIE[2]]
    for a in (masks, dets, classes, planes):
        a.setflags(write=False)
    return masks, dets, classes, planes, stats


COUNTS = (24, 0, 7)


@functools.lru_cache(maxsize=None)
def frames(r=R):
    """F = 3 frames with counts (24, 0, 7): frame 0 the tie inputs, frame 1 empty, frame
    2 the first 7 rows of another draw.  -> masks [31,r,r] in (frame, detection) order,
    dets [3,24,5], classes [3,24], counts [3] and the per-frame planes.  Rows past a
    frame's count hold a confident whole-frame box that must never be painted."""
    m0, d0, c0, p0, _ = inputs(r)
    m2, d2, c2 = make(1, r)
    dets = np.zeros((3, N, 5), np.float32)
    dets[:] = (-5, -4, 90, 41, 0.99)
    classes = np.full((3, N), 77, np.int32)
    dets[0], classes[0] = d0, c0
    dets[2, :7], classes[2, :7] = d2[:7], c2[:7]
    masks = np.concatenate([m0, m2[:7]])
    planes = [p0, planes_of(m2[:0], d2[:0]), planes_of(m2[:7], d2[:7])]
    for a in [masks, dets, classes] + planes:
        a.setflags(write=False)
    return masks, dets, classes, np.asarray(COUNTS, np.int32), planes


def reference(planes, dets, classes, counts, thresh=THRESH, gt_thresh=GT_THRESH, lut=None,
              valid=None):
    """(label, gt) [F,H,W] of frames()-shaped inputs by paint()."""
    out = []
    for f, k in enumerate(counts):
        v = None if valid is None else valid[f, :k]
        out.append(paint(planes[f][:k], dets[f, :k, 4], classes[f, :k], thresh, gt_thresh, lut, v))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def rle_decode(rle):
    """pycocotools mask.decode of one {'size', 'counts' (str)}: rleFrString, then the
    runs laid out in column-major order, zeros first."""
    h, w = rle["size"]
    s = rle["counts"]
    s = s.decode("ascii") if isinstance(s, bytes) else s
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    flat = np.repeat(np.arange(len(cnts)) & 1, cnts).astype(np.uint8)
    assert flat.size == h * w, (flat.size, h, w)
    return flat.reshape((w, h)).T
