"""The problem instances of the guarded-buffer tests (tests/guarded.py), in numpy
and host arithmetic only: tests/test_guarded_cpu.py shows from the oracle that
every case reaches the branch it is there for, the GPU tests run them."""
import functools
import os
import re

import numpy as np

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vosdetectron_amd", "csrc")


def _constant(path, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, (path, pattern)
    value = 1
    for factor in m.group(1).split("*"):  # "8192", "160 * 1024"
        value *= int(factor)
    return value


@functools.lru_cache(maxsize=None)
def nms_constants():
    """(kNmsMaxN, VD_LDS_BYTES) as the sources define them."""
    return (_constant("nms.hip", r"kNmsMaxN\s*=\s*(\d+)"),
            _constant("common.hpp", r"#define\s+VD_LDS_BYTES\s+\(([^)]+)\)"))


def nms_in_lds(n):
    """launch_nms' choice: mask_bytes + 2 * kNmsMaxN + 256 <= VD_LDS_BYTES."""
    max_n, lds = nms_constants()
    return 8 * n * ((n + 63) // 64) + 2 * max_n + 256 <= lds


def nms_lds_boundary():
    """The largest n whose mask still takes the in-LDS resolve."""
    max_n, _ = nms_constants()
    n = max(k for k in range(1, max_n + 1) if nms_in_lds(k))
    assert nms_in_lds(n) and not nms_in_lds(n + 1)
    return n


def nms_sizes():
    b = nms_lds_boundary()
    return [1, 63, 64, 65, b, b + 1, nms_constants()[0]]


def nms_dets(n, seed=0):
    """n boxes on a coarse integer grid (16-pixel corners in a square that grows with
    sqrt(n), sides of 16..64), so that many pairs overlap in every 64-block of the
    processing order; scores on a 1/16 grid: ties everywhere."""
    rng = np.random.default_rng(1000 + n + seed)
    cells = max(2, int(np.sqrt(n) / 2))
    xy = rng.integers(0, cells, (n, 2)) * 16
    wh = rng.integers(1, 5, (n, 2)) * 16
    s = rng.integers(1, 17, n) / 16.0
    return np.hstack([xy, xy + wh - 1, s[:, None]]).astype(np.float32)


# --------------------------------------------------------------------------- proposals
RPN_LEVELS = ((3, 40, 56), (3, 20, 28), (3, 4, 5))   # small; the last is take-all at pre 1000
RPN_IM_INFO = np.array([[640, 896, 1.0], [600, 800, 1.0]], np.float32)  # two different rows

# name -> (levels, pre, post, nms_thresh, min_size, env, scores)
RPN_CASES = {
    "small-split": (RPN_LEVELS, 1000, 300, 0.7, 0, {}, "random"),
    "small-unsplit": (RPN_LEVELS, 1000, 300, 0.7, 0, {"VOSDET_RPN_SPLIT": "0"}, "random"),
    "small-presel0": (RPN_LEVELS, 1000, 300, 0.7, 0, {"VOSDET_RPN_PRESEL": "0"}, "random"),
    "small-mask-lds": (RPN_LEVELS, 1000, 300, 0.7, 0, {"VOSDET_RPN_MASK_LDS": "1"}, "random"),
    "small-no-nms": (RPN_LEVELS, 1000, 300, 0.0, 0, {}, "random"),
    "small-pre40": (RPN_LEVELS, 40, 300, 0.7, 0, {}, "random"),
    "large-by-pre": (((15, 24, 30),), 2049, 300, 0.7, 0, {}, "random"),
    # take-all above kPreMax: every candidate's box arrays live in the slot
    "large-take-all": (((15, 23, 23),), 0, 300, 0.7, 0, {}, "random"),
    "all-tied": (RPN_LEVELS, 1000, 300, 0.7, 0, {}, "tied"),
    "all-filtered": (RPN_LEVELS, 1000, 300, 0.7, 2000, {}, "random"),
    # not a case of its own: the larger instance that runs first in the same carves
    "leftover-source": (((15, 20, 27),), 0, 300, 0.7, 0, {}, "random"),
}
# pre_nms_topN = 0 on 8640 anchors: take-all makes pre = 8640, past the large variant's
# kPreMaxL = 8192 rows, so the library refuses the level (VD_ERR_SHAPE, size function 256)
# -- no take-all level can be "large by n_all > kSelCap" (8192) and still be planned
RPN_REFUSED = (((15, 24, 24),), 0, 300, 0.7, 0)
RPN_ENV = ("VOSDET_RPN_SPLIT", "VOSDET_RPN_PRESEL", "VOSDET_RPN_MASK_LDS")
RPN_LEFTOVER = "leftover-source"


def rpn_anchors(levels):
    """Anchors and spatial scales of a case's levels: FPN levels 4, 5, 6 (strides 16,
    32, 64 -- a 640 x 896 blob) for the 3-anchor cases, the C4 set for 15 anchors."""
    if levels[0][0] == 15:
        return [orc.generate_anchors(16, (32, 64, 128, 256, 512), (0.5, 1, 2))], [1. / 16]
    return [orc.fpn_level_anchors(l) for l in (4, 5, 6)][:len(levels)], \
        [1. / 16, 1. / 32, 1. / 64][:len(levels)]


@functools.lru_cache(maxsize=None)
def rpn_inputs(name):
    """(probs, deltas, anchors, scales, im_info) of a proposals case, two images."""
    levels, _, _, _, _, _, scores = RPN_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    anchors, scales = rpn_anchors(levels)
    probs, deltas = [], []
    for A, H, W in levels:
        p = rng.uniform(0, 1, (2, A, H, W)).astype(np.float32)
        if scores == "tied":
            p[:] = np.float32(0.5)
        else:
            p = (np.round(p * 512) / 512).astype(np.float32)  # ties among distinct values
        probs.append(p)
        deltas.append(rng.normal(0, 0.5, (2, 4 * A, H, W)).astype(np.float32))
    info = RPN_IM_INFO.copy()
    if levels[0][0] == 15:
        info[:, :2] = [[levels[0][1] * 16, levels[0][2] * 16], [levels[0][1] * 16 - 40,
                                                                 levels[0][2] * 16 - 24]]
    return probs, deltas, anchors, scales, info


@functools.lru_cache(maxsize=None)
def rpn_reference(name):
    """[(rois, probs)] per level and image by orc.generate_proposals."""
    levels, pre, post, nms, min_size, _, _ = RPN_CASES[name]
    probs, deltas, anchors, scales, info = rpn_inputs(name)
    out = []
    for l in range(len(levels)):
        r, p = orc.generate_proposals(anchors[l], scales[l], probs[l], deltas[l], info, pre, post,
                                      nms, min_size)
        if nms <= 0:  # the op's output capacity is post_nms_topN with or without the NMS
            keep = np.concatenate([np.where(r[:, 0] == i)[0][:post] for i in range(2)])
            r, p = r[keep.astype(np.int64)], p[keep.astype(np.int64)]
        out.append([(r[r[:, 0] == i], p[r[:, 0] == i, 0]) for i in range(2)])
    return out


def rpn_unbracketable():
    """tests/test_edge_cases_gpu.py's score map on which the one-workgroup select
    (VOSDET_RPN_PRESEL=0) cannot bracket pre_nms_topN: image 1 of two; image 0 is an
    ordinary random map, so the failing slot has a neighbour on each side."""
    H, W, A = 200, 336, 3
    n_all, S = H * W * A, 2048
    flat = np.full(n_all, 0.5, np.float32)
    samp = (np.arange(S, dtype=np.int64) * n_all) // S
    flat[samp] = 0.0
    flat[samp[:4]] = 1.0
    bad = flat.reshape(H * W, A).T.reshape(A, H, W)
    rng = np.random.default_rng(5)
    p = rng.uniform(0, 1, (2, A, H, W)).astype(np.float32)
    p[1] = bad
    d = np.zeros((2, 4 * A, H, W), np.float32)
    d[0] = rng.normal(0, 0.5, (4 * A, H, W))
    info = np.array([[800, 1344, 1.0], [800, 1344, 1.0]], np.float32)
    return p, d, orc.fpn_level_anchors(2), 1. / 4, info


# --------------------------------------------------------------------------- detections
# name -> (N, R, K, roi_count, dets_per_im, det_cap, score_thresh)
DET_CASES = {
    "r65": (2, 65, 3, (65, 0), 100, 256, 0.05),
    "r1000": (2, 1000, 5, (1000, 963), 20, 20, 0.05),      # dets_per_im == det_cap < survivors
    "r2048": (1, 2048, 2, (2048,), 100, 128, 0.05),        # kDetRMax
    "r65-nothing": (2, 65, 3, (65, 40), 100, 256, 2.0),    # nothing above the score threshold
}
DET_IM = (480, 854)


@functools.lru_cache(maxsize=None)
def det_inputs(name):
    N, R, K, counts = DET_CASES[name][:4]
    rng = np.random.default_rng(R + K)
    rois = np.zeros((N, R, 5), np.float32)
    for i in range(N):
        xy = rng.uniform(0, 800, (R, 2))
        wh = rng.uniform(8, 200, (R, 2))
        rois[i, :, 0] = i
        rois[i, :, 1:3] = xy
        rois[i, :, 3:5] = np.minimum(xy + wh, [DET_IM[1] + 9, DET_IM[0] - 1])
    logits = rng.normal(0, 1.5, (N, R, K)).astype(np.float32)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    cls = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    pred = rng.normal(0, 1.0, (N, R, 4 * K)).astype(np.float32)
    return rois, cls, pred, np.array(counts, np.int32)


def det_reference(name, i, **kw):
    """(scores, boxes, classes, survivors before the limit) of image i."""
    N, R, K, counts, per_im, _, thr = DET_CASES[name]
    rois, cls, pred, _ = det_inputs(name)
    r = counts[i]
    if r == 0:
        z = np.zeros
        return z(0, np.float32), z((0, 4), np.float32), z(0, np.int32), 0
    pb = orc.clip_tiled_boxes(orc.bbox_transform(rois[i, :r, 1:5], pred[i, :r], (10., 10., 5., 5.)),
                              (DET_IM[0], DET_IM[1], 3))
    s, b, cb = orc.box_results_with_nms_and_limit(cls[i, :r], pb, K, score_thresh=thr,
                                                  dets_per_im=per_im, **kw)
    c = np.concatenate([[j] * len(cb[j]) for j in range(1, K)] + [np.zeros(0)]).astype(np.int32)
    _, _, cb_all = orc.box_results_with_nms_and_limit(cls[i, :r], pb, K, score_thresh=thr,
                                                      dets_per_im=0, **kw)
    return s, b, c, sum(len(cb_all[j]) for j in range(1, K))


# --------------------------------------------------------------------------- RLE
RLE_R = 28
RLE_FRAMES = ((37, 53), (24, 9000))


@functools.lru_cache(maxsize=None)
def rle_planes(H, W):
    """Planes for vd_mask_rle in the order that places the rows as the case needs:
    row 0 fits, a middle row (the checkerboard, H * W runs) and the last row
    overflow, one row needs exactly cap; an all-zero and an all-one plane."""
    rng = np.random.default_rng(H + W)
    # alternating in column-major order (the checkerboard for odd H): H * W runs
    cb = ((np.arange(W)[None] * H + np.arange(H)[:, None]) % 2).astype(np.uint8)
    blob = np.zeros((H, W), np.uint8)
    blob[2:9, 3:11] = 1
    blob[4, 5] = 0
    exact = np.zeros((H, W), np.uint8)
    exact[1:6:2, 2:8] = 1                    # 6 columns x 3 separate pixels
    noise = (rng.uniform(0, 1, (H, W)) < 0.5).astype(np.uint8)
    planes = np.stack([blob, np.zeros((H, W), np.uint8), cb, np.ones((H, W), np.uint8), exact,
                       noise])
    need = np.array([len(orc.rle_encode(p)[1]) for p in planes])
    return planes, need, int(need[4])        # cap: what the "exact" row needs


@functools.lru_cache(maxsize=None)
def rle_masks(H, W):
    """Masks and boxes for the fused vd_segm_rle / vd_paste_masks in the same row
    roles: boxes touch all four frame edges, one is a degenerate 1-pixel box."""
    rng = np.random.default_rng(7 * H + W)
    R = RLE_R
    cb = ((np.arange(R)[:, None] + np.arange(R)[None]) % 2).astype(np.float32) * 0.9 + 0.05
    full = [0, 0, W - 1, H - 1, 1]
    masks = np.stack([rng.uniform(0.6, 1, (R, R)),          # 0: a solid box: few runs
                      np.zeros((R, R)),                      # 1: all zero
                      cb,                                    # 2: checkerboard, full frame
                      np.full((R, R), 0.9),                  # 3: all one, full frame
                      rng.uniform(0.6, 1, (R, R)),           # 4: the row that needs exactly cap
                      np.full((R, R), 0.9),                  # 5: degenerate 1-pixel box
                      rng.uniform(0, 1, (R, R))]).astype(np.float32)  # 6: noise, full frame
    boxes = np.array([[3.2, 4.1, 17.7, 20.3, 1], full, full, full,
                      [W - 12.4, H - 9.6, W - 1, H - 1, 1], [7, 7, 7, 7, 1], full], np.float32)
    ref = orc.paste_masks(masks, boxes, H, W)
    need = np.array([len(orc.rle_encode(p)[1]) for p in ref])
    return masks, boxes, ref, need, int(need[4])


RLE_RAGGED_HW = ((37, 53), (40, 60))   # even rows in the first frame, odd in the second


@functools.lru_cache(maxsize=None)
def rle_ragged():
    """The (37, 53) masks and boxes, each detection pasted into its own frame."""
    masks, boxes = rle_masks(37, 53)[:2]
    hw = np.array([RLE_RAGGED_HW[i % 2] for i in range(len(masks))], np.int32)
    ref = [orc.paste_masks(masks[i:i + 1], boxes[i:i + 1], int(hw[i, 0]), int(hw[i, 1]))[0]
           for i in range(len(masks))]
    need = np.array([len(orc.rle_encode(p)[1]) for p in ref])
    return masks, boxes, hw, ref, need, int(need[4])


RLE_STRING_ROWS = ([5, 1, 2 ** 31 - 1, 3, 0], [], [1066400], [2 ** 31 - 1], [], [0, 1066400],
                   [3, 10, 2, 1, 900, 4, 3])


# --------------------------------------------------------------------------- mask-IoU NMS
MASK_NMS_CASES = ((5, 37, 53), (9, 5, 130), (1, 64, 64))


@functools.lru_cache(maxsize=None)
def mask_nms_inputs(n, H, W):
    """Blobs that overlap a little (few are discarded), two classes: with n = 9 class 1
    holds more survivors than max_per_class = 2."""
    rng = np.random.default_rng(n * H + W)
    masks = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        x0 = (i * W) // (n + 1)
        masks[i, :, x0:x0 + max(2, W // (n + 1)) + 1] = 1
        masks[i] &= (rng.uniform(0, 1, (H, W)) < 0.9).astype(np.uint8)
    masks[-1, -1, -1] = 1                                # the last bit of the partial word
    dets = np.hstack([rng.uniform(0, 40, (n, 4)),
                      np.round(rng.uniform(0.2, 1, (n, 1)) * 8) / 8]).astype(np.float32)
    cls = np.sort(np.where(np.arange(n) < max(1, (2 * n) // 3), 1, 2)).astype(np.int32)
    return masks, dets, cls


# --------------------------------------------------------------------------- union
UNION = dict(F=2, R=48, K=3, T=2, cand_cap=40, big_cap=128, im=(300, 451), scales=(1.0, 1.5),
             hflip=(False, True), ar=(None, 1.25))


def union_view_width(t):
    from tests import aspect_ref
    W, ar = UNION["im"][1], UNION["ar"][t]
    return W if ar is None else aspect_ref.aspect_width(W, ar)


@functools.lru_cache(maxsize=None)
def union_inputs():
    """Two views (the second flipped and aspect-stretched: vd_box_union_add_view_ar) of
    two images, K = 3: class 1 of image 0 holds 30 candidates in view 0 and 30 more in
    view 1 (past cand_cap = 40 in the second view, inside big_cap); class 2 has
    candidates in no view; image 1 stays small."""
    u = UNION
    rng = np.random.default_rng(23)
    T, F, R, K = u["T"], u["F"], u["R"], u["K"]
    rois = np.zeros((T, F, R, 5), np.float32)
    cls = np.zeros((T, F, R, K), np.float32)
    pred = rng.normal(0, 0.3, (T, F, R, 4 * K)).astype(np.float32)
    counts = np.array([[R, R - 7], [R - 3, R]], np.int32)
    for t in range(T):
        Wv = union_view_width(t)
        for i in range(F):
            xy = rng.uniform(0, [Wv - 130, 170], (R, 2))
            wh = rng.uniform(20, 120, (R, 2))
            rois[t, i, :, 0] = i
            rois[t, i, :, 1:3] = xy * u["scales"][t]
            rois[t, i, :, 3:5] = np.minimum(xy + wh, [Wv - 1, u["im"][0] - 1]) * u["scales"][t]
            hot = 30 if i == 0 else 6
            cls[t, i, :hot, 1] = rng.uniform(0.1, 0.9, hot)
            cls[t, i, hot:, 1] = rng.uniform(0, 0.04, R - hot)
            cls[t, i, :, 2] = rng.uniform(0, 0.04, R)
            cls[t, i, :, 0] = 1 - cls[t, i, :, 1:].sum(-1)
    return rois, cls.astype(np.float32), pred, counts


@functools.lru_cache(maxsize=None)
def union_reference(i):
    """(scores, boxes, classes, candidates per class 1..K-1) of image i by the oracle
    tests/test_tta_gpu.py and tests/test_aspect_views_gpu.py use."""
    from tests import aspect_ref, aug_ref
    u = UNION
    rois, cls, pred, counts = union_inputs()
    H, W = u["im"]
    scores_ts, boxes_ts = [], []
    for t in range(u["T"]):
        n = counts[t, i]
        scores_ts.append(cls[t, i, :n])
        boxes_ts.append(aspect_ref.decode_view(rois[t, i, :n], pred[t, i, :n],
                                               np.float32(u["scales"][t]), H, W, u["ar"][t],
                                               u["hflip"][t]))
    sc, bx = aug_ref.union(scores_ts, boxes_ts)
    s, b, cb = orc.box_results_with_nms_and_limit(sc, bx, u["K"])
    c = np.concatenate([[j] * len(cb[j]) for j in range(1, u["K"])] +
                       [np.zeros(0)]).astype(np.int32)
    return s, b, c, (sc[:, 1:] >= 0.05).sum(0)
