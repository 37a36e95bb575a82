"""im_detect_bbox on caller-given boxes (MODEL.FASTER_RCNN False), restated in numpy
for F frames: lib/core/test.py:128-190 with _get_rois_blob (:877-906).

Per frame: rois = float32(hstack(frame, float64(boxes) * im_scale)); hashes =
np.round(rois * DEDUP_BOXES) (float32, half to even) . (1, 1e3, 1e6, 1e9, 1e12) in
float64; np.unique with return_index / return_inverse (the distinct hashes ascending,
each by its first row); the head runs on rois[index]; bbox_transform on boxes[index];
scores and pred_boxes are read back through inv_index.

The fixture (tests/golden/given_boxes.npz, tools/gen_goldens.py given_boxes) is the
reference's own im_detect_bbox run with the stand-in model `standin_head` below, whose
cls_score and bbox_pred are fixed float32 functions of the RoI rows it is handed: the
outputs pin which rows the head saw and in what order.  The same functions make the
boxes of every fixture case (`case_boxes`), so the generator and the tests share them.

`half_away` and `last` plant the two defects the fixture must catch.
"""
import numpy as np

from oracle import oracle as orc

V = np.array([1, 1e3, 1e6, 1e9, 1e12])
K = 5  # classes of the stand-in head
REG_WEIGHTS = (10., 10., 5., 5.)


def rois_blob(boxes, im_scale, frame=0):
    """_get_rois_blob: float64 product, float32 blob; column 0 is the frame."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    rois = b.astype(np.float64) * np.float64(im_scale)
    lv = np.full((b.shape[0], 1), frame, np.float64)
    return np.hstack((lv, rois)).astype(np.float32)


def _round_half_away(x):
    return (np.sign(x) * np.floor(np.abs(x) + np.float32(0.5))).astype(x.dtype)


def hashes(rois, dedup, half_away=False):
    q = rois * np.float32(dedup)
    assert q.dtype == np.float32
    q = _round_half_away(q) if half_away else np.round(q)
    return q.astype(np.float64).dot(V)


def dedup(rois, dedup_boxes, half_away=False, last=False):
    """-> (rois[index], index, inv_index) of test.py:132-139; dedup_boxes == 0: identity."""
    n = rois.shape[0]
    if not dedup_boxes > 0:
        idx = np.arange(n, dtype=np.int64)
        return rois.copy(), idx, idx.copy()
    h = hashes(rois, dedup_boxes, half_away)
    _, index, inv = np.unique(h, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    if last:
        index = np.array([np.flatnonzero(inv == u).max() for u in range(index.size)], np.int64)
    return rois[index], index.astype(np.int64), inv.astype(np.int64)


def rois_from_boxes(boxes, counts, im_scale, dedup_boxes, **defect):
    """vd_rois_from_boxes' outputs for boxes [F,cap,4], counts [F], im_scale [F]: rois
    [F,cap,5], ucounts [F], index [F,cap], inv_index [F,cap]; rows past the counts zero
    (the kernel leaves them untouched).  A count above cap: ucounts -1, nothing else."""
    F, cap = boxes.shape[:2]
    rois = np.zeros((F, cap, 5), np.float32)
    ucounts = np.zeros((F,), np.int32)
    index = np.zeros((F, cap), np.int32)
    inv_index = np.zeros((F, cap), np.int32)
    for f in range(F):
        n = int(counts[f])
        if n > cap:
            ucounts[f] = -1
            continue
        if n <= 0:
            ucounts[f] = n
            continue
        r, i, v = dedup(rois_blob(boxes[f, :n], im_scale[f], f), dedup_boxes, **defect)
        ucounts[f] = len(i)
        rois[f, :len(i)], index[f, :len(i)], inv_index[f, :n] = r, i, v
    return rois, ucounts, index, inv_index


def standin_head(rois, num_classes=K):
    """The stand-in model's cls_score [R, K] and bbox_pred [R, 4K], float32 functions of
    the RoI rows.  cls_score is the row itself times 2^-11 (K = 5 columns, exact and
    one-to-one, so a score row names the RoI row it came from even where two RoIs differ
    in their last bit); bbox_pred mixes the columns into deltas within +-0.4."""
    r = np.asarray(rois, np.float32)
    assert num_classes == r.shape[1] == 5
    scores = (r * np.float32(2. ** -11)).astype(np.float32)
    base = (r[:, 0] * np.float32(7.) + r[:, 1] * np.float32(0.37) + r[:, 2] * np.float32(0.11)
            + r[:, 3] * np.float32(0.23) + r[:, 4] * np.float32(0.05)).astype(np.float32)
    dd = np.arange(4 * num_classes, dtype=np.float32)
    deltas = ((np.mod(base[:, None] * np.float32(0.007) + dd[None] * np.float32(0.17),
                      np.float32(1.)) - np.float32(0.5)) * np.float32(0.8)).astype(np.float32)
    return scores, deltas


def detect_bbox(boxes, im_scale, dedup_boxes, im_shape, fpn, frame=0, k_min=2, k_max=5,
                **defect):
    """im_detect_bbox for one frame with the stand-in head -> dict: rois (the rows the head
    saw), index, inv_index, scores, pred_boxes (the caller's rows), and with fpn the
    per-level RoIs and the restore index of _add_multilevel_rois_for_test."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    rois, index, inv = dedup(rois_blob(boxes, im_scale, frame), dedup_boxes, **defect)
    out = {"rois": rois, "index": index, "inv_index": inv}
    if fpn:
        d = orc.distribute(rois, k_min, k_max)
        for lvl in range(k_min, k_max + 1):
            out["rois_fpn%d" % lvl] = d["rois_fpn%d" % lvl]
        out["rois_idx_restore_int32"] = d["rois_idx_restore_int32"]
    scores, deltas = standin_head(rois)
    pred = orc.bbox_transform(boxes[index], deltas, REG_WEIGHTS)
    pred = orc.clip_tiled_boxes(pred, im_shape)
    out["scores"], out["pred_boxes"] = scores[inv], pred[inv]
    return out


# --------------------------------------------------------------------------- #
# the fixture's cases                                                          #
# --------------------------------------------------------------------------- #
IM_SHAPE = (480, 854, 3)  # im_scale 1 at TEST.SCALE 480, MAX_SIZE 854
IM_SHAPE_SCALED = (375, 500, 3)  # TEST.SCALE 600 / MAX_SIZE 1000: im_scale 1.6


def _random_boxes(rng, n, hw, dup_frac=0.):
    H, W = hw
    xy = rng.uniform(0, [W - 40, H - 40], (n, 2))
    wh = rng.uniform(4, [W / 2, H / 2], (n, 2))
    b = np.hstack([xy, np.minimum(xy + wh, [W - 1, H - 1])]).astype(np.float32)
    ndup = int(n * dup_frac)
    if ndup:
        dst = rng.choice(n, ndup, replace=False)
        b[dst] = b[rng.integers(0, n, ndup)]
    return b


def case_boxes():
    """name -> (boxes [N,4] float32, im_shape, (TEST.SCALE, TEST.MAX_SIZE), DEDUP_BOXES)."""
    rng = np.random.default_rng(20261021)
    hw, ident = IM_SHAPE[:2], (480, 854)
    c = {}
    c["n1"] = (_random_boxes(rng, 1, hw), IM_SHAPE, ident, 0.0625)
    c["n5_equal"] = (np.repeat(_random_boxes(rng, 1, hw), 5, axis=0), IM_SHAPE, ident, 0.0625)
    c["n64"] = (_random_boxes(rng, 64, hw, 0.25), IM_SHAPE, ident, 0.0625)
    c["n65"] = (_random_boxes(rng, 65, hw, 0.25), IM_SHAPE, ident, 0.0625)
    c["n300"] = (_random_boxes(rng, 300, hw, 1. / 3), IM_SHAPE, ident, 0.0625)
    # rows 0, 3 (a copy) and 4 (differs below the quantum of 16 pixels at 1/16) share a
    # hash and are merged onto row 0; rows 1 and 2 differ by one quantum in x2: kept apart
    c["below_quantum"] = (np.array([[100.5, 50.25, 300., 200.], [17., 33., 121., 90.],
                                    [17., 33., 137., 90.], [100.5, 50.25, 300., 200.],
                                    [101.75, 49., 303.5, 199.]], np.float32),
                          IM_SHAPE, ident, 0.0625)
    # products with 1/16 exactly on .5, both parities: 8 -> 0.5 -> 0, 24 -> 1.5 -> 2,
    # 40 -> 2.5 -> 2, 56 -> 3.5 -> 4.  Half away from zero gives 1, 2, 3, 4 instead, which
    # splits (8, 0) and merges (8, 16), (40, 48): both index and inv_index change
    c["half_even"] = (np.array([[8., 8., 200., 200.], [0., 0., 200., 200.],
                                [16., 16., 200., 200.], [24., 24., 200., 200.],
                                [32., 32., 200., 200.], [40., 40., 200., 200.],
                                [48., 48., 200., 200.], [56., 56., 200., 200.],
                                [64., 64., 200., 200.], [8., 24., 40., 56.],
                                [0., 32., 32., 64.]], np.float32), IM_SHAPE, ident, 0.0625)
    c["dedup0"] = (_random_boxes(rng, 40, hw, 0.25), IM_SHAPE, ident, 0.)
    c["dedup_tenth"] = (np.vstack([_random_boxes(rng, 60, hw, 0.2),
                                   # 0.1f * 25 rounds in float32; 5, 15, 25 sit near .5
                                   [[5., 15., 25., 35.], [15., 25., 35., 45.],
                                    [4.99999, 15.00001, 25., 35.]]]).astype(np.float32),
                        IM_SHAPE, ident, 0.1)
    c["scaled"] = (_random_boxes(rng, 80, IM_SHAPE_SCALED[:2], 0.25), IM_SHAPE_SCALED,
                   (600, 1000), 0.0625)
    return c


CASES = ("n1", "n5_equal", "n64", "n65", "n300", "below_quantum", "half_even", "dedup0",
         "dedup_tenth", "scaled")
RECORDED = ("rois", "index", "inv_index", "scores", "pred_boxes")
RECORDED_FPN = RECORDED + ("rois_fpn2", "rois_fpn3", "rois_fpn4", "rois_fpn5",
                           "rois_idx_restore_int32")
