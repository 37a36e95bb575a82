"""numpy restatement of keypoint_results' OKS NMS (lib/utils/keypoints.py:225-266
nms_oks / compute_oks), written from the arithmetic the reference's numpy code
performs under numpy 2 -- the yardstick of vd_nms_oks_frames / vd_compute_oks on
machines without the reference.  tests/golden/nms_oks.npz (the executed
reference) pins it: scores and vars bit for bit, keep exactly, every ovr within
1e-12.

Every step is spelled out instead of left to np.mean / np.sum so that the order
of the additions is the one numpy's pairwise summation uses for 17 terms:
r[j] = a[j] + a[8 + j] (j < 8), ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)),
then + a[16].  Ties in the score are processed higher index first (numpy's stable
sort reversed: its order for n <= 16, and the library's definition for every n).
NaN logits are unsupported."""
import numpy as np

f32, f64 = np.float32, np.float64
K = 17
COCO_SIGMAS = (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87,
               .89, .89)
VARS = (np.array(COCO_SIGMAS, f64) / 10.0 * 2) ** 2
EPS = f64(2.0 ** -52)  # np.spacing(1)


def pairwise17(a):
    """Sum over the last axis (17 terms) in numpy's pairwise order, in a's dtype."""
    assert a.shape[-1] == K
    r = a[..., :8] + a[..., 8:16]
    return (((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3]))
            + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))) + a[..., 16]


def scores(kp):
    """kp [n, 4, 17] float32 -> the mean logit of every row, float32."""
    kp = np.asarray(kp, f32)
    return (pairwise17(kp[:, 2, :]) / f32(K)).astype(f32)


def processing_order(sc):
    """Descending score, the higher index first among equal scores."""
    n = len(sc)
    return np.lexsort((np.arange(n), sc))[::-1]


def compute_oks(src_keypoints, src_roi, dst_keypoints, dst_roi=None):
    """One source row [4, 17] with its box [4] against dst [N, 4, 17] -> [N] float64.
    Only the source's box enters; the prob row is not read."""
    s = np.asarray(src_keypoints, f32)
    b = np.asarray(src_roi, f32)
    d = np.asarray(dst_keypoints, f32).reshape(-1, 4, K)
    area = (b[2] - b[0] + f32(1)) * (b[3] - b[1] + f32(1))
    dx = d[:, 0, :] - s[0, :]
    dy = d[:, 1, :] - s[1, :]
    d2 = dx * dx + dy * dy
    assert d2.dtype == f32 and area.dtype == f32
    e = d2.astype(f64) / VARS / (f64(area) + EPS) / 2
    return pairwise17(np.exp(-e)) / f64(K)


def nms_oks(kp, rois, thresh, record=None):
    """keep: the kept row indices in processing order.  record: a list that receives
    every ovr vector in the order the loop evaluates them."""
    kp = np.asarray(kp, f32).reshape(-1, 4, K)
    rois = np.asarray(rois, f32)
    order = processing_order(scores(kp))
    keep = []
    while order.size:
        i = order[0]
        keep.append(int(i))
        ovr = compute_oks(kp[i], rois[i, :4], kp[order[1:]])
        if record is not None:
            record.append(ovr)
        order = order[1:][ovr <= thresh]
    return keep


def nms_oks_frames(keyps, dets, classes, counts, thresh=0.3):
    """vd_nms_oks_frames on host arrays: keyps [rows, 4, 17] frame-major at the prefix
    sum of the non-negative counts, dets [F, D, 5], classes [F, D], counts [F] ->
    dict(keep [F, D] (-1 past the count), counts [F], dets, classes (zeros past the
    count), keyps [rows, 4, 17] compacted (zeros past the total), scores [F, D])."""
    keyps, dets = np.asarray(keyps, f32), np.asarray(dets, f32)
    classes, counts = np.asarray(classes, np.int32), np.asarray(counts, np.int32)
    F, D = classes.shape
    out = {"keep": np.full((F, D), -1, np.int32), "counts": counts.copy(),
           "dets": np.zeros_like(dets), "classes": np.zeros_like(classes),
           "keyps": np.zeros_like(keyps), "scores": np.zeros((F, D), f32)}
    src = dst = 0
    for f in range(F):
        n = int(counts[f])
        if n < 0:
            continue
        kp = keyps[src:src + n]
        out["scores"][f, :n] = scores(kp)
        keep = nms_oks(kp, dets[f, :n, :4], thresh)
        k = len(keep)
        out["keep"][f, :k] = keep
        out["counts"][f] = k
        out["dets"][f, :k] = dets[f, keep]
        out["classes"][f, :k] = classes[f, keep]
        out["keyps"][dst:dst + k] = kp[keep]
        src += n
        dst += k
    return out


def fixture_cases(path=None):
    """tests/golden/nms_oks.npz (tools/gen_goldens.py nms_oks: the executed reference)
    as (thresh, vars, [case dicts]); ovr is the list of vectors the loop evaluated."""
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "nms_oks.npz")
    z = np.load(path)
    cases = []
    for i in range(int(z["count"])):
        c = {k: z["%s_%d" % (k, i)] for k in ("kp", "rois", "cluster", "keep", "scores")}
        c["kind"] = str(z["kind_%d" % i])
        c["n"] = len(c["kp"])
        c["ovr"] = np.split(z["ovr_%d" % i], np.cumsum(z["ovr_len_%d" % i])[:-1]) \
            if len(z["ovr_len_%d" % i]) else []
        cases.append(c)
    return float(z["thresh"]), z["vars"], cases
