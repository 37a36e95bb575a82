"""numpy restatement of im_detect_keypoints_aug's host side (lib/core/test.py:567-730,
lib/utils/keypoints.py:90-100), written from their description: the view list with its
ds / us tags, flip_heatmaps, the HM_AVG / HM_MAX combination and its size-dependent
form.  tests/test_kps_aug_cpu.py pins it to tests/golden/kps_aug.npz (the executed
reference); the GPU tests compare the kernel and the pipeline with it."""
import numpy as np

f32 = np.float32

# the 17 COCO keypoints: nose, then (left, right) pairs -- eye, ear, shoulder, elbow,
# wrist, hip, knee, ankle
COCO_FLIP_PERM = [0] + [i + 1 if i % 2 else i - 1 for i in range(1, 17)]


def views(test_scale, test_max_size, aug):
    """-> (views, ds_tags, us_tags), views as (scale, max_size, hflip) in heatmaps_ts
    order: identity, flip at the test scale, then each scale and its flip."""
    v, ds, us = [(test_scale, test_max_size, False)], [False], [False]
    if aug["H_FLIP"]:
        v.append((test_scale, test_max_size, True))
        ds.append(False)
        us.append(False)
    for s in aug["SCALES"]:
        flips = [False, True] if aug["SCALE_H_FLIP"] else [False]
        for hf in flips:
            v.append((s, aug["MAX_SIZE"], hf))
            ds.append(bool(s < test_scale))
            us.append(bool(s > test_scale))
    return v, ds, us


def flip_heatmaps(h, perm=None):
    """[R, K, M, M]: channel k taken from channel perm[k], the last axis reversed."""
    perm = COCO_FLIP_PERM if perm is None else list(perm)
    return np.ascontiguousarray(h[:, perm][:, :, :, ::-1])


def boxes_area(boxes):
    """float32, each of the three operations per side / product rounded."""
    b = np.asarray(boxes, f32)
    w = (b[:, 2] - b[:, 0]) + f32(1)
    h = (b[:, 3] - b[:, 1]) + f32(1)
    return w * h


def _fold(maps, heur):
    """maps: a list of float32 arrays of one shape, in view order."""
    acc = maps[0].astype(f32, copy=True)
    for m in maps[1:]:
        acc = acc + m if heur == "HM_AVG" else np.maximum(acc, m)
    if heur == "HM_AVG":
        acc = acc / f32(len(maps))
    assert acc.dtype == f32
    return acc


def combine(view_maps, hflips, heur, ds=None, us=None, boxes=None, area_th=None, perm=None):
    """view_maps: T arrays [R, K, M, M] as the network returned them.  Without area_th
    every row combines all T views; with it a row of area < area_th leaves out the ds
    views and any other row the us views.  -> (combined [R, K, M, M], T_row [R])."""
    assert heur in ("HM_AVG", "HM_MAX")
    ts = [flip_heatmaps(m, perm) if hf else np.asarray(m, f32)
          for m, hf in zip(view_maps, hflips)]
    R = ts[0].shape[0]
    if area_th is None:
        return _fold(ts, heur), np.full(R, len(ts), np.int64)
    area = boxes_area(boxes)
    out = np.empty_like(ts[0])
    t_row = np.zeros(R, np.int64)
    for i in range(R):
        small = area[i] < f32(area_th)
        kept = [t[i] for t, d, u in zip(ts, ds, us) if not (d if small else u)]
        out[i] = _fold(kept, heur)
        t_row[i] = len(kept)
    return out, t_row
