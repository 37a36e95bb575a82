"""The objects of a label map, restated in numpy, and the inputs of the label-object tests.

Reference: DAVIS_imdb.get_gt / get_bboxes (imdb/vos/davis_db.py:180-204), the box form of
lib_vos/tools/get_cls_mapper.py:129-136, and DAVIS_imdb.add_gt_annotations_to_entry
(davis_db.py:407-517) with _expand_box (:399-405), box_utils.xywh_to_xyxy and
clip_xyxy_to_image (lib/utils/boxes.py:80-88, :129-135).

remap(): get_gt's rule -- if 255 occurs its pixels take len(np.unique(map)) - 1, the count
of every distinct value of the raw map (0 and 255 included).
bounding_rect(): cv2.boundingRect of a binary mask: (xmin, ymin, xmax - xmin + 1,
ymax - ymin + 1), (0, 0, 0, 0) for an empty one.
rle_counts(): pycocotools mask.encode's run lengths: column-major, the first run counts
zeros (and is 0 when the first pixel is set).
objects(): one frame -> ids, rects, areas, boxes (float32), rle rows, in np.unique order.
  rect form (expand None): (x, y, x + w, y + h), every object kept;
  entry form: float64 all the way -- e = sqrt(w * h) * expand, x -= e / 2, y -= e / 2,
  h += e, w += e, x2 = x + max(0, w - 1), the clip to [0, W - 1] / [0, H - 1], the filter
  area > 0 and x2 > x1 and y2 > y1 -- and one rounding to float32 at the end
  (entry['boxes'] is float32).
"""
import functools

import numpy as np

FAILED = -1  # VD_COUNT_SELECT_FAILED
H, W = 37, 83  # the golden frame


def remap(lab):
    lab = np.asarray(lab, np.uint8)
    vals = np.unique(lab)
    out = np.array(lab)
    if vals.size and vals[-1] == 255:
        out[lab == 255] = len(vals) - 1
    return out


def bounding_rect(mask):
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return 0, 0, 0, 0
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1),
            int(ys.max() - ys.min() + 1))


def rle_counts(mask):
    flat = np.asarray(mask, np.uint8).T.reshape(-1) != 0  # column-major
    if flat.size == 0:
        return np.zeros(1, np.uint32)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    pos = np.concatenate([[0], change, [flat.size]])
    runs = np.diff(pos)
    if flat[0]:
        runs = np.concatenate([[0], runs])
    return runs.astype(np.uint32)


def rle_decode_counts(counts, h, w):
    flat = np.repeat(np.arange(len(counts)) & 1, np.asarray(counts, np.int64)).astype(np.uint8)
    assert flat.size == h * w, (flat.size, h, w)
    return flat.reshape((w, h)).T


def expand_box(x, y, w, h, rate):
    e = np.sqrt(np.float64(w * h)) * np.float64(rate)
    x = x - e / 2.
    y = y - e / 2.
    h = h + e
    w = w + e
    return x, y, w, h


def entry_box(rect, expand, im_h, im_w):
    """-> ((x1, y1, x2, y2) float64, kept-by-the-box-test)."""
    x, y, w, h = expand_box(*rect, rate=expand)
    x1, y1 = x, y
    x2 = x1 + np.maximum(0., w - 1.)
    y2 = y1 + np.maximum(0., h - 1.)
    x1 = np.minimum(im_w - 1., np.maximum(0., x1))
    y1 = np.minimum(im_h - 1., np.maximum(0., y1))
    x2 = np.minimum(im_w - 1., np.maximum(0., x2))
    y2 = np.minimum(im_h - 1., np.maximum(0., y2))
    return (x1, y1, x2, y2), bool(x2 > x1 and y2 > y1)


def objects(lab, expand=0.05, remap255=False):
    """One H x W frame -> dict(ids u8 [k], rects i32 [k,4], areas i32 [k], boxes f32 [k,4],
    rle list of uint32 arrays), kept objects in ascending value order."""
    lab = np.asarray(lab, np.uint8)
    im_h, im_w = lab.shape
    gt = remap(lab) if remap255 else lab
    ids, rects, areas, boxes, rle = [], [], [], [], []
    for val in np.unique(gt):
        if val == 0:
            continue
        mask = np.array(gt == val, dtype=np.uint8)
        rect = bounding_rect(mask)
        area = int(mask.sum())
        if expand is None:
            x, y, w, h = rect
            box, keep = (x, y, x + w, y + h), True
        else:
            box, ok = entry_box(rect, expand, im_h, im_w)
            keep = area > 0 and ok
        if not keep:
            continue
        ids.append(val)
        rects.append(rect)
        areas.append(area)
        boxes.append(np.asarray(box, np.float64).astype(np.float32))
        rle.append(rle_counts(mask))
    return dict(ids=np.asarray(ids, np.uint8), rects=np.asarray(rects, np.int32).reshape(-1, 4),
                areas=np.asarray(areas, np.int32),
                boxes=np.asarray(boxes, np.float32).reshape(-1, 4), rle=rle)


def batch(labels, expand=0.05, remap255=False, obj_cap=255):
    """F frames -> (per-frame objects() dicts, counts int32 [F]); a frame with more kept
    objects than obj_cap has count FAILED."""
    objs = [objects(l, expand, remap255) for l in labels]
    counts = np.asarray([len(o["ids"]) if len(o["ids"]) <= obj_cap else FAILED for o in objs],
                        np.int32)
    return objs, counts


# --------------------------------------------------------------------------- input makers
def blobs(h, w, n, seed=0, values=None):
    """n elliptical objects painted in turn on a zero map (later ones cover earlier ones);
    object i takes values[i] (default i + 1)."""
    rng = np.random.default_rng(20261021 + seed)
    lab = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        sx, sy = rng.uniform(0.04 * w + 1, 0.25 * w + 1), rng.uniform(0.04 * h + 1, 0.25 * h + 1)
        inside = ((xx - cx) / sx) ** 2 + ((yy - cy) / sy) ** 2 <= 1.0
        lab[inside] = (i + 1) if values is None else values[i]
    return lab


@functools.lru_cache(maxsize=None)
def golden_frame():
    """The 37 x 83 frame of tests/golden/label_objects.npz: blobs with values 1, 2, 3, 5 and
    255 (so that get_gt's remap acts), a single row, a single pixel in a corner (its
    expanded box is clipped at the border) and a block on the left and bottom borders."""
    lab = blobs(H, W, 5, seed=1, values=(1, 2, 3, 5, 255))
    lab[2, 40:52] = 9        # one row
    lab[0, 82] = 12          # a single pixel in the top right corner
    lab[30:37, 0:6] = 4      # touches the left and bottom borders
    lab.setflags(write=False)
    return lab


def checkerboard(h, w, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((yy + xx) & 1, a, b).astype(np.uint8)
