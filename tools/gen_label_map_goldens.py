#!/usr/bin/env python3
"""tests/golden/label_map.npz: the reference's own viz_mask_result
(lib/utils/vis.py:119-157) executed in this container on one frame.

pycocotools is absent, so mask_util.decode -- the one third-party step -- is a stub that
returns the recorded planes (oracle.paste_masks of the inputs, H x W x n as decode returns
them); everything after it (convert_from_cls_format, the argsort, the two thresholds, the
painting, the box lists) is the reference's code.  img_saver records the image it is
handed: that is outImg.  Reuses gen_goldens.install_shims; only data is written.

Contents: a 37 x 83 frame, 24 detections with distinct float32 scores
(tests/label_map_ref.make(distinct=True)), thresh 0.25, rvt_cls_threshold 0.6; the inputs
(masks, boxes, classes) and outImg, rtv_gt, rtv_bboxs (as a [k, 5] array of (class, x1,
y1, x2, y2) in the reference's per-class append order).  Member timestamps are fixed, so
the file regenerates byte for byte.

Usage: python tools/gen_label_map_goldens.py   (writes tests/golden/label_map.npz)
"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_goldens import OUT, install_shims  # noqa: E402


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the file depends on the arrays
    alone, so a second run writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    install_shims()
    import utils.vis as ref_vis
    from tests import label_map_ref as lm

    masks, dets, classes = lm.make(0, distinct=True)
    assert dets.dtype == np.float32 and np.unique(dets[:, 4]).size == lm.N
    assert np.all(np.diff(classes) >= 0)
    planes = lm.planes_of(masks, dets)

    class _MaskUtil:
        @staticmethod
        def decode(segms):
            assert len(segms) == lm.N
            return np.ascontiguousarray(planes.transpose(1, 2, 0))
    ref_vis.mask_util = _MaskUtil

    K = int(classes.max()) + 1
    cls_boxes = [dets[classes == j] for j in range(K)]
    cls_segms = [[{"row": int(i)} for i in np.flatnonzero(classes == j)] for j in range(K)]
    saved = []

    def img_saver(path, img):
        saved.append(np.array(img, copy=True))
        return img

    im = np.zeros((lm.H, lm.W, 3), np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        rtv_gt, rtv_bboxs, clr = ref_vis.viz_mask_result(
            im, "frame", os.path.join(tmp, "out"), cls_boxes, cls_segms, thresh=lm.THRESH,
            img_saver=img_saver, rvt_cls_threshold=lm.GT_THRESH)
    assert len(saved) == 1 and saved[0].dtype == np.uint8 and saved[0].shape == (lm.H, lm.W)
    assert rtv_gt.dtype == np.uint8 and len(rtv_bboxs) == 256
    rows = [np.concatenate([[c], b]) for c, bl in enumerate(rtv_bboxs) for b in bl]
    bb = np.asarray(rows, np.float32).reshape(-1, 5)
    assert (saved[0] != 0).any() and (rtv_gt != saved[0]).any() and len(bb) > 0

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "label_map.npz")
    save_npz(path, masks=masks, dets=dets, classes=classes,
             im_hw=np.array([lm.H, lm.W], np.int64), thresh=np.float64(lm.THRESH),
             rvt_cls_threshold=np.float64(lm.GT_THRESH), outImg=saved[0], rtv_gt=rtv_gt,
             rtv_bboxs=bb)
    size = os.path.getsize(path)
    assert size <= 1 << 20, size
    print("wrote %s (%d bytes): %d boxes in rtv_bboxs, %.0f %% of outImg nonzero"
          % (path, size, len(bb), 100 * (saved[0] != 0).mean()))


if __name__ == "__main__":
    main()
