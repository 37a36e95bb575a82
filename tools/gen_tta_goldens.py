#!/usr/bin/env python3
"""tests/golden/tta.npz: the reference's own im_detect_bbox_aug and im_detect_mask_aug
(lib/core/test.py:193-363, 405-526) executed in this container on recorded per-view
network outputs.

The network calls -- im_detect_bbox, im_conv_body_only, im_detect_mask -- are replaced
by stubs that log their arguments and return recorded arrays; everything between them
(the view order, the flips, np.vstack, the three mask heuristics) is the reference's
code.  box_results_with_nms_and_limit is the fork's (lib_vos/tools/vos_test.py; the
soft_nms fixture explains why), with and without TEST.BBOX_VOTE.  Reuses
gen_goldens.install_shims; only data is written.

Size: T = 6 views (H_FLIP, two scales, SCALE_H_FLIP), R = 200 proposals per view,
K = 5 classes, M = 7 detections with 14 x 14 masks of every class, a 96 x 133 frame (odd
width), tie-free scores.

Usage: python tools/gen_tta_goldens.py   (writes tests/golden/tta.npz)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_goldens import OUT, REF, distinct_scores, install_shims  # noqa: E402

TEST_SCALE, TEST_MAX_SIZE = 96, 133
AUG_SCALES, AUG_MAX_SIZE = (64, 128), 192
R, K, M, RES = 200, 5, 7, 14
IM_H, IM_W = 96, 133
WEIGHTS = (10., 10., 5., 5.)


def main():
    install_shims()
    from core.config import cfg
    import utils.blob as blob_utils
    import utils.boxes as box_utils
    try:
        import core.test as ref_test
        source = "lib/core/test.py"
    except Exception:  # core.test does not import under the shims
        sys.path.insert(0, os.path.join(REF, "lib_vos", "tools"))
        import vos_test as ref_test
        source = "lib_vos/tools/vos_test.py"
    sys.path.insert(0, os.path.join(REF, "lib_vos", "tools"))
    import vos_test  # the fork's box_results_with_nms_and_limit

    rng = np.random.default_rng(20261020)
    im = rng.integers(0, 256, (IM_H, IM_W, 3), dtype=np.uint8)
    T = 2 + 2 * len(AUG_SCALES)
    all_scores = distinct_scores(rng, T * R * K).reshape(T, R, K)
    centres = rng.uniform([15, 15], [IM_W - 15, IM_H - 15], (12, 2))
    state = {"bbox_calls": [], "mask_calls": [], "body_calls": [], "rois": [], "deltas": [],
             "im_scale": [], "mask_boxes": [], "view_masks": None}

    def flipped(a):
        if np.array_equal(a, im):
            return False
        assert np.array_equal(a, im[:, ::-1, :])
        return True

    def scale_of(a, target_scale, target_max_size):
        return blob_utils.get_target_scale(min(a.shape[:2]), max(a.shape[:2]), target_scale,
                                           target_max_size)

    def im_detect_bbox(model, a, target_scale, target_max_size, boxes=None):
        t = len(state["bbox_calls"])
        hf = flipped(a)
        im_scale = scale_of(a, target_scale, target_max_size)
        state["bbox_calls"].append((target_scale, target_max_size, int(hf)))
        c = centres[rng.integers(0, len(centres), R)] + rng.normal(0, 4, (R, 2))
        wh = rng.uniform(8, 50, (R, 2))
        box = np.clip(np.hstack([c - wh / 2, c + wh / 2]), 0,
                      [IM_W - 1, IM_H - 1, IM_W - 1, IM_H - 1])
        if hf:  # the network saw the flipped frame
            box = box_utils.flip_boxes(box, IM_W)
        rois = np.zeros((R, 5), np.float32)
        rois[:, 1:] = (box * im_scale).astype(np.float32)
        deltas = rng.normal(0, 0.3, (R, 4 * K)).astype(np.float32)
        # im_detect_bbox's own decode (test.py:157-179)
        pred = box_utils.bbox_transform(rois[:, 1:5] / im_scale, deltas, WEIGHTS)
        pred = box_utils.clip_tiled_boxes(pred, a.shape)
        state["rois"].append(rois)
        state["deltas"].append(deltas)
        state["im_scale"].append(im_scale)
        return all_scores[t], pred, im_scale, ("blob_conv", t)

    def im_conv_body_only(model, a, target_scale, target_max_size):
        state["body_calls"].append((target_scale, target_max_size, int(flipped(a))))
        return ("blob_conv", "mask"), scale_of(a, target_scale, target_max_size)

    def im_detect_mask(model, im_scale, boxes, blob_conv):
        t = len(state["mask_calls"])
        state["mask_calls"].append(float(im_scale))
        state["mask_boxes"].append(np.array(boxes, copy=True))
        return state["view_masks"][t]

    ref_test.im_detect_bbox = im_detect_bbox
    ref_test.im_conv_body_only = im_conv_body_only
    ref_test.im_detect_mask = im_detect_mask

    cfg.MODEL.NUM_CLASSES = K
    cfg.MODEL.FASTER_RCNN = True
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = TEST_SCALE, TEST_MAX_SIZE
    cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = 0.05, 0.5, M
    for aug in (cfg.TEST.BBOX_AUG, cfg.TEST.MASK_AUG):
        aug.ENABLED, aug.H_FLIP, aug.SCALE_H_FLIP = True, True, True
        aug.SCALES, aug.MAX_SIZE = AUG_SCALES, AUG_MAX_SIZE
    cfg.TEST.BBOX_AUG.SCORE_HEUR = cfg.TEST.BBOX_AUG.COORD_HEUR = "UNION"

    scores_c, boxes_c, im_scale_i, blob_conv_i = ref_test.im_detect_bbox_aug(None, im)
    assert len(state["bbox_calls"]) == T and scores_c.shape == (T * R, K)
    out = dict(source=np.array(source), im=im, bbox_calls=np.array(state["bbox_calls"], np.float64),
               view_rois=np.stack(state["rois"]), view_deltas=np.stack(state["deltas"]),
               view_scores=all_scores, view_im_scale=np.array(state["im_scale"], np.float64),
               scores_c=scores_c, boxes_c=boxes_c, im_scale_i=np.float64(im_scale_i),
               test_cfg=np.array([0.05, 0.5, M], np.float64),
               weights=np.array(WEIGHTS, np.float64))
    for name, vote in (("plain", False), ("vote", True)):
        cfg.TEST.BBOX_VOTE.ENABLED = vote
        cfg.TEST.BBOX_VOTE.SCORING_METHOD, cfg.TEST.BBOX_VOTE.VOTE_TH = "AVG", 0.9
        _, _, cls_b = vos_test.box_results_with_nms_and_limit(scores_c, boxes_c)
        out["det_%s_dets" % name] = np.vstack([cls_b[j] for j in range(1, K)]).astype(
            np.float32).reshape(-1, 5)
        out["det_%s_cls" % name] = np.concatenate(
            [[j] * len(cls_b[j]) for j in range(1, K)]).astype(np.int32)
    cfg.TEST.BBOX_VOTE.ENABLED = False
    out["vote_cfg"] = np.array([0.9], np.float64)
    boxes = out["det_plain_dets"][:, :4]
    assert len(boxes) == M, len(boxes)

    # masks: the sigmoid outputs of every view, with exact 0 / 1 / 1e-20 planted
    vm = rng.uniform(0, 1, (T, M, K, RES, RES)).astype(np.float32)
    vm[1, 0, :, 3, 4], vm[2, 1, :, 5, 6], vm[3, 2, :, 7, 8] = 0.0, 1.0, 1e-20
    state["view_masks"] = vm
    for heur in ("SOFT_AVG", "SOFT_MAX", "LOGIT_AVG"):
        cfg.TEST.MASK_AUG.HEUR = heur
        state["mask_calls"], state["body_calls"], state["mask_boxes"] = [], [], []
        with np.errstate(divide="ignore", over="ignore"):
            masks_c = ref_test.im_detect_mask_aug(None, im, boxes, im_scale_i, blob_conv_i)
        assert len(state["mask_calls"]) == T
        out["masks_c_%s" % heur] = np.asarray(masks_c, np.float32)
        assert out["masks_c_%s" % heur].dtype == np.asarray(masks_c).dtype
    # the identity view calls im_detect_mask directly; every other view runs the body first
    out.update(view_masks=vm, mask_boxes=np.stack(state["mask_boxes"]),
               mask_im_scale=np.array(state["mask_calls"], np.float64),
               body_calls=np.array(state["body_calls"], np.float64))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "tta.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %s, %d box views, %d detections"
          % (path, os.path.getsize(path), source, T, M))


if __name__ == "__main__":
    main()
