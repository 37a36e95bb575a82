#!/usr/bin/env python3
"""tests/golden/tta_ar.npz: the reference's own im_detect_bbox_aug, im_detect_mask_aug
and im_detect_keypoints_aug (lib/core/test.py:193-363, 405-526, 567-702) executed in
this container with TEST.{BBOX,MASK,KPS}_AUG.ASPECT_RATIOS and ASPECT_RATIO_H_FLIP on
recorded per-view network outputs.

As in gen_tta_goldens.py the network calls -- im_detect_bbox, im_conv_body_only,
im_detect_mask, im_detect_keypoints -- are stubs that log their arguments and return
recorded arrays; everything between them (aspect_ratio_rel, box_utils.aspect_ratio,
the flips, the view order, np.vstack, the mask heuristics, the keypoint tags) is the
reference's code.  cv2 is not importable here: the shimmed cv2.resize is backed by
tests/aspect_ref.resize_width_u8, the numpy restatement of OpenCV's 8-bit INTER_LINEAR
path, and asserts that only the width changes.  Only data is written.

Size: tta.npz's -- R = 200 proposals per view, K = 5 classes, M = 7 detections with
14 x 14 masks, a 96 x 133 frame (odd width), tie-free scores -- with T = 7 box views:
H_FLIP, one scale (64), the ratios 0.75 and 1.5 each with its flip, the identity view.

Usage: python tools/gen_tta_ar_goldens.py   (writes tests/golden/tta_ar.npz)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_goldens import OUT, REF, REPO, distinct_scores, install_shims  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
import aspect_ref  # noqa: E402

TEST_SCALE, TEST_MAX_SIZE = 96, 133
AUG_SCALES, AUG_MAX_SIZE = (64,), 192
RATIOS = (0.75, 1.5)
R, K, M, RES = 200, 5, 7, 14
KP_K, KP_RES = 17, 2
IM_H, IM_W = 96, 133
WEIGHTS = (10., 10., 5., 5.)


def main():
    install_shims()
    import cv2

    def resize(src, dsize=None, *args, **kw):
        assert not args and not kw and dsize is not None and dsize[1] == src.shape[0]
        return aspect_ref.resize_width_u8(src, int(dsize[0]))

    cv2.resize = resize
    from core.config import cfg
    import utils.blob as blob_utils
    import utils.boxes as box_utils
    import utils.image as image_utils
    try:
        import core.test as ref_test
        source = "lib/core/test.py"
    except Exception:  # core.test does not import under the shims
        sys.path.insert(0, os.path.join(REF, "lib_vos", "tools"))
        import vos_test as ref_test
        source = "lib_vos/tools/vos_test.py"
    sys.path.insert(0, os.path.join(REF, "lib_vos", "tools"))
    import vos_test  # the fork's box_results_with_nms_and_limit
    for name in ("im_detect_bbox_aspect_ratio", "im_detect_mask_aspect_ratio",
                 "im_detect_keypoints_aspect_ratio"):
        assert hasattr(ref_test, name), (source, name)
    assert image_utils.cv2 is cv2

    rng = np.random.default_rng(20261022)
    im = rng.integers(0, 256, (IM_H, IM_W, 3), dtype=np.uint8)
    # the images a stub may be handed: (ar or 0, hflip) -> array
    seen = {(0.0, 0): im, (0.0, 1): im[:, ::-1, :]}
    for ar in RATIOS:
        im_ar = image_utils.aspect_ratio_rel(im, ar)
        assert im_ar.dtype == np.uint8 and im_ar.shape == (IM_H, int(round(ar * IM_W)), 3)
        seen[(ar, 0)], seen[(ar, 1)] = im_ar, im_ar[:, ::-1, :]

    def which(a):
        for key, img in seen.items():
            if a.shape == img.shape and np.array_equal(a, img):
                return key
        raise AssertionError("a stub was handed an unknown image %s" % (a.shape,))

    T = 2 + len(AUG_SCALES) + 2 * len(RATIOS)
    all_scores = distinct_scores(rng, T * R * K).reshape(T, R, K)
    centres = rng.uniform([15, 15], [IM_W - 15, IM_H - 15], (12, 2))
    state = {"bbox_calls": [], "mask_calls": [], "body_calls": [], "rois": [], "deltas": [],
             "im_scale": [], "mask_boxes": [], "view_masks": None, "im_shapes": [],
             "kps_boxes": [], "kps_scales": [], "kps_tags": None}

    def scale_of(a, target_scale, target_max_size):
        return blob_utils.get_target_scale(min(a.shape[:2]), max(a.shape[:2]), target_scale,
                                           target_max_size)

    def im_detect_bbox(model, a, target_scale, target_max_size, boxes=None):
        t = len(state["bbox_calls"])
        ar, hf = which(a)
        im_scale = scale_of(a, target_scale, target_max_size)
        state["bbox_calls"].append((target_scale, target_max_size, hf, ar))
        state["im_shapes"].append(a.shape[:2])
        c = centres[rng.integers(0, len(centres), R)] + rng.normal(0, 4, (R, 2))
        wh = rng.uniform(8, 50, (R, 2))
        box = np.clip(np.hstack([c - wh / 2, c + wh / 2]), 0,
                      [IM_W - 1, IM_H - 1, IM_W - 1, IM_H - 1])
        if ar:  # the network saw im_ar
            box = box_utils.aspect_ratio(box, ar)
        if hf:  # ... flipped
            box = box_utils.flip_boxes(box, a.shape[1])
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
        ar, hf = which(a)
        state["body_calls"].append((target_scale, target_max_size, hf, ar) + a.shape[:2])
        return ("blob_conv", "head"), scale_of(a, target_scale, target_max_size)

    def im_detect_mask(model, im_scale, boxes, blob_conv):
        t = len(state["mask_calls"])
        state["mask_calls"].append(float(im_scale))
        state["mask_boxes"].append(np.array(boxes, copy=True))
        return state["view_masks"][t]

    def im_detect_keypoints(model, im_scale, boxes, blob_conv):
        state["kps_scales"].append(float(im_scale))
        state["kps_boxes"].append(np.array(boxes, copy=True))
        return rng.standard_normal((len(boxes), KP_K, KP_RES, KP_RES)).astype(np.float32)

    def combine_heatmaps_size_dep(hms_ts, ds_ts, us_ts, boxes, heur_f):
        state["kps_tags"] = (list(ds_ts), list(us_ts))  # the tags are what is recorded
        return heur_f(hms_ts)

    ref_test.im_detect_bbox = im_detect_bbox
    ref_test.im_conv_body_only = im_conv_body_only
    ref_test.im_detect_mask = im_detect_mask
    ref_test.im_detect_keypoints = im_detect_keypoints
    ref_test.combine_heatmaps_size_dep = combine_heatmaps_size_dep

    cfg.MODEL.NUM_CLASSES = K
    cfg.MODEL.FASTER_RCNN = True
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = TEST_SCALE, TEST_MAX_SIZE
    cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = 0.05, 0.5, M
    for aug in (cfg.TEST.BBOX_AUG, cfg.TEST.MASK_AUG, cfg.TEST.KPS_AUG):
        aug.ENABLED, aug.H_FLIP, aug.SCALE_H_FLIP = True, True, False
        aug.SCALES, aug.MAX_SIZE = AUG_SCALES, AUG_MAX_SIZE
        aug.ASPECT_RATIOS, aug.ASPECT_RATIO_H_FLIP = RATIOS, True
    cfg.TEST.BBOX_AUG.SCORE_HEUR = cfg.TEST.BBOX_AUG.COORD_HEUR = "UNION"

    scores_c, boxes_c, im_scale_i, blob_conv_i = ref_test.im_detect_bbox_aug(None, im)
    assert len(state["bbox_calls"]) == T and scores_c.shape == (T * R, K)
    assert boxes_c.dtype == np.float32
    out = dict(source=np.array(source), im=im, ratios=np.array(RATIOS, np.float64),
               aug_scales=np.array(AUG_SCALES + (AUG_MAX_SIZE,), np.float64),
               bbox_calls=np.array(state["bbox_calls"], np.float64),
               bbox_im_shapes=np.array(state["im_shapes"], np.int64),
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

    # masks: the class-selected sigmoid outputs of every view (one class plane per
    # detection keeps the file small: the heuristics are elementwise)
    vm = rng.uniform(0, 1, (T, M, 1, RES, RES)).astype(np.float32)
    vm[1, 0, :, 3, 4], vm[2, 1, :, 5, 6] = 0.0, 1.0
    state["view_masks"] = vm
    for heur in ("SOFT_AVG", "SOFT_MAX"):
        cfg.TEST.MASK_AUG.HEUR = heur
        state["mask_calls"], state["body_calls"], state["mask_boxes"] = [], [], []
        masks_c = ref_test.im_detect_mask_aug(None, im, boxes, im_scale_i, blob_conv_i)
        assert len(state["mask_calls"]) == T
        out["masks_c_%s" % heur] = np.asarray(masks_c, np.float32)
        assert out["masks_c_%s" % heur].dtype == np.asarray(masks_c).dtype
    # the identity view calls im_detect_mask directly; every other view runs the body
    # first: body_calls rows are (scale, max_size, hflip, ar or 0, H, W of the image)
    out.update(view_masks=vm, mask_boxes=np.stack(state["mask_boxes"]),
               mask_im_scale=np.array(state["mask_calls"], np.float64),
               mask_body_calls=np.array(state["body_calls"], np.float64))

    # keypoints: the call order, the boxes of every view and the ds / us tags
    cfg.KRCNN.HEATMAP_SIZE, cfg.KRCNN.NUM_KEYPOINTS = KP_RES, KP_K
    cfg.TEST.KPS_AUG.HEUR, cfg.TEST.KPS_AUG.SCALE_SIZE_DEP = "HM_AVG", True
    state["body_calls"] = []
    ref_test.im_detect_keypoints_aug(None, im, boxes, im_scale_i, blob_conv_i)
    assert len(state["kps_boxes"]) == T and state["kps_tags"] is not None
    out.update(kps_boxes=np.stack(state["kps_boxes"]),
               kps_im_scale=np.array(state["kps_scales"], np.float64),
               kps_body_calls=np.array(state["body_calls"], np.float64),
               kps_ds=np.array(state["kps_tags"][0], np.bool_),
               kps_us=np.array(state["kps_tags"][1], np.bool_))

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "tta_ar.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1 << 20, size
    print("wrote %s (%d bytes): %s, %d box views, %d detections"
          % (path, size, source, T, M))


if __name__ == "__main__":
    main()
