#!/usr/bin/env python3
"""tests/golden/kps_aug.npz: the reference's own im_detect_keypoints_aug
(lib/core/test.py:567-730) and flip_heatmaps (lib/utils/keypoints.py:90-100) executed
in this container on recorded per-view heatmaps.

The network calls -- im_detect_keypoints and im_conv_body_only -- are replaced by stubs
that log their arguments and return recorded random float32 heatmaps; everything between
them (the view order and tags, flip_boxes, flip_heatmaps, np.mean / np.amax,
combine_heatmaps_size_dep) is the reference's code.  Reuses gen_goldens.install_shims;
only data is written.

Size: T = 6 views (H_FLIP, one scale below and one above TEST.SCALE, SCALE_H_FLIP),
6 float32 boxes, K = 17, 12 x 12 heatmaps (KRCNN.HEATMAP_SIZE), a 300 x 451 frame (odd
width), AREA_TH the reference's 180**2.  Box 0 has area exactly 32400 (it counts as
large), box 1 is just under it, boxes 2-3 are small, boxes 4-5 large.  HM_AVG and
HM_MAX, each with and without SCALE_SIZE_DEP.

With one scale below and one above TEST.SCALE every box drops exactly one tagged pair
(area < AREA_TH the downscaled one, any other area the upscaled one), so those runs
divide every row by 4.  Rows with different divisors in one call come from a second
view list with two scales below and one above (T = 8: a small box keeps 4 views, a large
one 6), recorded for both heuristics as combined_*_dep8; the generator asserts that
both counts occur.

Usage: python tools/gen_kps_aug_goldens.py   (writes tests/golden/kps_aug.npz)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_goldens import OUT, REF, install_shims  # noqa: E402

TEST_SCALE, TEST_MAX_SIZE = 300, 451
AUG_SCALES, AUG_MAX_SIZE = (200, 400), 700
AUG_SCALES_8 = (150, 200, 400)
K, RES = 17, 12
IM_H, IM_W = 300, 451
BOXES = [(10, 20, 189, 199),          # 180 x 180 = 32400 exactly: large (>=)
         (10.5, 20, 189.25, 199),     # 179.75 x 180 = 32355: just under
         (300.25, 40.5, 330.75, 90),  # small
         (5, 5, 12.5, 9.25),          # small
         (100, 10, 440.5, 290.75),    # large
         (0, 0, 450, 299)]            # the frame


def main():
    install_shims()
    from core.config import cfg
    import utils.blob as blob_utils
    import utils.boxes as box_utils
    import utils.keypoints as keypoint_utils
    try:
        import core.test as ref_test
        source = "lib/core/test.py"
    except Exception:  # core.test does not import under the shims
        sys.path.insert(0, os.path.join(REF, "lib_vos", "tools"))
        import vos_test as ref_test
        source = "lib_vos/tools/vos_test.py"
    for name in ("im_detect_keypoints_aug", "im_detect_keypoints_hflip",
                 "im_detect_keypoints_scale", "combine_heatmaps_size_dep"):
        assert hasattr(ref_test, name), (source, name)

    rng = np.random.default_rng(20261021)
    im = rng.integers(0, 256, (IM_H, IM_W, 3), dtype=np.uint8)
    boxes = np.asarray(BOXES, np.float32)
    R = len(boxes)
    T8 = 2 + 2 * len(AUG_SCALES_8)
    vh = (rng.standard_normal((T8, R, K, RES, RES)) * 3).astype(np.float32)
    state = {}

    def flipped(a):
        if np.array_equal(a, im):
            return False
        assert np.array_equal(a, im[:, ::-1, :])
        return True

    def im_conv_body_only(model, a, target_scale, target_max_size):
        state["body_calls"].append((target_scale, target_max_size, int(flipped(a))))
        return ("blob_conv", len(state["body_calls"])), blob_utils.get_target_scale(
            min(a.shape[:2]), max(a.shape[:2]), target_scale, target_max_size)

    def im_detect_keypoints(model, im_scale, b, blob_conv):
        t = len(state["head_boxes"])
        state["head_boxes"].append(np.array(b, copy=True))
        state["head_scales"].append(float(im_scale))
        return vh[t].copy()

    ref_test.im_conv_body_only = im_conv_body_only
    ref_test.im_detect_keypoints = im_detect_keypoints

    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = TEST_SCALE, TEST_MAX_SIZE
    cfg.KRCNN.HEATMAP_SIZE, cfg.KRCNN.NUM_KEYPOINTS = RES, K
    aug = cfg.TEST.KPS_AUG
    aug.ENABLED, aug.H_FLIP, aug.SCALE_H_FLIP = True, True, True
    aug.MAX_SIZE = AUG_MAX_SIZE
    assert aug.AREA_TH == 180 ** 2
    im_scale_i = blob_utils.get_target_scale(IM_H, IM_W, TEST_SCALE, TEST_MAX_SIZE)

    # The fork's boxes_area returns (areas, indices of negative areas) for fpn.py's use;
    # combine_heatmaps_size_dep still reads its result as upstream's areas alone and would
    # compare a tuple with AREA_TH.  It is handed the areas -- the first element, the
    # fork's own arithmetic -- and nothing else of the reference is touched.
    fork_boxes_area = box_utils.boxes_area

    class _Areas:
        def __getattr__(self, name):
            return getattr(box_utils, name)

        @staticmethod
        def boxes_area(b):
            return fork_boxes_area(b)[0]

    ref_test.box_utils = _Areas()
    areas = fork_boxes_area(boxes)[0]
    assert areas.dtype == np.float32 and areas[0] == 32400 and 32300 < areas[1] < 32400
    out = dict(source=np.array(source), im_hw=np.array([IM_H, IM_W], np.int64), boxes=boxes,
               areas=areas, area_th=np.float64(aug.AREA_TH), view_heatmaps=vh,
               test_cfg=np.array([TEST_SCALE, TEST_MAX_SIZE, AUG_MAX_SIZE], np.float64),
               aug_scales=np.array(AUG_SCALES, np.float64),
               aug_scales_8=np.array(AUG_SCALES_8, np.float64),
               im_scale_i=np.float64(im_scale_i))

    def run(scales, heur, dep):
        aug.SCALES, aug.HEUR, aug.SCALE_SIZE_DEP = scales, heur, dep
        state.update(body_calls=[], head_boxes=[], head_scales=[])
        c = ref_test.im_detect_keypoints_aug(None, im, boxes, im_scale_i, ("blob_conv", 0))
        T = 2 + 2 * len(scales)
        assert len(state["head_boxes"]) == T and len(state["body_calls"]) == T - 1
        assert c.dtype == np.float32 and c.shape == vh.shape[1:]
        return c

    def t_rows(scales):
        tags = [(False, False)] * 2 + [(s < TEST_SCALE, s > TEST_SCALE)
                                       for s in scales for _ in range(2)]
        return np.array([sum(1 for ds, us in tags
                             if not ((a < aug.AREA_TH and ds) or (a >= aug.AREA_TH and us)))
                         for a in areas], np.int64)

    for heur in ("HM_AVG", "HM_MAX"):
        for dep in (False, True):
            out["combined_%s_%s" % (heur, "dep" if dep else "all")] = run(AUG_SCALES, heur, dep)
    # the call log of the last 6-view run: the same for all four
    out.update(head_boxes=np.stack(state["head_boxes"]),
               head_scales=np.array(state["head_scales"], np.float64),
               body_calls=np.array(state["body_calls"], np.float64))
    out["t_row"] = t_rows(AUG_SCALES)
    assert set(out["t_row"].tolist()) == {4}
    for heur in ("HM_AVG", "HM_MAX"):
        out["combined_%s_dep8" % heur] = run(AUG_SCALES_8, heur, True)
    out["t_row_8"] = t_rows(AUG_SCALES_8)
    assert set(out["t_row_8"].tolist()) == {4, 6}, out["t_row_8"]
    out["body_calls_8"] = np.array(state["body_calls"], np.float64)

    one = vh[0]
    fl = keypoint_utils.flip_heatmaps(one)
    out["flipped_view0"] = np.ascontiguousarray(fl)
    assert fl.dtype == np.float32 and not np.array_equal(fl, one)

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "kps_aug.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)
                  if f != "kps_aug.npz")
    assert size <= min(largest, 1 << 20), (size, largest)
    print("wrote %s (%d bytes): %s, T_row %s / %s" % (path, size, source,
                                                      out["t_row"].tolist(),
                                                      out["t_row_8"].tolist()))


if __name__ == "__main__":
    main()
