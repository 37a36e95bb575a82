"""Label maps (viz_mask_result) without a device: the numpy restatement against the
executed reference (tests/golden/label_map.npz, tools/gen_label_map_goldens.py), the two
forms of the restatement against each other on tied scores, and the argument checks that
come before any launch."""
import numpy as np
import pytest

from tests import label_map_ref as lm


def test_restatement_equals_the_executed_reference(golden):
    g = golden("label_map")
    masks, dets, classes = g["masks"], g["dets"], g["classes"]
    m2, d2, c2 = lm.make(0, distinct=True)
    assert np.array_equal(masks, m2) and np.array_equal(dets, d2) and np.array_equal(classes, c2)
    assert np.unique(dets[:, 4]).size == lm.N and tuple(g["im_hw"]) == (lm.H, lm.W)
    thresh, gt_thresh = float(g["thresh"]), float(g["rvt_cls_threshold"])
    assert (thresh, gt_thresh) == (lm.THRESH, lm.GT_THRESH)
    planes = lm.planes_of(masks, dets)
    label, gt = lm.paint(planes, dets[:, 4], classes, thresh, gt_thresh)
    assert np.array_equal(label, g["outImg"])
    assert np.array_equal(gt, g["rtv_gt"])
    assert (g["outImg"] != g["rtv_gt"]).any()
    bb = lm.bboxs(dets, classes, thresh, gt_thresh)
    rows = np.asarray([np.concatenate([[c], b]) for c, bl in enumerate(bb) for b in bl],
                      np.float32).reshape(-1, 5)
    assert np.array_equal(rows, g["rtv_bboxs"]) and len(rows) > 0
    # the first-hit form on the same inputs
    l2, g2 = lm.first_hit(planes, dets[:, 4], classes, thresh, gt_thresh)
    assert np.array_equal(l2, g["outImg"]) and np.array_equal(g2, g["rtv_gt"])


@pytest.mark.parametrize("r", [28, 14])
def test_paint_equals_first_hit_on_ties(r):
    masks, dets, classes, planes, stats = lm.inputs(r)
    valid = np.ones(lm.N, np.uint8)
    valid[::3] = 0
    lut = ((np.arange(64) * 37 + 11) % 256).astype(np.uint8)
    for kw in ({}, {"valid": valid}, {"lut": lut}):
        a = lm.paint(planes, dets[:, 4], classes, lm.THRESH, lm.GT_THRESH, **kw)
        b = lm.first_hit(planes, dets[:, 4], classes, lm.THRESH, lm.GT_THRESH, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), kw
    # the tie rule is visible: where rows 5 and 6 both cover and nothing higher does,
    # row 6 (or 7, the same score and a higher row) is what the map shows
    label, _ = lm.paint(planes, dets[:, 4], classes, lm.THRESH, lm.GT_THRESH)
    both = (planes[5] > 0) & (planes[6] > 0)
    higher = np.zeros_like(both)
    for i in np.flatnonzero(dets[:, 4] > dets[5, 4]):
        higher |= planes[i] > 0
    seen = label[both & ~higher]
    assert seen.size >= 20 and set(seen.tolist()) <= {int(classes[6]), int(classes[7])}
    assert int(classes[6]) in seen


def test_painting_order_of_the_package_is_the_restatement():
    from vosdetectron_amd import vis
    _, dets, _, _, _ = lm.inputs()
    assert np.array_equal(vis.painting_order(dets[:, 4], lm.THRESH),
                          lm.order_of(dets[:, 4], lm.THRESH))
    # float32 rule: a score equal to float32(thresh) is painted, the next one below is not
    t = np.float32(0.3)
    s = np.array([t, np.nextafter(t, np.float32(0))], np.float32)
    assert vis.painting_order(s, 0.3).tolist() == [0]
    assert float(t) > 0.3  # in float64 the comparison would come out the same here, and
    s = np.array([np.float32(0.1)], np.float32)  # here it would not: float32(0.1) > 0.1
    assert float(s[0]) > 0.1 and vis.painting_order(s, 0.1).tolist() == [0]
    t6 = np.float32(0.6)  # float32(0.6) > 0.6 in float64, equal in float32: not `>`
    assert float(t6) > 0.6 and not (t6 > np.float32(0.6))


def test_ragged_outputs_are_refused():
    from vosdetectron_amd import engine
    for out in ({"frame_hw": [(30, 40)]}, {"im_hw": None}):
        with pytest.raises(NotImplementedError, match="RaggedFramePipeline"):
            engine.frame_label_maps(None, out)


def test_lut_checks_need_no_device():
    import torch
    from vosdetectron_amd import ops
    for bad in ([], np.zeros((2, 2), np.uint8), [1, 256], [-1], [0.5, 1.0]):
        with pytest.raises(ValueError, match="lut"):
            ops.label_lut(bad)
        with pytest.raises(ValueError, match="lut"):  # before any tensor is looked at
            ops.label_maps(torch.zeros((1, 28, 28)), torch.zeros((1, 1, 5)),
                           torch.zeros((1, 1), dtype=torch.int32),
                           torch.zeros((1,), dtype=torch.int32), 8, 8, 0.5, lut=bad)
    assert ops.label_lut([0, 255, 3]).dtype == np.uint8


def test_c_abi_refusals_without_a_device():
    """Every refusal comes before the first launch; the pointers are never followed."""
    import ctypes
    from vosdetectron_amd import _lib
    L = _lib.lib()
    F, cap = 3, 24
    size = L.vd_label_maps_workspace_size(F, cap)
    assert size >= F * 4 + F * cap * 8
    assert L.vd_label_maps_workspace_size(F, 256) > size
    assert L.vd_label_maps_workspace_size(F, 1 << 20) == 0  # above the kernel's limit
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(masks=p, R=28, dets=p, classes=p, counts=p, valid=None, F=F, cap=cap, h=37, w=83,
             lut=None, lut_n=0, label=p, gt=p, ws=p, wsb=size):
        return L.vd_label_maps(masks, R, dets, classes, counts, valid, F, cap, h, w, 0.5, 0.25,
                               0.6, lut, lut_n, label, gt, ws, wsb, None)

    for name in ("masks", "dets", "classes", "counts", "label", "ws"):
        assert call(**{name: None}) == _lib.VD_ERR_ARG, name
    assert call(lut=p, lut_n=0) == _lib.VD_ERR_ARG
    for kw in ({"R": 0}, {"R": 63}, {"h": 0}, {"w": 0}, {"cap": 1 << 20}, {"cap": 0}):
        assert call(**kw) == _lib.VD_ERR_SHAPE, kw
    assert call(wsb=size - 1) == _lib.VD_ERR_WORKSPACE
    assert call(wsb=0) == _lib.VD_ERR_WORKSPACE
    assert call(F=0) == _lib.VD_OK  # nothing to do
