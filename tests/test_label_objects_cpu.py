"""The host side of the label-map objects: the numpy restatement (tests/
label_objects_ref.py) against the golden recorded from the reference's own davis_db code
(tools/gen_label_objects_goldens.py), the RLE's round trip, and the refusals that come
before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import label_objects_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_objects.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _rle_rows(flat, n):
    return np.split(flat, np.cumsum(n)[:-1]) if len(n) else []


def test_restatement_equals_golden(golden):
    lab = golden["labels"]
    assert np.array_equal(lab, R.golden_frame())
    assert np.array_equal(R.remap(lab), golden["gt"])
    assert (lab == 255).any() and not (golden["gt"] == 255).any()
    # get_bboxes (after get_gt) and get_cls_mapper's float32 box form
    rect = R.objects(lab, expand=None, remap255=True)
    assert np.array_equal(rect["rects"], golden["bboxes_xywh"])
    assert rect["boxes"].dtype == np.float32
    assert np.array_equal(rect["boxes"].view(np.int32), golden["rect_boxes"].view(np.int32))
    # add_gt_annotations_to_entry on the raw map and on get_gt's map
    for tag, remap255 in (("raw", False), ("gt", True)):
        o = R.objects(lab, expand=float(golden["expand"]), remap255=remap255)
        assert np.array_equal(o["boxes"].view(np.int32), golden[tag + "_boxes"].view(np.int32)), tag
        assert np.array_equal(o["areas"].astype(np.float32), golden[tag + "_seg_areas"]), tag
        assert np.array_equal(o["ids"].astype(np.int32), golden[tag + "_instance_id"]), tag
        assert np.array_equal(np.asarray([len(r) for r in o["rle"]], np.int32),
                              golden[tag + "_rle_n"]), tag
        assert np.array_equal(np.concatenate(o["rle"]), golden[tag + "_rle"]), tag
    assert golden["raw_instance_id"][-1] == 255 and golden["gt_instance_id"].max() < 255
    # the same frame given already remapped needs no remap255
    o2 = R.objects(golden["gt"], expand=float(golden["expand"]))
    assert np.array_equal(o2["boxes"], golden["gt_boxes"])


def test_rle_round_trip(golden):
    rng = np.random.default_rng(7)
    maps = [golden["labels"], R.checkerboard(16, 16, 1, 2), np.full((5, 9), 3, np.uint8),
            np.zeros((4, 4), np.uint8), rng.integers(0, 4, (13, 7), dtype=np.uint8),
            R.blobs(65, 3, 2), R.blobs(130, 2, 2)]
    for lab in maps:
        h, w = lab.shape
        o = R.objects(lab, expand=None)
        assert list(o["ids"]) == [v for v in np.unique(lab) if v]
        for v, rect, area, runs in zip(o["ids"], o["rects"], o["areas"], o["rle"]):
            assert int(runs.astype(np.int64).sum()) == h * w
            plane = R.rle_decode_counts(runs, h, w)
            assert np.array_equal(plane, (lab == v).astype(np.uint8))
            assert area == int(plane.sum()) == int(runs[1::2].astype(np.int64).sum())
            x, y, bw, bh = rect
            assert plane[y:y + bh, x:x + bw].sum() == area
            assert plane[y].any() and plane[y + bh - 1].any()
            assert plane[:, x].any() and plane[:, x + bw - 1].any()
    # a set first pixel: the first run is the empty zero run
    assert R.rle_counts(np.ones((2, 3), np.uint8)).tolist() == [0, 6]
    assert R.rle_counts(np.array([[0, 1], [1, 0]], np.uint8)).tolist() == [1, 2, 1]


def test_oracle_entry_form_filter():
    """Of the restatement alone (it passes without the feature).  1 x 7: every object is
    dropped by y2 > y1 (the clip leaves y1 == y2 == 0); the rect form keeps them."""
    lab = np.array([[1, 1, 0, 2, 0, 3, 3]], np.uint8)
    assert len(R.objects(lab, expand=0.05)["ids"]) == 0
    o = R.objects(lab, expand=None)
    assert o["ids"].tolist() == [1, 2, 3]
    assert o["boxes"].tolist() == [[0, 0, 2, 1], [3, 0, 4, 1], [5, 0, 7, 1]]


def test_remap_rules():
    """The restatement and davis_db.get_gt (torch, on the host here) on get_gt's cases."""
    from vosdetectron_amd import davis_db
    for lab, want in (([[0, 1, 2, 255]], [[0, 1, 2, 3]]),
                      ([[0, 1, 3, 255]], [[0, 1, 3, 3]]),     # 255 merges into 3
                      ([[1, 255]], [[1, 1]]),                 # no zero: len(vals) - 1 == 1
                      ([[255, 255]], [[0, 0]]),               # 255 alone becomes background
                      ([[0, 7]], [[0, 7]])):
        lab = np.array(lab, np.uint8)
        assert R.remap(lab).tolist() == want
        assert davis_db.get_gt(torch.from_numpy(lab)).tolist() == want
        assert davis_db.get_gt(torch.from_numpy(lab[None]))[0].tolist() == want
    # more pixels than one scatter chunk, the 255 in the last one
    big = np.zeros((3, davis_db._GT_CHUNK + 5), np.uint8)
    big[1, 7], big[2, -1], big[0, 3] = 4, 255, 9
    assert np.array_equal(davis_db.get_gt(torch.from_numpy(big)).numpy(), R.remap(big))
    assert R.remap(big)[2, -1] == 3


def test_get_gt_torch(golden):
    from vosdetectron_amd import davis_db
    maps = [golden["labels"], np.array(golden["labels"]) % 7]
    maps[1][0, 0] = 255
    lab = torch.from_numpy(np.stack(maps))
    got = davis_db.get_gt(lab).numpy()
    assert got.dtype == np.uint8
    for f in range(2):
        assert np.array_equal(got[f], R.remap(maps[f])), f
    assert np.array_equal(davis_db.get_gt(lab[0]).numpy(), golden["gt"])


# --------------------------------------------------------------------------- the C entry
def _lib():
    from vosdetectron_amd import _lib
    return _lib


def test_workspace_size():
    L = _lib().lib()
    assert L.vd_label_objects_workspace_size(3, 37, 83, 255) == 3 * (5136 + 32 * 255)
    assert L.vd_label_objects_workspace_size(1, 1, 1, 1) == 5136 + 32
    for F, H, W, cap in ((0, 5, 5, 4), (65536, 5, 5, 4), (1, 0, 5, 4), (1, 5, 0, 4), (1, 5, 8193, 4),
                         (1, 1 << 20, 1 << 11, 4), (1, 5, 5, 0), (1, 5, 5, 256), (-1, 5, 5, 4)):
        assert L.vd_label_objects_workspace_size(F, H, W, cap) == 0, (F, H, W, cap)
    assert L.vd_label_objects_workspace_size(1, (1 << 20) - 1, 1 << 11, 4) > 0


def test_refusals_before_any_launch():
    """Every refusal returns its code on the host; the pointers are never followed."""
    lib = _lib()
    L = lib.lib()
    F, H, W, cap = 2, 5, 3, 4
    size = L.vd_label_objects_workspace_size(F, H, W, cap)
    buf = ctypes.create_string_buffer(size + 16)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(labels=p, F=F, H=H, W=W, remap255=0, expand=0.05, obj_cap=cap, rle_cap=8, ids=p,
             rects=p, areas=p, boxes=p, counts=p, rle_counts=p, rle_n=p, ws=p, wsb=size):
        return L.vd_label_objects(labels, F, H, W, remap255, expand, obj_cap, rle_cap, ids, rects,
                                  areas, boxes, counts, rle_counts, rle_n, ws, wsb, None)

    for name in ("labels", "ids", "rects", "areas", "boxes", "counts", "rle_counts", "rle_n", "ws"):
        assert call(**{name: None}) == lib.VD_ERR_ARG, name
    for kw in ({"remap255": 2}, {"rle_cap": -1}, {"expand": float("nan")}, {"F": -1},
               {"ws": p + 4}):
        assert call(**kw) == lib.VD_ERR_ARG, kw
    for kw in ({"obj_cap": 0}, {"obj_cap": 256}, {"H": 0}, {"W": 0}, {"W": 8193}, {"F": 65536},
               {"H": 1 << 20, "W": 1 << 11}):
        assert call(**kw) == lib.VD_ERR_SHAPE, kw
    assert call(wsb=size - 1) == lib.VD_ERR_WORKSPACE
    assert call(F=0) == lib.VD_OK
    assert call(F=0, labels=None, ws=None) == lib.VD_OK


def test_wrapper_refusals():
    from vosdetectron_amd import engine, ops
    with pytest.raises(ValueError, match="device"):
        ops.label_objects(torch.zeros((1, 4, 4), dtype=torch.uint8))
    for out in ({"frame_hw": [(30, 40)]}, {"im_hw": None}):
        with pytest.raises(NotImplementedError, match="RaggedFramePipeline"):
            engine.frame_label_objects(None, out, gt_thresh=0.5)
    with pytest.raises(ValueError, match="which"):
        engine.frame_label_objects(None, {}, which="both")
