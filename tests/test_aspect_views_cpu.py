"""Aspect-ratio views of the test-time augmentation without a device: the opt-in and
its refusals, the view order against the executed reference's call log, boxes.
aspect_ratio, known answers of tests/aspect_ref.py (the numpy restatement the GPU tests
compare with), aspect_ref's box maps against tests/golden/tta_ar.npz -- the reference's
own im_detect_*_aug executed by tools/gen_tta_ar_goldens.py -- and the C ABI's argument
checks."""
import ctypes
import os

import numpy as np
import pytest

from tests import aspect_ref
from vosdetectron_amd import config as vcfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta_ar.npz")
KEYS = ("TEST.BBOX_AUG.ASPECT_RATIOS", "TEST.MASK_AUG.ASPECT_RATIOS",
        "TEST.KPS_AUG.ASPECT_RATIOS")
KP = {"MODEL.KEYPOINTS_ON": True, "MODEL.MASK_ON": False, "FPN.FPN_ON": True,
      "KRCNN.ROI_KEYPOINTS_HEAD": vcfg.KEYPOINT_HEAD}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _golden_overrides(z, kps=False):
    """The generator's configuration as overrides."""
    s, ms = z["aug_scales"][:-1], z["aug_scales"][-1]
    o = {"TEST.SCALE": 96, "TEST.MAX_SIZE": 133}
    if kps:
        o.update(KP)
    for name in ("BBOX_AUG", "KPS_AUG" if kps else "MASK_AUG"):
        o.update({"TEST.%s.ENABLED" % name: True, "TEST.%s.H_FLIP" % name: True,
                  "TEST.%s.SCALES" % name: tuple(int(x) for x in s),
                  "TEST.%s.MAX_SIZE" % name: int(ms), "TEST.%s.SCALE_H_FLIP" % name: False,
                  "TEST.%s.ASPECT_RATIOS" % name: tuple(float(r) for r in z["ratios"]),
                  "TEST.%s.ASPECT_RATIO_H_FLIP" % name: True})
    return o


def _as_calls(views):
    """Views as the golden's call rows (scale, max_size, hflip, ar or 0)."""
    return [[float(v[0]), float(v[1]), float(v[2]), float(v[3]) if len(v) > 3 else 0.0]
            for v in views]


# --------------------------------------------------------------------------- #
# acceptance                                                                   #
# --------------------------------------------------------------------------- #
def _aug_on(key, val):
    block = key.split(".")[1]
    o = {"TEST.%s.ENABLED" % block: True, key: val}
    if block == "KPS_AUG":
        o.update(KP)
    return o


@pytest.mark.parametrize("key", KEYS)
def test_opt_in_accepts_and_test_aug_alone_refuses(key):
    o = _aug_on(key, (0.5, 2.0))
    cfg = vcfg.load_cfg(overrides=o, test_aug=True, aspect_views=True)
    assert tuple(cfg.TEST[key.split(".")[1]].ASPECT_RATIOS) == (0.5, 2.0)
    vcfg.check_supported(cfg, test_aug=True, aspect_views=True)
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")) as e:
        vcfg.load_cfg(overrides=o, test_aug=True)
    assert "aspect_views=True" in str(e.value)
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        vcfg.check_supported(cfg, test_aug=True)
    with pytest.raises(NotImplementedError):  # the default load refuses the AUG block itself
        vcfg.load_cfg(overrides=o)
    with pytest.raises(NotImplementedError):  # the opt-in means nothing without test_aug
        vcfg.load_cfg(overrides=o, aspect_views=True)


def test_opt_in_drops_only_the_aspect_refusals():
    for key, val in (("TEST.BBOX_AUG.SCALE_SIZE_DEP", True), ("TEST.BBOX_AUG.SCORE_HEUR", "AVG"),
                     ("TEST.MASK_AUG.SCALE_SIZE_DEP", True), ("TEST.MASK_AUG.HEUR", "HARD_AVG")):
        with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
            vcfg.load_cfg(overrides=_aug_on(key, val), test_aug=True, aspect_views=True)
    assert set(vcfg.ASPECT_VIEW_KEYS) == set(KEYS)


@pytest.mark.parametrize("bad", [0.0, -0.5, float("inf"), float("nan"), "wide", True])
def test_bad_ratios_are_refused(bad):
    for key in KEYS:
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            vcfg.load_cfg(overrides=_aug_on(key, (0.5, bad)), test_aug=True, aspect_views=True)


def test_ratio_under_two_columns_is_refused():
    cfg = vcfg.load_cfg(overrides=_aug_on(KEYS[0], (0.01, 0.5)), test_aug=True,
                        aspect_views=True)
    vcfg.check_aspect_ratios(cfg, 1333)  # 13 columns
    vcfg.check_aspect_ratios(cfg, 150)   # round(1.5) = 2 columns
    with pytest.raises(ValueError, match=r"0\.01.*under 2"):
        vcfg.check_aspect_ratios(cfg, 149)  # round(1.49) = 1
    assert vcfg.aspect_width(133, 0.75) == 100 and vcfg.aspect_width(133, 1.5) == 200
    assert vcfg.aspect_width(5, 0.5) == 2 and vcfg.aspect_width(7, 0.5) == 4  # half to even


# --------------------------------------------------------------------------- #
# view order                                                                   #
# --------------------------------------------------------------------------- #
def test_view_order_is_the_references_call_order(gold):
    cfg = vcfg.load_cfg(overrides=_golden_overrides(gold), test_aug=True, aspect_views=True)
    box, mask = vcfg.aug_views(cfg)
    assert _as_calls(box) == gold["bbox_calls"].tolist()
    # the identity view calls im_detect_mask on the kept blob_conv: no body call
    assert _as_calls(mask[1:]) == gold["mask_body_calls"][:, :4].tolist()
    assert mask[0] == (96, 133, False) and box[-1] == (96, 133, False)
    for v in box + mask:  # only aspect-ratio views are 4-tuples
        assert len(v) == (4 if v in [(96, 133, hf, ar) for hf in (False, True)
                                     for ar in gold["ratios"]] else 3)
    # the images the stubs received: H unchanged, War = int(round(ar * W))
    H, W = gold["im"].shape[:2]
    for v, shape in zip(box, gold["bbox_im_shapes"].tolist()):
        assert shape == [H, aspect_ref.aspect_width(W, v[3]) if len(v) > 3 else W]


def test_keypoint_view_order_and_tags(gold):
    cfg = vcfg.load_cfg(overrides=_golden_overrides(gold, kps=True), test_aug=True,
                        aspect_views=True)
    views, ds, us = vcfg.kps_aug_views(cfg)
    assert _as_calls(views[1:]) == gold["kps_body_calls"][:, :4].tolist()
    assert ds == gold["kps_ds"].tolist() and us == gold["kps_us"].tolist()
    assert not any(d or u for v, d, u in zip(views, ds, us) if len(v) > 3)
    assert vcfg.aug_views(cfg)[0] == vcfg.aug_views(
        vcfg.load_cfg(overrides=_golden_overrides(gold), test_aug=True, aspect_views=True))[0]


def test_views_without_ratios_are_unchanged():
    o = {"TEST.BBOX_AUG.ENABLED": True, "TEST.BBOX_AUG.H_FLIP": True,
         "TEST.BBOX_AUG.ASPECT_RATIO_H_FLIP": True}
    a = vcfg.aug_views(vcfg.load_cfg(overrides=o, test_aug=True))
    b = vcfg.aug_views(vcfg.load_cfg(overrides=o, test_aug=True, aspect_views=True))
    assert a == b == ([(600, 1000, True), (600, 1000, False)], [(600, 1000, False)])


# --------------------------------------------------------------------------- #
# boxes.aspect_ratio                                                           #
# --------------------------------------------------------------------------- #
def test_aspect_ratio_is_the_reference_expression():
    import torch
    from vosdetectron_amd import boxes as vboxes
    rng = np.random.default_rng(5)
    b = rng.uniform(0, 1300, (64, 8)).astype(np.float32)
    for ar in (0.37, 0.5, 0.75, 1.5, 2.0, 2.6):
        for f in (ar, 1.0 / ar):
            ref = b.copy()
            ref[:, 0::4] = f * b[:, 0::4]
            ref[:, 2::4] = f * b[:, 2::4]
            got = vboxes.aspect_ratio(b, f)
            assert got.dtype == np.float32 and np.array_equal(got, ref)
            assert np.array_equal(got, aspect_ref.aspect_ratio(b, f))
            # the float32 product the kernel evaluates: x * float32(f)
            assert np.array_equal(got[:, 0::4], b[:, 0::4] * np.float32(f))
            assert np.array_equal(got[:, 1::2], b[:, 1::2])  # y untouched
            t = vboxes.aspect_ratio(torch.from_numpy(b), f)
            assert t.dtype == torch.float32 and np.array_equal(t.numpy(), ref)
    assert b is not vboxes.aspect_ratio(b, 1.0) and np.array_equal(vboxes.aspect_ratio(b, 1.0), b)


# --------------------------------------------------------------------------- #
# known answers of the restatement                                             #
# --------------------------------------------------------------------------- #
def test_restatement_identity_ratio():
    rng = np.random.default_rng(7)
    im = rng.integers(0, 256, (9, 53, 3), dtype=np.uint8)
    assert np.array_equal(aspect_ref.aspect_ratio_rel(im, 1.0), im)
    sx, sx1, a0, a1 = aspect_ref.stage1_coeffs(53, 53)
    assert np.array_equal(sx, np.arange(53)) and set(a0.tolist()) == {2048} and not a1.any()


@pytest.mark.parametrize("ar", [0.37, 0.5, 0.75, 1.5, 2.0, 2.6])
def test_restatement_constant_frame_stays_constant(ar):
    for W in (53, 40):
        sx, sx1, a0, a1 = aspect_ref.stage1_coeffs(W, aspect_ref.aspect_width(W, ar))
        assert sx.min() >= 0 and sx1.max() <= W - 1
        for val in (0, 1, 127, 255):
            im = np.full((5, W, 3), val, np.uint8)
            out = aspect_ref.aspect_ratio_rel(im, ar)
            assert out.shape == (5, aspect_ref.aspect_width(W, ar), 3) and out.dtype == np.uint8
            assert (out == val).all(), (ar, W, val, np.unique(out))


def test_restatement_hand_computed_2x_row():
    """W = 4 -> War = 8: scale 0.5, fx = dx / 2 - 0.25.  Interior columns alternate the
    weights (0.75, 0.25) -> (1536, 512) and (0.25, 0.75) -> (512, 1536); column 0 has
    sx = -1 (clamped to the first pixel), column 7 has sx = 3 = W - 1 (the last)."""
    row = np.array([10, 50, 200, 90], np.uint8)
    sx, sx1, a0, a1 = aspect_ref.stage1_coeffs(4, 8)
    assert sx.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and sx1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert a0.tolist() == [2048, 1536, 512, 1536, 512, 1536, 512, 2048]
    assert a1.tolist() == [0, 512, 1536, 512, 1536, 512, 1536, 0]

    def px(s0, s1, w0, w1):  # ((D >> 9) + 2) >> 2 by hand
        return (((s0 * w0 + s1 * w1) >> 9) + 2) >> 2

    want = [10, px(10, 50, 1536, 512), px(10, 50, 512, 1536), px(50, 200, 1536, 512),
            px(50, 200, 512, 1536), px(200, 90, 1536, 512), px(200, 90, 512, 1536), 90]
    assert want == [10, 20, 40, 88, 163, 173, 118, 90]  # 0.75 / 0.25 blends, rounded
    im = np.repeat(row[None, :, None], 3, axis=2)
    assert aspect_ref.resize_width_u8(im, 8)[0, :, 1].tolist() == want


def test_restatement_flip_is_applied_after_the_resize():
    rng = np.random.default_rng(11)
    im = rng.integers(0, 256, (4, 53, 3), dtype=np.uint8)
    for ar in (0.75, 1.37):
        v = aspect_ref.view_image(im, ar, True)
        assert np.array_equal(v, aspect_ref.aspect_ratio_rel(im, ar)[:, ::-1])
    # the row is mirrored, not recomputed: column x of the view is column War-1-x
    sx, sx1, a0, a1 = aspect_ref.stage1_coeffs(53, aspect_ref.aspect_width(53, 1.37))
    v = aspect_ref.view_image(im, 1.37, True)
    x = 5
    D = im[:, sx[-1 - x]].astype(np.int32) * int(a0[-1 - x]) \
        + im[:, sx1[-1 - x]].astype(np.int32) * int(a1[-1 - x])
    assert np.array_equal(v[:, x], (((D >> 9) + 2) >> 2).astype(np.uint8))


def test_view_blob_area_path_case():
    """48 x 40 at ar 2.0 and TEST.SCALE 24: im_ar is 48 x 80, im_scale exactly 0.5."""
    rng = np.random.default_rng(13)
    fr = rng.integers(0, 256, (1, 48, 40, 3), dtype=np.uint8)
    blob, scale = aspect_ref.view_blob(fr, 2.0, False, 24, 1333, 32)
    assert scale == 0.5 and blob.shape == (1, 3, 32, 64)
    assert not blob[:, :, 24:].any() and not blob[:, :, :, 40:].any()
    im_ar = aspect_ref.aspect_ratio_rel(fr[0], 2.0).astype(np.float32)
    from oracle import oracle as orc
    mean = (im_ar - orc.PIXEL_MEANS).astype(np.float32)
    want = (mean[0::2, 0::2] + mean[0::2, 1::2] + mean[1::2, 0::2] + mean[1::2, 1::2]) \
        * np.float32(0.25)
    assert np.array_equal(blob[0, :, :24, :40], want.transpose(2, 0, 1))


# --------------------------------------------------------------------------- #
# aspect_ref's box maps against the executed reference                         #
# --------------------------------------------------------------------------- #
def test_boxes_c_recomputed_equals_golden(gold):
    z = gold
    H, W = z["im"].shape[:2]
    rows = []
    for t, (_, _, hf, ar) in enumerate(z["bbox_calls"].tolist()):
        rows.append(aspect_ref.decode_view(z["view_rois"][t], z["view_deltas"][t],
                                           z["view_im_scale"][t], H, W, ar or None, bool(hf),
                                           tuple(float(w) for w in z["weights"])))
    boxes_c = np.vstack(rows)
    assert boxes_c.dtype == np.float32 and np.array_equal(boxes_c, z["boxes_c"])
    assert np.array_equal(np.vstack(list(z["view_scores"])), z["scores_c"])
    # an aspect-ratio view's rows reach past the view's own width after the map back
    assert z["boxes_c"][2 * 200:4 * 200, 2::4].max() > aspect_ref.aspect_width(W, 0.75)


def test_head_boxes_recomputed_equal_golden(gold):
    z = gold
    W = z["im"].shape[1]
    boxes = z["det_plain_dets"][:, :4]
    calls = [[96.0, 133.0, 0.0, 0.0]] + z["mask_body_calls"][:, :4].tolist()
    for key, kcalls in (("mask_boxes", calls),
                        ("kps_boxes", [calls[0]] + z["kps_body_calls"][:, :4].tolist())):
        for t, (_, _, hf, ar) in enumerate(kcalls):
            got = aspect_ref.head_boxes(boxes, W, ar or None, bool(hf))
            assert got.dtype == np.float32 and np.array_equal(got, z[key][t]), (key, t)
    # the scales the heads' RoIs are taken at: get_target_scale of (H, War)
    from vosdetectron_amd import ops
    for (s, ms, _, ar), im_scale in zip(calls, z["mask_im_scale"].tolist()):
        Wv = aspect_ref.aspect_width(W, ar) if ar else W
        assert ops.target_scale(96, Wv, s, ms) == im_scale


def test_combined_masks_recomputed_equal_golden(gold):
    z = gold
    flips = [False] + [bool(r[2]) for r in z["mask_body_calls"].tolist()]
    ts = [m[..., ::-1] if hf else m for m, hf in zip(z["view_masks"], flips)]
    assert np.array_equal(np.mean(ts, axis=0), z["masks_c_SOFT_AVG"])
    assert np.array_equal(np.amax(ts, axis=0), z["masks_c_SOFT_MAX"])


# --------------------------------------------------------------------------- #
# C ABI                                                                        #
# --------------------------------------------------------------------------- #
def test_c_abi_argument_checks_without_a_device():
    from vosdetectron_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 768)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E = _lib.VD_ERR_ARG
    fn = L.vd_image_aspect_resize_to_blob
    assert fn(None, 1, 8, 8, 4, 0, p, 1.0, 8, 4, 32, 32, 0, p, None) == E  # no frames
    assert fn(p, 1, 8, 8, 4, 0, None, 1.0, 8, 4, 32, 32, 0, p, None) == E  # no lut
    assert fn(p, 1, 8, 8, 4, 0, p, 1.0, 8, 4, 32, 32, 0, None, None) == E  # no blob
    assert fn(p, 0, 8, 8, 4, 0, p, 1.0, 8, 4, 32, 32, 0, p, None) == E     # F < 1
    assert fn(p, 1, 8, 8, 0, 0, p, 1.0, 8, 4, 32, 32, 0, p, None) == E     # War < 1
    assert fn(p, 1, 8, 8, 4, 0, p, 0.0, 8, 4, 32, 32, 0, p, None) == E     # im_scale <= 0
    assert fn(p, 1, 8, 8, 4, 0, p, float("nan"), 8, 4, 32, 32, 0, p, None) == E
    assert fn(p, 1, 8, 8, 4, 0, p, 1.0, 8, 40, 32, 32, 0, p, None) == E    # Wr > Wp
    assert fn(p, 1, 8, 8, 4, 0, p, 1.0, 40, 4, 32, 32, 0, p, None) == E    # Hr > Hp
    assert fn(p, 1, 8, 8, 4, 0, p, 1.0, 8, 4, 65536, 32, 0, p, None) == E  # grid limit
    un = L.vd_box_union_add_view_ar
    w = (ctypes.c_float * 4)(10, 10, 5, 5)
    wp = ctypes.cast(w, ctypes.c_void_p)
    assert un(None, p, p, p, 8, 1, 5, p, p, 0, 1.0, 1, 0.05, wp, 64, p, 1 << 20, None) == E
    for bad in (0.0, -1.0, float("inf"), float("nan")):  # x_inv positive and finite
        assert un(p, p, p, p, 8, 1, 5, p, p, 0, bad, 1, 0.05, wp, 64, p, 1 << 20, None) == E
    # a short workspace is reported before anything is launched
    assert un(p, p, p, p, 8, 1, 5, p, p, 0, 0.5, 1, 0.05, wp, 64, p, 16, None) == \
        _lib.VD_ERR_WORKSPACE


def test_header_and_bindings_name_the_new_entries():
    from vosdetectron_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "vosdet.h")) as f:
        hdr = f.read()
    for name in ("vd_image_aspect_resize_to_blob", "vd_box_union_add_view_ar"):
        assert name in hdr and name in _lib.SIGNATURES
    assert "unpinned" in hdr[hdr.index("The blob of an aspect-ratio view"):
                             hdr.index("int vd_image_aspect_resize_to_blob")]
