"""Keypoint test-time augmentation without a device: the config switch and its refusals,
config.kps_aug_views' order and tags, and tests/kps_aug_ref.py (the CPU reference the GPU
tests compare with) against tests/golden/kps_aug.npz -- the reference's own
im_detect_keypoints_aug and flip_heatmaps executed by tools/gen_kps_aug_goldens.py."""
import os

import numpy as np
import pytest

from tests import aug_ref, kps_aug_ref as kar
from vosdetectron_amd import config as vcfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kps_aug.npz")
KP = {"MODEL.KEYPOINTS_ON": True, "MODEL.MASK_ON": False, "FPN.FPN_ON": True,
      "KRCNN.ROI_KEYPOINTS_HEAD": vcfg.KEYPOINT_HEAD, "TEST.SCALE": 300, "TEST.MAX_SIZE": 451}
AUG = {"ENABLED": True, "H_FLIP": True, "SCALES": (200, 400), "MAX_SIZE": 700,
       "SCALE_H_FLIP": True}


def _overrides(kps=True, box=False, keypoints=True, **more):
    o = dict(KP) if keypoints else {"TEST.SCALE": 300, "TEST.MAX_SIZE": 451}
    for name, on in (("KPS_AUG", kps), ("BBOX_AUG", box)):
        if on:
            o.update({"TEST.%s.%s" % (name, k): v for k, v in AUG.items()})
    o.update(more)
    return o


def test_defaults_are_the_references():
    k = vcfg.default_cfg().TEST.KPS_AUG
    assert dict(k) == dict(ENABLED=False, HEUR="HM_AVG", H_FLIP=False, SCALES=(), MAX_SIZE=4000,
                           SCALE_H_FLIP=False, SCALE_SIZE_DEP=False, AREA_TH=32400,
                           ASPECT_RATIOS=(), ASPECT_RATIO_H_FLIP=False)


def test_acceptance():
    cfg = vcfg.load_cfg(overrides=_overrides(), test_aug=True)
    assert cfg.TEST.KPS_AUG.ENABLED and cfg.TEST.KPS_AUG.HEUR == "HM_AVG"
    for heur in ("HM_AVG", "HM_MAX"):
        for dep in (False, True):
            c = vcfg.load_cfg(overrides=_overrides(**{"TEST.KPS_AUG.HEUR": heur,
                                                      "TEST.KPS_AUG.SCALE_SIZE_DEP": dep}),
                              test_aug=True)
            assert (c.TEST.KPS_AUG.HEUR, c.TEST.KPS_AUG.SCALE_SIZE_DEP) == (heur, dep)
    # BBOX_AUG on a keypoint config, alone and with KPS_AUG
    vcfg.load_cfg(overrides=_overrides(kps=False, box=True), test_aug=True)
    vcfg.load_cfg(overrides=_overrides(box=True), test_aug=True)
    # a block that is not enabled is not judged
    vcfg.load_cfg(overrides=_overrides(kps=False, **{"TEST.KPS_AUG.HEUR": "X"}), test_aug=True)
    # a float32-exact threshold other than the default
    vcfg.load_cfg(overrides=_overrides(**{"TEST.KPS_AUG.SCALE_SIZE_DEP": True,
                                          "TEST.KPS_AUG.AREA_TH": 96.5 ** 2}), test_aug=True)
    # an inexact one is not judged while SCALE_SIZE_DEP is off
    vcfg.load_cfg(overrides=_overrides(**{"TEST.KPS_AUG.AREA_TH": 0.1}), test_aug=True)


def test_without_test_aug_the_key_is_refused_and_points_at_the_pipeline():
    for o in ({"TEST.KPS_AUG.ENABLED": True}, _overrides()):
        with pytest.raises(NotImplementedError, match=r"TEST\.KPS_AUG\.ENABLED") as e:
            vcfg.load_cfg(overrides=o)
        assert "test_aug=True" in str(e.value)
        assert "engine.KeypointAugFramePipeline" in str(e.value)
        assert "out of scope" not in str(e.value)
    assert vcfg.TEST_AUG_KEYS == ("TEST.BBOX_AUG.ENABLED", "TEST.MASK_AUG.ENABLED")


@pytest.mark.parametrize("key,o", [
    ("TEST.KPS_AUG.ENABLED", _overrides(keypoints=False)),
    ("TEST.KPS_AUG.ASPECT_RATIOS", _overrides(**{"TEST.KPS_AUG.ASPECT_RATIOS": (0.5,)})),
    ("TEST.KPS_AUG.HEUR", _overrides(**{"TEST.KPS_AUG.HEUR": "HM_MEDIAN"})),
    ("TEST.KPS_AUG.AREA_TH", _overrides(**{"TEST.KPS_AUG.SCALE_SIZE_DEP": True,
                                          "TEST.KPS_AUG.AREA_TH": 0.1})),
    ("TEST.KPS_AUG.AREA_TH", _overrides(**{"TEST.KPS_AUG.SCALE_SIZE_DEP": True,
                                          "TEST.KPS_AUG.AREA_TH": 2 ** 24 + 1})),
    ("TEST.KPS_AUG.AREA_TH", _overrides(**{"TEST.KPS_AUG.SCALE_SIZE_DEP": True,
                                          "TEST.KPS_AUG.AREA_TH": -1})),
    ("TEST.MASK_AUG.ENABLED", _overrides(**{"TEST.MASK_AUG.ENABLED": True})),
    ("TEST.BBOX_AUG.ASPECT_RATIOS", _overrides(box=True,
                                               **{"TEST.BBOX_AUG.ASPECT_RATIOS": (2.0,)})),
])
def test_refusals_with_test_aug(key, o):
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        vcfg.load_cfg(overrides=o, test_aug=True)


def test_kps_aug_views_order_and_tags():
    cfg = vcfg.load_cfg(overrides=_overrides(), test_aug=True)
    v, ds, us = vcfg.kps_aug_views(cfg)
    assert v == [(300, 451, False), (300, 451, True), (200, 700, False), (200, 700, True),
                 (400, 700, False), (400, 700, True)]
    assert ds == [False, False, True, True, False, False]
    assert us == [False, False, False, False, True, True]
    assert (v, ds, us) == kar.views(300, 451, cfg.TEST.KPS_AUG)
    # a scale equal to TEST.SCALE carries neither tag; no flips
    cfg = vcfg.load_cfg(overrides=_overrides(**{
        "TEST.KPS_AUG.SCALES": (300, 500), "TEST.KPS_AUG.H_FLIP": False,
        "TEST.KPS_AUG.SCALE_H_FLIP": False}), test_aug=True)
    assert vcfg.kps_aug_views(cfg) == ([(300, 451, False), (300, 700, False), (500, 700, False)],
                                       [False, False, False], [False, False, True])
    assert vcfg.kps_aug_views(cfg) == kar.views(300, 451, cfg.TEST.KPS_AUG)
    # off: the identity view alone, whatever the block holds; aug_views keeps its pair
    cfg = vcfg.load_cfg(overrides=_overrides(kps=False, **{"TEST.KPS_AUG.H_FLIP": True}),
                        test_aug=True)
    assert vcfg.kps_aug_views(cfg) == ([(300, 451, False)], [False], [False])
    assert vcfg.aug_views(cfg) == ([(300, 451, False)], [(300, 451, False)])


def test_flip_permutation_is_the_references_map():
    from vosdetectron_amd import keypoints
    names, flip = keypoints.get_keypoints()
    perm = keypoints.flip_permutation()
    assert perm == kar.COCO_FLIP_PERM and sorted(perm) == list(range(17)) and perm[0] == 0
    for l, r in flip.items():
        assert perm[names.index(l)] == names.index(r) and perm[names.index(r)] == names.index(l)


# --------------------------------------------------------------------------- #
# kps_aug_ref against the executed reference                                   #
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _golden_views(g, scales_key="aug_scales"):
    ts, tm, am = (int(x) for x in g["test_cfg"])
    aug = dict(H_FLIP=True, SCALE_H_FLIP=True, SCALES=tuple(int(s) for s in g[scales_key]),
               MAX_SIZE=am)
    return kar.views(ts, tm, aug)


def test_golden_contents(g):
    """The cases the fixture is there for: the area exactly at the threshold, the one
    just under, an odd frame width, and rows of 4 and of 6 views in one call."""
    assert str(g["source"]) in ("lib/core/test.py", "lib_vos/tools/vos_test.py")
    vh, boxes = g["view_heatmaps"], g["boxes"]
    assert vh.dtype == np.float32 and boxes.dtype == np.float32
    assert vh.shape == (8, 6, 17, 12, 12) and boxes.shape == (6, 4)
    assert int(g["im_hw"][1]) % 2 == 1 and float(g["area_th"]) == 180 ** 2
    area = kar.boxes_area(boxes)
    assert np.array_equal(area, g["areas"])
    assert area[0] == 32400 and 32300 < area[1] < 32400 and area[3] < 100 and area[5] > 1e5
    assert g["t_row"].tolist() == [4] * 6 and sorted(set(g["t_row_8"].tolist())) == [4, 6]
    size = os.path.getsize(GOLDEN)
    others = [os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f))
              for f in os.listdir(os.path.dirname(GOLDEN)) if f != "kps_aug.npz"]
    assert size <= max(others) and size <= 1 << 20


def test_golden_calls_are_the_views(g):
    """The reference's head calls get flip_boxes of the detections for flipped views, at
    each view's blob scale; its body calls are the non-identity views, in order."""
    v, ds, us = _golden_views(g)
    H, W = (int(x) for x in g["im_hw"])
    assert [(int(s), int(m), bool(f)) for s, m, f in g["body_calls"]] == v[1:]
    assert [(int(s), int(m), bool(f)) for s, m, f in g["body_calls_8"]] == \
        _golden_views(g, "aug_scales_8")[0][1:]
    from oracle import oracle as orc
    for t, view in enumerate(v):
        want = aug_ref.flip_boxes(g["boxes"], W) if view[2] else g["boxes"]
        assert g["head_boxes"][t].dtype == np.float32
        assert np.array_equal(g["head_boxes"][t], want), t
        assert g["head_scales"][t] == orc.target_scale(min(H, W), max(H, W), view[0], view[1])
    cfg = vcfg.load_cfg(overrides=_overrides(), test_aug=True)
    assert vcfg.kps_aug_views(cfg) == (v, ds, us)


@pytest.mark.parametrize("heur", ["HM_AVG", "HM_MAX"])
@pytest.mark.parametrize("dep", [False, True])
def test_restatement_equals_golden(g, heur, dep):
    v, ds, us = _golden_views(g)
    got, t_row = kar.combine(list(g["view_heatmaps"][:6]), [x[2] for x in v], heur, ds, us,
                             g["boxes"], float(g["area_th"]) if dep else None)
    want = g["combined_%s_%s" % (heur, "dep" if dep else "all")]
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want)
    assert t_row.tolist() == (g["t_row"].tolist() if dep else [6] * 6)
    if dep:  # the size dependence changed the result
        assert not np.array_equal(want, g["combined_%s_all" % heur])


@pytest.mark.parametrize("heur", ["HM_AVG", "HM_MAX"])
def test_restatement_equals_golden_mixed_divisors(g, heur):
    """Two scales below and one above TEST.SCALE: small boxes keep 4 views, large 6."""
    v, ds, us = _golden_views(g, "aug_scales_8")
    got, t_row = kar.combine(list(g["view_heatmaps"]), [x[2] for x in v], heur, ds, us,
                             g["boxes"], float(g["area_th"]))
    assert np.array_equal(got, g["combined_%s_dep8" % heur])
    assert t_row.tolist() == g["t_row_8"].tolist()


def test_flip_heatmaps_equals_golden(g):
    one = g["view_heatmaps"][0]
    got = kar.flip_heatmaps(one)
    assert got.dtype == np.float32 and np.array_equal(got, g["flipped_view0"])
    assert np.array_equal(kar.flip_heatmaps(got), one)
