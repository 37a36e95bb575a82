"""Test-time augmentation without a device: the config switch and its refusals,
config.aug_views' order, boxes.flip_boxes, and tests/aug_ref.py (the CPU reference the
GPU tests compare with) against tests/golden/tta.npz -- the reference's own
im_detect_bbox_aug / im_detect_mask_aug executed by tools/gen_tta_goldens.py."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import aug_ref
from vosdetectron_amd import config as vcfg

REF = "/root/reference"
X152 = "configs/baselines/e2e_mask_rcnn_X-152-32x8d-FPN-IN5k_1.44x.yaml"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta.npz")
AUG = {"ENABLED": True, "H_FLIP": True, "SCALES": (160, 288), "MAX_SIZE": 384,
       "SCALE_H_FLIP": True}


def _overrides(box=True, mask=True, **more):
    o = {"TEST.SCALE": 224, "TEST.MAX_SIZE": 288}
    for name, on in (("BBOX_AUG", box), ("MASK_AUG", mask)):
        if on:
            o.update({"TEST.%s.%s" % (name, k): v for k, v in AUG.items()})
    o.update(more)
    return o


def test_aug_views_order_and_count():
    cfg = vcfg.load_cfg(overrides=_overrides(), test_aug=True)
    box, mask = vcfg.aug_views(cfg)
    ident, hf = (224, 288, False), (224, 288, True)
    scales = [(160, 384, False), (160, 384, True), (288, 384, False), (288, 384, True)]
    assert box == [hf] + scales + [ident]  # np.vstack order: the identity view last
    assert mask == [ident, hf] + scales    # masks_ts order: the identity view first
    for aug in ("BBOX_AUG", "MASK_AUG"):   # the reference's own loops give the same lists
        assert aug_ref.views(224, 288, cfg.TEST[aug], aug == "BBOX_AUG") == \
            (box if aug == "BBOX_AUG" else mask)
    cfg = vcfg.load_cfg(overrides=_overrides(mask=False), test_aug=True)
    assert vcfg.aug_views(cfg) == ([hf] + scales + [ident], [ident])
    cfg = vcfg.load_cfg(overrides=_overrides(box=False), test_aug=True)
    assert vcfg.aug_views(cfg) == ([ident], [ident, hf] + scales)
    cfg = vcfg.load_cfg(overrides=_overrides(**{"TEST.BBOX_AUG.SCALE_H_FLIP": False,
                                               "TEST.BBOX_AUG.H_FLIP": False}), test_aug=True)
    assert vcfg.aug_views(cfg)[0] == [(160, 384, False), (288, 384, False), ident]
    assert vcfg.aug_views(vcfg.load_cfg()) == ([(600, 1000, False)], [(600, 1000, False)])


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent")
def test_x152_yaml_loads_with_test_aug():
    cfg = vcfg.load_cfg(os.path.join(REF, X152), test_aug=True)
    box, mask = vcfg.aug_views(cfg)
    assert len(box) == 18 and len(mask) == 18 and len(set(box)) == 18
    assert box[-1] == mask[0] == (800, 1333, False) and box[0] == mask[1] == (800, 1333, True)
    assert box[1] == (400, 2000, False) and box[-2] == (1200, 2000, True)
    assert cfg.TEST.MASK_AUG.HEUR == "SOFT_AVG" and cfg.TEST.BBOX_VOTE.ENABLED
    assert cfg.TEST.BBOX_VOTE.VOTE_TH == 0.9


def test_default_load_still_refuses():
    for key in vcfg.TEST_AUG_KEYS:
        with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")) as e:
            vcfg.load_cfg(overrides={key: True})
        assert "test_aug=True" in str(e.value) and "engine.AugFramePipeline" in str(e.value)
    with pytest.raises(NotImplementedError, match=r"TEST\.BBOX_AUG\.ENABLED"):
        vcfg.merge_cfg_from_list(["TEST.BBOX_AUG.ENABLED", "True"])
    assert not vcfg.cfg.TEST.BBOX_AUG.ENABLED


@pytest.mark.parametrize("key,val", [
    ("TEST.BBOX_AUG.ASPECT_RATIOS", (0.5,)), ("TEST.MASK_AUG.ASPECT_RATIOS", (2.0,)),
    ("TEST.BBOX_AUG.SCALE_SIZE_DEP", True), ("TEST.MASK_AUG.SCALE_SIZE_DEP", True),
    ("TEST.BBOX_AUG.SCORE_HEUR", "AVG"), ("TEST.BBOX_AUG.COORD_HEUR", "ID"),
    ("TEST.MASK_AUG.HEUR", "HARD_AVG"), ("TEST.KPS_AUG.ENABLED", True)])
def test_refusals_with_test_aug(key, val):
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        vcfg.load_cfg(overrides=_overrides(**{key: val}), test_aug=True)


def test_mask_heuristics_load():
    for heur in ("SOFT_AVG", "SOFT_MAX", "LOGIT_AVG"):
        cfg = vcfg.load_cfg(overrides=_overrides(**{"TEST.MASK_AUG.HEUR": heur}), test_aug=True)
        assert cfg.TEST.MASK_AUG.HEUR == heur
    # an AUG block that is not enabled is not judged
    vcfg.load_cfg(overrides={"TEST.BBOX_AUG.SCORE_HEUR": "AVG"}, test_aug=True)


def test_flip_boxes_is_the_reference_expression():
    from vosdetectron_amd import boxes as vboxes
    import torch
    rng = np.random.default_rng(3)
    b = rng.uniform(0, 900, (50, 8)).astype(np.float32)
    for w in (901, 1333):
        ref = b.copy()
        ref[:, 0::4] = w - b[:, 2::4] - 1
        ref[:, 2::4] = w - b[:, 0::4] - 1
        got = vboxes.flip_boxes(b, w)
        assert got.dtype == np.float32 and np.array_equal(got, ref)
        assert np.array_equal(got, aug_ref.flip_boxes(b, w))
        # the float32 expression the kernels evaluate: (W - x2) - 1
        x1 = (np.float32(w) - b[:, 2::4]) - np.float32(1)
        assert np.array_equal(got[:, 0::4], x1)
        assert np.array_equal(vboxes.flip_boxes(torch.from_numpy(b), w).numpy(), ref)
    assert np.array_equal(vboxes.flip_boxes(vboxes.flip_boxes(b[:, :4].round(), 901), 901),
                          b[:, :4].round())


# --------------------------------------------------------------------------- #
# aug_ref against the executed reference                                       #
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def test_golden_view_order(g):
    """The reference's call sequence is config.aug_views' order."""
    assert str(g["source"]) == "lib/core/test.py"
    cfg = vcfg.load_cfg(overrides={
        "TEST.SCALE": 96, "TEST.MAX_SIZE": 133,
        **{"TEST.%s.%s" % (a, k): v for a in ("BBOX_AUG", "MASK_AUG")
           for k, v in dict(AUG, SCALES=(64, 128), MAX_SIZE=192).items()}}, test_aug=True)
    box, mask = vcfg.aug_views(cfg)
    calls = [(int(s), int(m), bool(f)) for s, m, f in g["bbox_calls"]]
    assert calls == box
    # the identity mask view reuses the box pass's blob; the others run the body, in order
    assert [(int(s), int(m), bool(f)) for s, m, f in g["body_calls"]] == mask[1:]
    H, W = g["im"].shape[:2]
    for v, s in zip(box, g["view_im_scale"]):
        assert orc.target_scale(min(H, W), max(H, W), v[0], v[1]) == s
    for v, s in zip(mask, g["mask_im_scale"]):
        assert orc.target_scale(min(H, W), max(H, W), v[0], v[1]) == s


def test_aug_ref_union_and_detections_match_golden(g):
    shape = g["im"].shape
    Kc = g["view_scores"].shape[2]
    # im_scale is a Python float in the reference: the division stays in float32
    weights = tuple(float(w) for w in g["weights"])  # Python floats, as the reference's cfg
    boxes_ts = [aug_ref.decode_view(g["view_rois"][t], g["view_deltas"][t],
                                    float(g["view_im_scale"][t]), shape,
                                    bool(g["bbox_calls"][t][2]), weights)
                for t in range(len(g["bbox_calls"]))]
    sc, bx = aug_ref.union(list(g["view_scores"]), boxes_ts)
    assert sc.dtype == g["scores_c"].dtype and np.array_equal(sc, g["scores_c"])
    assert bx.dtype == g["boxes_c"].dtype and np.array_equal(bx, g["boxes_c"])
    thr, nms, per_im = g["test_cfg"]
    for name, kw in (("plain", {}), ("vote", dict(bbox_vote="AVG",
                                                  bbox_vote_th=float(g["vote_cfg"][0])))):
        s, b, cls_boxes = orc.box_results_with_nms_and_limit(sc, bx, Kc, thr, nms, int(per_im),
                                                             **kw)
        want = g["det_%s_dets" % name]
        assert np.array_equal(b, want[:, :4]) and np.array_equal(s, want[:, 4])
        assert np.array_equal(np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, Kc)]),
                              g["det_%s_cls" % name])


def test_aug_ref_mask_views_match_golden(g):
    """The boxes handed to each mask view and the three heuristics."""
    boxes = g["det_plain_dets"][:, :4]
    W = g["im"].shape[1]
    flips = [False] + [bool(f) for _, _, f in g["body_calls"]]
    for t, hf in enumerate(flips):
        want = aug_ref.flip_boxes(boxes, W) if hf else boxes
        assert np.array_equal(g["mask_boxes"][t], want), t
    vm = g["view_masks"]  # [T, M, K, R, R] as the network returns them
    T, M, Kc, Rm, _ = vm.shape
    masks_ts = [aug_ref.invert_masks(vm[t].reshape(M * Kc, Rm, Rm), flips[t]) for t in range(T)]
    for heur in ("SOFT_AVG", "SOFT_MAX"):
        got = aug_ref.combine_masks(masks_ts, heur).reshape(M, Kc, Rm, Rm)
        assert got.dtype == np.float32 and np.array_equal(got, g["masks_c_" + heur])
    got = aug_ref.combine_masks(masks_ts, "LOGIT_AVG").reshape(M, Kc, Rm, Rm)
    want = g["masks_c_LOGIT_AVG"]
    bound = 4 * aug_ref.logit_avg_float32_error(masks_ts)
    assert bound < 1e-6
    exact = (want == 0) | (want == 1) | ~np.isfinite(want)
    assert exact.any() and np.array_equal(got[exact], want[exact])
    assert np.abs(got[~exact] - want[~exact]).max() <= bound
