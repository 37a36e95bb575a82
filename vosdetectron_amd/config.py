"""Configuration: the subset of the reference's global ``cfg`` (lib/core/config.py)
that the per-frame inference hot path reads, with the reference's defaults, and
a YAML merge that accepts the reference's own config files unchanged
(merge_cfg_from_file, config.py:1107-1113).  Unknown keys are ignored (the
training / dataset keys are out of scope), but a config that ENABLES an
inference option this path does not implement raises NotImplementedError
naming the keys (``UNSUPPORTED`` below) instead of silently running different
semantics.
"""
from __future__ import annotations

import ast
import copy
import math

import yaml


class AttrDict(dict):
    """lib/utils/collections.py AttrDict equivalent."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value


def _d(**kw):
    return AttrDict(kw)


def default_cfg() -> AttrDict:
    """Defaults from lib/core/config.py (line numbers cited per group)."""
    return _d(
        MODEL=_d(  # config.py:392-432
            TYPE="generalized_rcnn", CONV_BODY="FPN.fpn_ResNet50_conv5_body", NUM_CLASSES=81,
            CLS_AGNOSTIC_BBOX_REG=False, BBOX_REG_WEIGHTS=(10., 10., 5., 5.),
            FASTER_RCNN=True, MASK_ON=True, KEYPOINTS_ON=False, RPN_ONLY=False,
            # fork additions, config.py:404, 926-931
            ADD_UNKNOWN_CLASS=False, IDENTITY_TRAINING=False, IDENTITY_REPLACE_CLASS=True,
            TOTAL_INSTANCE_NUM=0, USE_DELTA_FLOW=False, LOAD_FLOW_FILE=False),
        RESNETS=_d(  # config.py:870-905
            NUM_GROUPS=1, WIDTH_PER_GROUP=64, STRIDE_1X1=True,
            TRANS_FUNC="bottleneck_transformation", STEM_FUNC="basic_bn_stem",
            SHORTCUT_FUNC="basic_bn_shortcut", RES5_DILATION=1, USE_GN=False),
        FPN=_d(  # config.py:680-726
            FPN_ON=False, DIM=256, COARSEST_STRIDE=32, MULTILEVEL_ROIS=False, MULTILEVEL_RPN=False,
            ROI_CANONICAL_SCALE=224, ROI_CANONICAL_LEVEL=4, ROI_MAX_LEVEL=5, ROI_MIN_LEVEL=2,
            RPN_MAX_LEVEL=6, RPN_MIN_LEVEL=2, RPN_ASPECT_RATIOS=(0.5, 1, 2),
            RPN_ANCHOR_START_SIZE=32, RPN_COLLECT_SCALE=1, EXTRA_CONV_LEVELS=False,
            USE_GN=False),
        FAST_RCNN=_d(  # config.py:620-645
            ROI_BOX_HEAD="fast_rcnn_heads.roi_2mlp_head", MLP_HEAD_DIM=1024,
            ROI_XFORM_METHOD="RoIPoolF", ROI_XFORM_SAMPLING_RATIO=0, ROI_XFORM_RESOLUTION=14,
            CONV_HEAD_DIM=256, NUM_STACKED_CONVS=4),
        MRCNN=_d(  # config.py:735-770
            ROI_MASK_HEAD="mask_rcnn_heads.mask_rcnn_fcn_head_v1up4convs", RESOLUTION=14,
            ROI_XFORM_METHOD="RoIAlign", ROI_XFORM_RESOLUTION=7, ROI_XFORM_SAMPLING_RATIO=0,
            DIM_REDUCED=256, DILATION=2, UPSAMPLE_RATIO=1, USE_FC_OUTPUT=False,
            CLS_SPECIFIC_MASK=True, CONV_INIT="GaussianFill", THRESH_BINARIZE=0.5),
        KRCNN=_d(  # config.py:783-855
            ROI_KEYPOINTS_HEAD="", HEATMAP_SIZE=-1, UP_SCALE=-1, USE_DECONV=False,
            DECONV_DIM=256, USE_DECONV_OUTPUT=False, DILATION=1, DECONV_KERNEL=4,
            NUM_KEYPOINTS=-1, NUM_STACKED_CONVS=8, CONV_HEAD_DIM=256, CONV_HEAD_KERNEL=3,
            CONV_INIT="GaussianFill", NMS_OKS=False, KEYPOINT_CONFIDENCE="bbox",
            ROI_XFORM_METHOD="RoIAlign", ROI_XFORM_RESOLUTION=7, ROI_XFORM_SAMPLING_RATIO=0,
            INFERENCE_MIN_SIZE=0),
        GROUP_NORM=_d(DIM_PER_GP=-1, NUM_GROUPS=32, EPSILON=1e-5),  # config.py:983-989
        CONVGRU=_d(  # config.py:908-921
            HIDDEN_STATE_CHANNELS=(256, 256, 256, 256, 256), KERNEL_SIZE=3, STRIDE=1,
            DILATION=1, GROUPS=1, USE_GN=True, GN_GROUPS=32, DYNAMIC_MODEL=True),
        RPN=_d(CLS_ACTIVATION="sigmoid", SIZES=(64, 128, 256, 512), STRIDE=16,
               ASPECT_RATIOS=(0.5, 1, 2)),  # config.py:655-675
        TEST=_d(  # config.py:180-230, 945-950
            SCALE=600, MAX_SIZE=1000, NMS=0.3, BBOX_REG=True, RPN_NMS_THRESH=0.7,
            RPN_PRE_NMS_TOP_N=12000, RPN_POST_NMS_TOP_N=2000, RPN_MIN_SIZE=0,
            DETECTIONS_PER_IM=100, SCORE_THRESH=0.05, NUM_DET_PER_CLASS_PRE=0,
            NUM_DET_PER_CLASS_POST=0, NMS_CROSS_CLASS=0.,
            # config.py:356-383: soft-NMS and box voting (vd_box_detections_ex)
            SOFT_NMS=_d(ENABLED=False, METHOD="linear", SIGMA=0.5),
            BBOX_VOTE=_d(ENABLED=False, VOTE_TH=0.8, SCORING_METHOD="ID",
                         SCORING_METHOD_BETA=1.0),
            # config.py:246-316: test-time augmentation, accepted by load_cfg(test_aug=True)
            # only (engine.AugFramePipeline); aug_views() lists the views
            BBOX_AUG=_d(ENABLED=False, SCORE_HEUR="UNION", COORD_HEUR="UNION", H_FLIP=False,
                        SCALES=(), MAX_SIZE=4000, SCALE_H_FLIP=False, SCALE_SIZE_DEP=False,
                        ASPECT_RATIOS=(), ASPECT_RATIO_H_FLIP=False),
            MASK_AUG=_d(ENABLED=False, HEUR="SOFT_AVG", H_FLIP=False, SCALES=(), MAX_SIZE=4000,
                        SCALE_H_FLIP=False, SCALE_SIZE_DEP=False, ASPECT_RATIOS=(),
                        ASPECT_RATIO_H_FLIP=False),
            # config.py:322-351: keypoint test-time augmentation, accepted by
            # load_cfg(test_aug=True) on a MODEL.KEYPOINTS_ON config only
            # (engine.KeypointAugFramePipeline); kps_aug_views() lists the views
            KPS_AUG=_d(ENABLED=False, HEUR="HM_AVG", H_FLIP=False, SCALES=(), MAX_SIZE=4000,
                       SCALE_H_FLIP=False, SCALE_SIZE_DEP=False, AREA_TH=180 ** 2,
                       ASPECT_RATIOS=(), ASPECT_RATIO_H_FLIP=False),
            # (NMS_WITH_MASK_IOU / NMS_SMALL_BOX_IOU below are built: VOSPipeline)
            NMS_WITH_MASK_IOU=0., NMS_SMALL_BOX_IOU=0.,  # config.py:951-953: the VOS
            NMS_SMALL_BOX_SCORE_THRESHOLD=0.),  # loop's heuristics (engine.VOSPipeline)
        # config.py:86-96: read at inference by im_detect_bbox (lib/core/test.py:174-177);
        # refused when on (UNSUPPORTED), the other TRAIN keys stay out of scope
        TRAIN=_d(BBOX_NORMALIZE_TARGETS_PRECOMPUTED=False),
        # config.py:1004: the hash quantum of im_detect_bbox on caller-given boxes
        # (MODEL.FASTER_RCNN False, lib/core/test.py:132-139); 0 switches the de-dup off
        DEDUP_BOXES=1 / 16.,
        PIXEL_MEANS=(102.9801, 115.9465, 122.7717),  # config.py:1015
        BBOX_XFORM_CLIP=math.log(1000. / 16.),  # config.py:1009
        CROP_RESIZE_WITH_MAX_POOL=True,  # config.py:1058
    )


def _decode(v):
    """config.py _decode_cfg_value: strings that are Python literals (e.g. the
    YAML text "(32, 64, 128, 256, 512)") become values."""
    if isinstance(v, str):
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v
    return v


def _merge(a, b):
    for k, v in a.items():
        if k not in b:
            continue  # training / dataset keys: out of scope for the hot path
        if isinstance(v, dict) and isinstance(b[k], dict):
            _merge(v, b[k])
        else:
            v = _decode(v)
            if isinstance(b[k], tuple) and isinstance(v, (list, tuple)):
                v = tuple(v)
            b[k] = v


def _merge_yaml(y, cfg):
    """_merge of a reference YAML.  MODEL.MASK_ON defaults to True here (the mask
    family) and to False in the reference (config.py:432), which its keypoint YAMLs
    rely on: a YAML that switches KEYPOINTS_ON on and does not mention MASK_ON gets
    the reference's default."""
    _merge(y, cfg)
    m = y.get("MODEL") or {}
    if _decode(m.get("KEYPOINTS_ON", False)) is True and "MASK_ON" not in m:
        cfg["MODEL"]["MASK_ON"] = False


KEYPOINT_HEAD = "keypoint_rcnn_heads.roi_pose_head_v1convX"


class _WithCfg:
    """An UNSUPPORTED predicate that also reads other keys: called as fn(value, cfg)."""

    def __init__(self, fn):
        self.fn = fn


# Inference options of the reference that change detections and are not built
# here: (dotted key, "enabled" predicate, where the reference implements it).
UNSUPPORTED = (
    # the reference's call sites never pass SCORING_METHOD_BETA (test.py:770-775),
    # so GENERALIZED_AVG always runs at beta 1 = AVG; only TEMP_AVG is missing
    ("TEST.BBOX_VOTE", lambda v: bool(v.get("ENABLED")) and v.get("SCORING_METHOD") not in (
        "ID", "AVG", "IOU_AVG", "QUASI_SUM", "GENERALIZED_AVG"),
     "box-voting scoring TEMP_AVG (numpy float32 log / exp), lib/utils/boxes.py:300-320"),
    ("TEST.SOFT_NMS", lambda v: bool(v.get("ENABLED")) and v.get("METHOD") not in (
        "hard", "linear", "gaussian"), "soft-NMS method (boxes.py:344 asserts)"),
    ("TEST.BBOX_AUG.ENABLED", bool, "box test-time augmentation, lib/core/test.py:193-363, as "
     "a config key: load_cfg(..., test_aug=True) accepts it for engine.AugFramePipeline"),
    ("TEST.MASK_AUG.ENABLED", bool, "mask test-time augmentation, lib/core/test.py:405-526, as "
     "a config key: load_cfg(..., test_aug=True) accepts it for engine.AugFramePipeline"),
    ("TEST.KPS_AUG.ENABLED", bool, "keypoint test-time augmentation, lib/core/test.py:567-730, "
     "as a config key: load_cfg(..., test_aug=True) accepts it on a MODEL.KEYPOINTS_ON config "
     "for engine.KeypointAugFramePipeline"),
    ("TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED", bool,
     "legacy de-normalisation of the box deltas by precomputed means and stds, "
     "lib/core/test.py:174-177"),
    ("MODEL.USE_DELTA_FLOW", _WithCfg(lambda v, c: bool(v) and not c.get("VOS", False)),
     "delta-flow head on a model other than Generalized_VOS_RCNN: only the VOS builder has it, "
     "lib_vos/vos_modeling/vos_model_builder.py:95-104"),
    # Keypoint R-CNN is built for the FPN family with the v1convX head and the
    # plain per-box decode (engine.KeypointFramePipeline)
    ("KRCNN.NMS_OKS", bool, "OKS NMS of keypoint_results, lib/core/test.py:864-870, as a config "
     "key: the device kernel is switched on by engine.KeypointFramePipeline(nms_oks=True), or "
     "called as keypoints.nms_oks"),
    ("KRCNN.ROI_KEYPOINTS_HEAD", _WithCfg(lambda v, c: bool(c.MODEL.KEYPOINTS_ON) and v != KEYPOINT_HEAD),
     "keypoint head other than %s" % KEYPOINT_HEAD),
    ("MODEL.KEYPOINTS_ON", _WithCfg(lambda v, c: bool(v) and bool(c.MODEL.MASK_ON)),
     "MODEL.KEYPOINTS_ON together with MODEL.MASK_ON (one RoI head family per model)"),
    ("MODEL.KEYPOINTS_ON", _WithCfg(lambda v, c: bool(v) and (not c.FPN.FPN_ON
                                                              or bool(c.get("VOS", False)))),
     "MODEL.KEYPOINTS_ON with a C4 (FPN.FPN_ON False) or VOS model"),
)


def _get(cfg, key):
    for p in key.split("."):
        cfg = cfg[p]
    return cfg


TEST_AUG_KEYS = ("TEST.BBOX_AUG.ENABLED", "TEST.MASK_AUG.ENABLED")
KPS_AUG_KEY = "TEST.KPS_AUG.ENABLED"  # test_aug accepts it too, on keypoint configs
MASK_AUG_HEURS = ("SOFT_AVG", "SOFT_MAX", "LOGIT_AVG")
KPS_AUG_HEURS = ("HM_AVG", "HM_MAX")


def _aug_on(aug):
    return lambda v, c: bool(c.TEST[aug].ENABLED) and bool(v)


def _aug_not(aug, allowed):
    return lambda v, c: bool(c.TEST[aug].ENABLED) and v not in allowed


def _float32_exact(v):
    """v is a non-negative number that float32 holds exactly (the size-dependent
    combination compares float32 box areas with it on the device)."""
    import struct
    try:
        f = float(v)
        return f >= 0 and f == v and struct.unpack("f", struct.pack("f", f))[0] == f
    except (TypeError, ValueError, OverflowError):
        return False


# What load_cfg(test_aug=True) still refuses of an enabled TEST.BBOX_AUG / MASK_AUG /
# KPS_AUG.
UNSUPPORTED_TEST_AUG = tuple(
    (key, _WithCfg(pred), where) for key, pred, where in (
        ("TEST.BBOX_AUG.ASPECT_RATIOS", _aug_on("BBOX_AUG"),
         "aspect-ratio views need an anisotropic resize, lib/core/test.py:330-363; "
         "load_cfg(..., test_aug=True, aspect_views=True) accepts them"),
        ("TEST.MASK_AUG.ASPECT_RATIOS", _aug_on("MASK_AUG"),
         "aspect-ratio views need an anisotropic resize, lib/core/test.py:509-526; "
         "load_cfg(..., test_aug=True, aspect_views=True) accepts them"),
        ("TEST.BBOX_AUG.SCALE_SIZE_DEP", _aug_on("BBOX_AUG"),
         "the reference asserts it off, lib/core/test.py:197"),
        ("TEST.MASK_AUG.SCALE_SIZE_DEP", _aug_on("MASK_AUG"),
         "the reference asserts it off, lib/core/test.py:418"),
        ("TEST.BBOX_AUG.SCORE_HEUR", _aug_not("BBOX_AUG", ("UNION",)),
         "the reference asserts UNION for Faster R-CNN models, lib/core/test.py:205-207"),
        ("TEST.BBOX_AUG.COORD_HEUR", _aug_not("BBOX_AUG", ("UNION",)),
         "UNION whenever the score heuristic is, lib/core/test.py:199-201"),
        ("TEST.MASK_AUG.HEUR", _aug_not("MASK_AUG", MASK_AUG_HEURS),
         "the reference raises, lib/core/test.py:471-474"),
        ("TEST.KPS_AUG.ENABLED", lambda v, c: bool(v) and not c.MODEL.KEYPOINTS_ON,
         "keypoint test-time augmentation needs a MODEL.KEYPOINTS_ON config"),
        ("TEST.MASK_AUG.ENABLED", lambda v, c: bool(v) and bool(c.MODEL.KEYPOINTS_ON),
         "a MODEL.KEYPOINTS_ON model has no mask head"),
        ("TEST.KPS_AUG.ASPECT_RATIOS", _aug_on("KPS_AUG"),
         "aspect-ratio views need an anisotropic resize, lib/core/test.py:684-702; "
         "load_cfg(..., test_aug=True, aspect_views=True) accepts them"),
        ("TEST.KPS_AUG.HEUR", _aug_not("KPS_AUG", KPS_AUG_HEURS),
         "the reference raises, lib/core/test.py:631-638"),
        ("TEST.KPS_AUG.AREA_TH", lambda v, c: bool(c.TEST.KPS_AUG.ENABLED) and bool(
            c.TEST.KPS_AUG.SCALE_SIZE_DEP) and not _float32_exact(v),
         "with SCALE_SIZE_DEP the threshold must be a non-negative number that float32 holds "
         "exactly: the float32 box areas are compared with it on the device"),
    ))


# The keys of UNSUPPORTED_TEST_AUG that aspect_views=True accepts (the views run on the
# augmented pipelines through vd_image_aspect_resize_to_blob).
ASPECT_VIEW_KEYS = ("TEST.BBOX_AUG.ASPECT_RATIOS", "TEST.MASK_AUG.ASPECT_RATIOS",
                    "TEST.KPS_AUG.ASPECT_RATIOS")


def aspect_width(im_w: int, ar: float) -> int:
    """aspect_ratio_rel's width (lib/utils/image.py:30): int(round(ar * im_w))."""
    return int(round(float(ar) * im_w))


def check_aspect_ratios(cfg, im_w=None) -> None:
    """Raise ValueError for an enabled ASPECT_RATIOS entry that is not a positive finite
    number or, given the frame width im_w, whose view would be under 2 columns wide."""
    bad = []
    for key in ASPECT_VIEW_KEYS:
        aug = cfg.TEST[key.split(".")[1]]
        if not aug.ENABLED:
            continue
        for ar in aug.ASPECT_RATIOS:
            try:
                f = float(ar)
            except (TypeError, ValueError):
                f = float("nan")
            if isinstance(ar, bool) or not (f > 0.0 and math.isfinite(f)):
                bad.append("%s holds %r: a ratio is a positive finite number" % (key, ar))
            elif im_w is not None and aspect_width(im_w, f) < 2:
                bad.append("%s holds %r: at frame width %d the view is %d column(s) wide, "
                           "under 2" % (key, ar, im_w, aspect_width(im_w, f)))
    if bad:
        raise ValueError("aspect-ratio views: " + "; ".join(bad))


def check_supported(cfg, test_aug: bool = False, aspect_views: bool = False) -> None:
    """Raise NotImplementedError naming every enabled option of ``UNSUPPORTED``;
    test_aug accepts TEST.BBOX_AUG / TEST.MASK_AUG / TEST.KPS_AUG but for
    ``UNSUPPORTED_TEST_AUG``; aspect_views (with test_aug) also accepts the three
    ``ASPECT_VIEW_KEYS`` and checks their ratios (check_aspect_ratios: ValueError)."""
    bad = []
    table = UNSUPPORTED
    if test_aug:
        table = tuple(r for r in UNSUPPORTED if r[0] not in TEST_AUG_KEYS + (KPS_AUG_KEY,)) \
            + tuple(r for r in UNSUPPORTED_TEST_AUG
                    if not (aspect_views and r[0] in ASPECT_VIEW_KEYS))
    for key, enabled, where in table:
        try:
            v = _get(cfg, key)
        except (KeyError, TypeError):
            continue
        if enabled.fn(v, cfg) if isinstance(enabled, _WithCfg) else enabled(v):
            bad.append("%s=%r (%s)" % (key, v, where))
    if bad:
        raise NotImplementedError("inference options not implemented by vosdetectron_amd: "
                                  + "; ".join(bad))
    if test_aug and aspect_views:
        check_aspect_ratios(cfg)


def aug_views(cfg):
    """The views of im_detect_bbox_aug / im_detect_mask_aug as two ordered lists of
    (scale, max_size, hflip).  Box views in np.vstack order (lib/core/test.py:218-261):
    the flipped view at (TEST.SCALE, TEST.MAX_SIZE), each BBOX_AUG.SCALES entry (then
    its flip with SCALE_H_FLIP), each ASPECT_RATIOS entry (then its flip with
    ASPECT_RATIO_H_FLIP), the identity view LAST.  Mask views in masks_ts order
    (test.py:425-456): the identity view FIRST, the flipped view, the scales, the aspect
    ratios.  An aspect-ratio view is the 4-tuple (TEST.SCALE, TEST.MAX_SIZE, hflip, ar);
    every other view stays a 3-tuple.  With an AUG key off its list is the identity
    view alone."""
    tst = cfg.TEST
    ident = (tst.SCALE, tst.MAX_SIZE, False)

    def extra(aug):
        v = []
        if aug.H_FLIP:
            v.append((tst.SCALE, tst.MAX_SIZE, True))
        for s in aug.SCALES:
            v.append((s, aug.MAX_SIZE, False))
            if aug.SCALE_H_FLIP:
                v.append((s, aug.MAX_SIZE, True))
        for ar in aug.ASPECT_RATIOS:
            v.append((tst.SCALE, tst.MAX_SIZE, False, ar))
            if aug.ASPECT_RATIO_H_FLIP:
                v.append((tst.SCALE, tst.MAX_SIZE, True, ar))
        return v

    box = (extra(tst.BBOX_AUG) if tst.BBOX_AUG.ENABLED else []) + [ident]
    mask = [ident] + (extra(tst.MASK_AUG) if tst.MASK_AUG.ENABLED else [])
    return box, mask


def kps_aug_views(cfg):
    """The views of im_detect_keypoints_aug in heatmaps_ts order (lib/core/test.py:
    591-615) -> (views, ds_tags, us_tags): views as aug_views' (scale, max_size, hflip),
    the identity view FIRST, the flipped view at (TEST.SCALE, TEST.MAX_SIZE), then per
    KPS_AUG.SCALES entry the view at (scale, KPS_AUG.MAX_SIZE) and its flip with
    SCALE_H_FLIP.  A scale view is tagged ds when scale < TEST.SCALE and us when
    scale > TEST.SCALE (combine_heatmaps_size_dep drops ds views for small boxes and us
    views for large ones); the identity and plain-flip views carry neither.  Then per
    KPS_AUG.ASPECT_RATIOS entry (test.py:618-628) the 4-tuple (TEST.SCALE, TEST.MAX_SIZE,
    hflip, ar) and its flip with ASPECT_RATIO_H_FLIP, with neither tag.  With KPS_AUG
    off: the identity view alone."""
    tst = cfg.TEST
    aug = tst.KPS_AUG
    views, ds, us = [(tst.SCALE, tst.MAX_SIZE, False)], [False], [False]
    if not aug.ENABLED:
        return views, ds, us
    if aug.H_FLIP:
        views.append((tst.SCALE, tst.MAX_SIZE, True))
        ds.append(False)
        us.append(False)
    for s in aug.SCALES:
        for hf in (False, True) if aug.SCALE_H_FLIP else (False,):
            views.append((s, aug.MAX_SIZE, hf))
            ds.append(s < tst.SCALE)
            us.append(s > tst.SCALE)
    for ar in aug.ASPECT_RATIOS:
        for hf in (False, True) if aug.ASPECT_RATIO_H_FLIP else (False,):
            views.append((tst.SCALE, tst.MAX_SIZE, hf, ar))
            ds.append(False)
            us.append(False)
    return views, ds, us


def load_cfg(path: str | None = None, overrides: dict | None = None,
             test_aug: bool = False, aspect_views: bool = False) -> AttrDict:
    """Defaults, then a reference YAML (safe loader), then dotted overrides.
    Raises NotImplementedError if the result enables an ``UNSUPPORTED`` option.
    test_aug=True accepts TEST.BBOX_AUG.ENABLED / TEST.MASK_AUG.ENABLED (the config
    runs on engine.AugFramePipeline only) and, on a MODEL.KEYPOINTS_ON config,
    TEST.BBOX_AUG.ENABLED / TEST.KPS_AUG.ENABLED (engine.KeypointAugFramePipeline
    only); it refuses ``UNSUPPORTED_TEST_AUG``.  aspect_views=True (with test_aug) drops
    the refusal of the three ASPECT_RATIOS keys (``ASPECT_VIEW_KEYS``) and of nothing
    else; a non-positive or non-finite ratio raises ValueError."""
    cfg = default_cfg()
    if path:
        with open(path) as f:
            _merge_yaml(yaml.safe_load(f) or {}, cfg)
    for key, val in (overrides or {}).items():
        d = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            d = d[p]
        d[parts[-1]] = val
    check_supported(cfg, test_aug, aspect_views)
    return cfg


# The configurations BASELINE.json names, restated as overrides of the defaults
# (values from configs/baselines/*.yaml of the reference).
def e2e_mask_rcnn_R_50_FPN_1x() -> AttrDict:
    return load_cfg(overrides={
        "FPN.FPN_ON": True, "FPN.MULTILEVEL_ROIS": True, "FPN.MULTILEVEL_RPN": True,
        "MODEL.CONV_BODY": "FPN.fpn_ResNet50_conv5_body", "MODEL.FASTER_RCNN": True,
        "MODEL.MASK_ON": True, "FAST_RCNN.ROI_BOX_HEAD": "fast_rcnn_heads.roi_2mlp_head",
        "FAST_RCNN.ROI_XFORM_METHOD": "RoIAlign", "FAST_RCNN.ROI_XFORM_RESOLUTION": 7,
        "FAST_RCNN.ROI_XFORM_SAMPLING_RATIO": 2,
        "MRCNN.ROI_MASK_HEAD": "mask_rcnn_heads.mask_rcnn_fcn_head_v1up4convs",
        "MRCNN.RESOLUTION": 28, "MRCNN.ROI_XFORM_METHOD": "RoIAlign",
        "MRCNN.ROI_XFORM_RESOLUTION": 14, "MRCNN.ROI_XFORM_SAMPLING_RATIO": 2,
        "MRCNN.DILATION": 1, "MRCNN.CONV_INIT": "MSRAFill", "TEST.SCALE": 800,
        "TEST.MAX_SIZE": 1333, "TEST.NMS": 0.5, "TEST.RPN_PRE_NMS_TOP_N": 1000,
        "TEST.RPN_POST_NMS_TOP_N": 1000})


def e2e_mask_rcnn_R_50_C4_1x() -> AttrDict:
    """configs/baselines/e2e_mask_rcnn_R-50-C4_1x.yaml (BASELINE.json configs[0]):
    no FPN (FPN_ON default False, config.py:682), ResNet50_conv4_body,
    ResNet_roi_conv5_head, mask_rcnn_fcn_head_v0upshare (-> MODEL.SHARE_RES5,
    config.py:1072-1095), RoIAlign 14x14 with the adaptive sampling ratio
    (ROI_XFORM_SAMPLING_RATIO default 0), RPN pre/post 6000/1000."""
    return load_cfg(overrides={
        "MODEL.CONV_BODY": "ResNet.ResNet50_conv4_body", "MODEL.FASTER_RCNN": True,
        "MODEL.MASK_ON": True, "RPN.SIZES": (32, 64, 128, 256, 512),
        "FAST_RCNN.ROI_BOX_HEAD": "ResNet.ResNet_roi_conv5_head",
        "FAST_RCNN.ROI_XFORM_METHOD": "RoIAlign", "FAST_RCNN.ROI_XFORM_RESOLUTION": 14,
        "FAST_RCNN.ROI_XFORM_SAMPLING_RATIO": 0,
        "MRCNN.ROI_MASK_HEAD": "mask_rcnn_heads.mask_rcnn_fcn_head_v0upshare",
        "MRCNN.RESOLUTION": 14, "MRCNN.ROI_XFORM_METHOD": "RoIAlign",
        "MRCNN.ROI_XFORM_RESOLUTION": 14, "MRCNN.ROI_XFORM_SAMPLING_RATIO": 0,
        "MRCNN.DILATION": 1, "MRCNN.CONV_INIT": "MSRAFill", "TEST.SCALE": 800,
        "TEST.MAX_SIZE": 1333, "TEST.NMS": 0.5, "TEST.RPN_PRE_NMS_TOP_N": 6000,
        "TEST.RPN_POST_NMS_TOP_N": 1000})


def e2e_mask_rcnn_R_101_FPN_2x() -> AttrDict:
    cfg = e2e_mask_rcnn_R_50_FPN_1x()
    cfg.MODEL.CONV_BODY = "FPN.fpn_ResNet101_conv5_body"
    return cfg


def e2e_mask_rcnn_X_101_32x8d_FPN_1x() -> AttrDict:
    cfg = e2e_mask_rcnn_R_50_FPN_1x()
    cfg.MODEL.CONV_BODY = "FPN.fpn_ResNet101_conv5_body"
    cfg.RESNETS.NUM_GROUPS = 32
    cfg.RESNETS.WIDTH_PER_GROUP = 8
    return cfg


def e2e_keypoint_rcnn_R_50_FPN_1x() -> AttrDict:
    """configs/baselines/e2e_keypoint_rcnn_R-50-FPN_1x.yaml: the R-50-FPN body, RPN
    and box head of the mask config, MASK_ON off (the reference's default), the
    v1convX pose head (8 x 512-channel 3x3 convs on 14x14 RoIAlign) and the deconv
    output + 2x bilinear upsample to 56x56 heatmaps of 17 keypoints."""
    return load_cfg(overrides={
        "FPN.FPN_ON": True, "FPN.MULTILEVEL_ROIS": True, "FPN.MULTILEVEL_RPN": True,
        "MODEL.CONV_BODY": "FPN.fpn_ResNet50_conv5_body", "MODEL.FASTER_RCNN": True,
        "MODEL.MASK_ON": False, "MODEL.KEYPOINTS_ON": True,
        "FAST_RCNN.ROI_BOX_HEAD": "fast_rcnn_heads.roi_2mlp_head",
        "FAST_RCNN.ROI_XFORM_METHOD": "RoIAlign", "FAST_RCNN.ROI_XFORM_RESOLUTION": 7,
        "FAST_RCNN.ROI_XFORM_SAMPLING_RATIO": 2,
        "KRCNN.ROI_KEYPOINTS_HEAD": KEYPOINT_HEAD, "KRCNN.NUM_STACKED_CONVS": 8,
        "KRCNN.NUM_KEYPOINTS": 17, "KRCNN.USE_DECONV_OUTPUT": True,
        "KRCNN.CONV_INIT": "MSRAFill", "KRCNN.CONV_HEAD_DIM": 512, "KRCNN.UP_SCALE": 2,
        "KRCNN.HEATMAP_SIZE": 56, "KRCNN.ROI_XFORM_METHOD": "RoIAlign",
        "KRCNN.ROI_XFORM_RESOLUTION": 14, "KRCNN.ROI_XFORM_SAMPLING_RATIO": 2,
        "KRCNN.KEYPOINT_CONFIDENCE": "bbox", "TEST.SCALE": 800, "TEST.MAX_SIZE": 1333,
        "TEST.NMS": 0.5, "TEST.RPN_PRE_NMS_TOP_N": 1000, "TEST.RPN_POST_NMS_TOP_N": 1000})


def vos_R_101_FPN_3x_gn_static_davis() -> AttrDict:
    """lib_vos/tools/R-101-FPN_3x_gn_static_davis.yaml, with the inference-time
    rewrite of lib_vos/tools/infer_davis_sequential.py:104-113 (IDENTITY_TRAINING
    and IDENTITY_REPLACE_CLASS -> NUM_CLASSES = 145, no identity head)."""
    cfg = load_cfg(overrides={
        "MODEL.CONV_BODY": "FPN.fpn_ResNet101_conv5_body", "MODEL.FASTER_RCNN": True,
        "MODEL.MASK_ON": True, "MODEL.CLS_AGNOSTIC_BBOX_REG": True,
        "MODEL.NUM_CLASSES": 145, "MODEL.IDENTITY_TRAINING": False,
        "FPN.FPN_ON": True, "FPN.MULTILEVEL_ROIS": True, "FPN.MULTILEVEL_RPN": True,
        "FPN.USE_GN": True, "FPN.COARSEST_STRIDE": 64, "FPN.RPN_ANCHOR_START_SIZE": 32,
        "FPN.ROI_CANONICAL_SCALE": 224,
        "RESNETS.STRIDE_1X1": False, "RESNETS.TRANS_FUNC": "bottleneck_gn_transformation",
        "RESNETS.STEM_FUNC": "basic_gn_stem", "RESNETS.SHORTCUT_FUNC": "basic_gn_shortcut",
        "RESNETS.USE_GN": True,
        "FAST_RCNN.ROI_BOX_HEAD": "fast_rcnn_heads.roi_Xconv1fc_gn_head",
        "FAST_RCNN.ROI_XFORM_METHOD": "RoIAlign", "FAST_RCNN.ROI_XFORM_RESOLUTION": 7,
        "FAST_RCNN.ROI_XFORM_SAMPLING_RATIO": 2,
        "MRCNN.ROI_MASK_HEAD": "mask_rcnn_heads.mask_rcnn_fcn_head_v1up4convs_gn",
        "MRCNN.RESOLUTION": 56, "MRCNN.ROI_XFORM_METHOD": "RoIAlign",
        "MRCNN.ROI_XFORM_RESOLUTION": 28, "MRCNN.ROI_XFORM_SAMPLING_RATIO": 2,
        "MRCNN.DILATION": 2, "MRCNN.CONV_INIT": "MSRAFill", "MRCNN.CLS_SPECIFIC_MASK": False,
        "CONVGRU.DYNAMIC_MODEL": False, "RPN.ASPECT_RATIOS": (0.2, 0.5, 1, 2, 5),
        "TEST.SCALE": 480, "TEST.MAX_SIZE": 1333, "TEST.NMS": 0.5,
        "TEST.RPN_PRE_NMS_TOP_N": 1000, "TEST.RPN_POST_NMS_TOP_N": 1000})
    cfg.VOS = True  # build Generalized_VOS_RCNN (vos_model_builder.py:70)
    return cfg


def vos_R_101_FPN_3x_gn_dynamic_davis() -> AttrDict:
    """lib_vos/tools/R-101-FPN_3x_gn_dynamic_simple_davis.yaml (ConvGRU hidden
    states carried across the frames of a sequence), same inference rewrite."""
    cfg = vos_R_101_FPN_3x_gn_static_davis()
    cfg.CONVGRU.DYNAMIC_MODEL = True
    cfg.TEST.MAX_SIZE = 1200
    return cfg


def vos_R_101_FPN_3x_gn_dynamic_delta_flow_davis() -> AttrDict:
    """The dynamic config with MODEL.USE_DELTA_FLOW: the model makes its own flow
    from the change of its per-level flow features (vos_model_builder.py:95-104,
    314-326), no .flo files."""
    cfg = vos_R_101_FPN_3x_gn_dynamic_davis()
    cfg.MODEL.USE_DELTA_FLOW = True  # after cfg.VOS = True: rejected on any other model
    check_supported(cfg)
    return cfg


CONFIGS = {
    "e2e_mask_rcnn_R-50-C4_1x": e2e_mask_rcnn_R_50_C4_1x,
    "e2e_mask_rcnn_R-50-FPN_1x": e2e_mask_rcnn_R_50_FPN_1x,
    "e2e_mask_rcnn_R-101-FPN_2x": e2e_mask_rcnn_R_101_FPN_2x,
    "e2e_mask_rcnn_X-101-32x8d-FPN_1x": e2e_mask_rcnn_X_101_32x8d_FPN_1x,
    "e2e_keypoint_rcnn_R-50-FPN_1x": e2e_keypoint_rcnn_R_50_FPN_1x,
    "vos_R-101-FPN_3x_gn_static_davis": vos_R_101_FPN_3x_gn_static_davis,
    "vos_R-101-FPN_3x_gn_dynamic_davis": vos_R_101_FPN_3x_gn_dynamic_davis,
    "vos_R-101-FPN_3x_gn_dynamic_delta_flow_davis": vos_R_101_FPN_3x_gn_dynamic_delta_flow_davis,
}


def get(name: str) -> AttrDict:
    return copy.deepcopy(CONFIGS[name]())


# The reference's module-global ``cfg`` (lib/core/config.py:25) that its
# operators read (GenerateProposalsOp, collect/distribute): the package's op
# mirrors read this one unless given a cfg explicitly.
cfg = e2e_mask_rcnn_R_50_FPN_1x()


def merge_cfg_from_file(path: str) -> None:
    """config.py:1107-1111: merge a reference YAML into the global cfg in place.
    An ``UNSUPPORTED`` option raises and leaves the global cfg unchanged."""
    with open(path) as f:
        new = copy.deepcopy(cfg)
        _merge_yaml(yaml.safe_load(f) or {}, new)
    check_supported(new)
    cfg.clear()
    cfg.update(new)


cfg_from_file = merge_cfg_from_file  # config.py:1113


def merge_cfg_from_list(cfg_list) -> None:
    """config.py:1121-1144: ['TEST.NMS', '0.4', ...] key/value pairs."""
    if len(cfg_list) % 2:
        raise ValueError("cfg_list must hold key/value pairs")
    new = copy.deepcopy(cfg)
    for key, val in zip(cfg_list[0::2], cfg_list[1::2]):
        d = new
        parts = key.split(".")
        for p in parts[:-1]:
            d = d[p]
        if parts[-1] not in d:
            raise KeyError("Non-existent config key: %s" % key)
        d[parts[-1]] = _decode(val)
    check_supported(new)
    cfg.clear()
    cfg.update(new)


def use(name: str) -> AttrDict:
    """Replace the global cfg's contents with a named BASELINE configuration."""
    cfg.clear()
    cfg.update(get(name))
    return cfg
