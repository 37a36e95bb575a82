"""Keypoint R-CNN without a GPU: the config block and its rejections, the numpy
restatement's own properties (tests/keypoint_ref.py), model construction (state-dict
names, the fixed bilinear filter) and vd_heatmaps_to_keypoints' host-side checks.
Reference: configs/baselines/e2e_keypoint_rcnn_*.yaml, lib/core/config.py:783-855,
lib/modeling/keypoint_rcnn_heads.py, lib/utils/keypoints.py:103-157."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import keypoint_ref as kref
from vosdetectron_amd import config as vcfg

REF = "/root/reference"
NAME = "e2e_keypoint_rcnn_R-50-FPN_1x"
f32 = np.float32


def test_named_config_loads():
    c = vcfg.get(NAME)
    assert c.MODEL.KEYPOINTS_ON is True and c.MODEL.MASK_ON is False
    kc = c.KRCNN
    assert (kc.ROI_KEYPOINTS_HEAD, kc.NUM_STACKED_CONVS, kc.CONV_HEAD_DIM) == \
        ("keypoint_rcnn_heads.roi_pose_head_v1convX", 8, 512)
    assert (kc.NUM_KEYPOINTS, kc.HEATMAP_SIZE, kc.UP_SCALE, kc.USE_DECONV_OUTPUT) == \
        (17, 56, 2, True)
    assert (kc.ROI_XFORM_RESOLUTION, kc.ROI_XFORM_SAMPLING_RATIO, kc.INFERENCE_MIN_SIZE) == \
        (14, 2, 0)
    # the mask configs carry the block at its defaults
    d = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    assert d.MODEL.KEYPOINTS_ON is False and d.KRCNN.NUM_KEYPOINTS == -1


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent")
def test_named_config_matches_reference_yaml():
    ours = vcfg.get(NAME)
    ref = vcfg.load_cfg(os.path.join(REF, "configs/baselines", NAME + ".yaml"))
    for k in ref.KRCNN:
        assert ours.KRCNN[k] == ref.KRCNN[k], k
    for k in ("KEYPOINTS_ON", "MASK_ON", "NUM_CLASSES", "CONV_BODY", "FASTER_RCNN"):
        assert ours.MODEL[k] == ref.MODEL[k], k
    for k in ref.TEST:
        assert ours.TEST[k] == ref.TEST[k], k
    for grp in ("FPN", "FAST_RCNN", "RESNETS"):
        assert ours[grp] == ref[grp], grp


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent")
def test_all_keypoint_yamls_load():
    paths = sorted(glob.glob(os.path.join(REF, "configs/baselines/e2e_keypoint_rcnn_*.yaml")))
    assert len(paths) == 8
    for p in paths:
        c = vcfg.load_cfg(p)
        assert c.MODEL.KEYPOINTS_ON and not c.MODEL.MASK_ON, p
        assert c.KRCNN.HEATMAP_SIZE == 56 and c.KRCNN.NUM_KEYPOINTS == 17, p


def test_config_rejections_name_the_key():
    base = {"MODEL.KEYPOINTS_ON": True, "MODEL.MASK_ON": False, "FPN.FPN_ON": True,
            "KRCNN.ROI_KEYPOINTS_HEAD": vcfg.KEYPOINT_HEAD}
    vcfg.load_cfg(overrides=base)  # the supported combination loads
    with pytest.raises(NotImplementedError, match=r"KRCNN\.NMS_OKS"):
        vcfg.load_cfg(overrides=dict(base, **{"KRCNN.NMS_OKS": True}))
    with pytest.raises(NotImplementedError, match=r"MODEL\.KEYPOINTS_ON.*MODEL\.MASK_ON"):
        vcfg.load_cfg(overrides=dict(base, **{"MODEL.MASK_ON": True}))
    with pytest.raises(NotImplementedError, match=r"KRCNN\.ROI_KEYPOINTS_HEAD"):
        vcfg.load_cfg(overrides=dict(base, **{"KRCNN.ROI_KEYPOINTS_HEAD": "other.head"}))
    with pytest.raises(NotImplementedError, match=r"MODEL\.KEYPOINTS_ON.*C4"):
        vcfg.load_cfg(overrides=dict(base, **{"FPN.FPN_ON": False}))
    # OKS NMS is rejected whether or not keypoints are on; the head name only with them
    with pytest.raises(NotImplementedError, match=r"KRCNN\.NMS_OKS"):
        vcfg.load_cfg(overrides={"KRCNN.NMS_OKS": True})
    vcfg.load_cfg(overrides={"KRCNN.ROI_KEYPOINTS_HEAD": "other.head"})


def test_restatement_tap_weights():
    """2x upscale: t is 0.75 / 0.25 alternately and the weights are exact binary
    fractions."""
    idx, w = kref.cubic_taps(16, 8)
    q = (f32(-0.10546875), f32(0.87890625), f32(0.26171875), f32(-0.03515625))
    for d in range(16):
        t = ((d + 0.5) * 0.5 - 0.5) % 1.0
        want = q if t == 0.25 else q[::-1]
        assert t in (0.25, 0.75) and tuple(w[d]) == want, (d, t, w[d])
    assert idx[0].tolist() == [0, 0, 0, 1] and idx[15].tolist() == [6, 7, 7, 7]  # replicate
    assert idx[5].tolist() == [1, 2, 3, 4]


def test_restatement_identity_scale():
    rng = np.random.default_rng(3)
    M, K = 12, 3
    maps = rng.standard_normal((1, K, M, M)).astype(f32)
    box = np.array([[5.5, -3.25, 5.5 + M, -3.25 + M]], f32)
    out = kref.heatmaps_to_keypoints(maps, box)
    for k in range(K):
        yi, xi = divmod(int(maps[0, k].argmax()), M)
        assert out[0, 0, k] == f32(xi + 0.5 + 5.5) and out[0, 1, k] == f32(yi + 0.5 - 3.25)
        assert out[0, 2, k] == maps[0, k, yi, xi]
    assert np.array_equal(kref.resize_cubic(maps[0, 0], M, M), maps[0, 0])


def test_restatement_constant_map():
    """A constant map resized by 2x and 4x (tap weights exact binary fractions that
    sum to exactly 1) stays constant: the first index wins, prob = 1 / (Wm * Hm)."""
    maps = np.full((1, 2, 8, 8), 1.5, f32)
    box = np.array([[10, 20, 10 + 16, 20 + 31.5]], f32)  # Wm = 16, Hm = 32
    assert kref.map_size(box[0])[2:] == (16, 32)
    assert np.array_equal(kref.resize_cubic(maps[0, 0], 32, 16), np.full((32, 16), 1.5, f32))
    out = kref.heatmaps_to_keypoints(maps, box)
    wc, hc = f32(16) / f32(16), f32(31.5) / f32(32)
    for k in range(2):
        assert out[0, 0, k] == f32(0.5 * np.float64(wc) + 10)
        assert out[0, 1, k] == f32(0.5 * np.float64(hc) + 20)
        assert out[0, 2, k] == f32(1.5)
        assert out[0, 3, k] == f32(1. / (16 * 32))


def test_restatement_min_size_and_small_box():
    w, h, Wm, Hm = kref.map_size([10.3, 20.7, 10.9, 21.2])
    assert (w, h, Wm, Hm) == (f32(1), f32(1), 1, 1)
    assert kref.map_size([0, 0, 3.2, 40.5], 16)[2:] == (16, 41)


def test_model_state_dict_names():
    from vosdetectron_amd.modeling import Generalized_RCNN, bilinear_upsample_filter
    kp = Generalized_RCNN(vcfg.get(NAME))
    sd = kp.state_dict()
    for i in range(8):
        assert tuple(sd["Keypoint_Head.conv_fcn.%d.weight" % (2 * i)].shape) == \
            (512, 256 if i == 0 else 512, 3, 3)
        assert tuple(sd["Keypoint_Head.conv_fcn.%d.bias" % (2 * i)].shape) == (512,)
    assert tuple(sd["Keypoint_Outs.classify.weight"].shape) == (512, 17, 4, 4)
    assert tuple(sd["Keypoint_Outs.classify.bias"].shape) == (17,)
    assert tuple(sd["Keypoint_Outs.upsample.upconv.weight"].shape) == (17, 17, 4, 4)
    assert not [k for k in sd if k.startswith("Mask_")]
    assert not [k for k in sd if "deconv" in k]  # USE_DECONV off
    up = kp.Keypoint_Outs.upsample.upconv
    assert (up.stride, up.padding, up.kernel_size) == ((2, 2), (1, 1), (4, 4))
    cl = kp.Keypoint_Outs.classify
    assert (cl.stride, cl.padding, cl.kernel_size) == ((2, 2), (1, 1), (4, 4))
    # the FCN bilinear filter on the channel diagonal, zero elsewhere and zero bias
    tri = np.array([0.25, 0.75, 0.75, 0.25])
    filt = np.outer(tri, tri).astype(f32)
    assert np.array_equal(bilinear_upsample_filter(4).astype(f32), filt)
    w = sd["Keypoint_Outs.upsample.upconv.weight"].numpy()
    for a in range(17):
        for b in range(17):
            assert np.array_equal(w[a, b], filt if a == b else np.zeros((4, 4), f32)), (a, b)
    assert not sd["Keypoint_Outs.upsample.upconv.bias"].any()
    # the synthetic weights leave the filter as constructed
    from vosdetectron_amd.weights import synthetic_state_dict
    syn = synthetic_state_dict(kp)
    assert torch.equal(syn["Keypoint_Outs.upsample.upconv.weight"],
                       sd["Keypoint_Outs.upsample.upconv.weight"])
    assert syn["Keypoint_Outs.classify.weight"].abs().max() > 0

    cfg = vcfg.get(NAME)
    cfg.KRCNN.USE_DECONV = True
    sd2 = Generalized_RCNN(cfg).state_dict()
    assert tuple(sd2["Keypoint_Outs.deconv.weight"].shape) == (512, 256, 4, 4)
    assert tuple(sd2["Keypoint_Outs.classify.weight"].shape) == (256, 17, 4, 4)


def test_mask_model_has_no_keypoint_modules():
    from vosdetectron_amd.modeling import Generalized_RCNN
    sd = Generalized_RCNN(vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")).state_dict()
    assert not [k for k in sd if k.startswith("Keypoint_")]
    assert "Mask_Head.conv_fcn.0.weight" in sd and "Mask_Outs.classify.weight" in sd


def test_head_restatement_shapes():
    """The torch CPU restatement runs the state-dict of the built model: 14 -> 56."""
    from vosdetectron_amd.modeling import Generalized_RCNN
    cfg = vcfg.get(NAME)
    cfg.KRCNN.NUM_STACKED_CONVS, cfg.KRCNN.CONV_HEAD_DIM = 2, 64
    m = Generalized_RCNN(cfg)
    x = torch.randn(2, 256, 14, 14, generator=torch.Generator().manual_seed(0))
    y = kref.keypoint_head_outputs(m.state_dict(), x, cfg, torch.float64)
    assert tuple(y.shape) == (2, 17, 56, 56) and y.dtype == torch.float64
    with torch.no_grad():
        z = m.Keypoint_Outs(m.Keypoint_Head.head(x))
    assert float((z.double() - y).abs().max()) <= 1e-5 * float(y.abs().max())


def test_host_argument_errors_without_gpu():
    from vosdetectron_amd import _lib
    L = _lib.lib()
    fn = L.vd_heatmaps_to_keypoints
    p = 256  # any non-null address: validation returns before a launch
    assert fn(None, 0, 17, 56, None, 4, 0, None, None) == _lib.VD_OK  # R == 0
    assert fn(None, 2, 17, 56, p, 4, 0, p, None) == _lib.VD_ERR_ARG
    assert fn(p, 2, 17, 56, None, 4, 0, p, None) == _lib.VD_ERR_ARG
    assert fn(p, 2, 17, 56, p, 4, 0, None, None) == _lib.VD_ERR_ARG
    assert fn(p, 2, 17, 65, p, 4, 0, p, None) == _lib.VD_ERR_ARG  # M > 64
    assert fn(p, 2, 33, 56, p, 4, 0, p, None) == _lib.VD_ERR_ARG  # K > 32
    assert fn(p, 2, 17, 56, p, 3, 0, p, None) == _lib.VD_ERR_ARG  # stride < 4
    assert fn(p, -1, 17, 56, p, 4, 0, p, None) == _lib.VD_ERR_ARG
    assert fn(p, 2, 17, 56, p, 4, -1, p, None) == _lib.VD_ERR_ARG


def test_keypoint_names():
    from vosdetectron_amd import keypoints
    names, flip = keypoints.get_keypoints()
    assert len(names) == 17 and names[0] == "nose" and names[-1] == "right_ankle"
    assert len(flip) == 8 and flip["left_eye"] == "right_eye" and flip["left_ankle"] == "right_ankle"
    assert all(k in names and v in names for k, v in flip.items())
    assert keypoints.get_person_class_index() == 1
