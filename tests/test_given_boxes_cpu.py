"""Detection from given boxes without a device: the numpy restatement
(tests/given_boxes_ref.py) against the fixture the reference's own im_detect_bbox wrote
(tests/golden/given_boxes.npz), the two planted defects the fixture must catch, the C
entries' refusals and the config / pipeline rules."""
import ctypes
import os

import numpy as np
import pytest

from tests import given_boxes_ref as gb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "given_boxes.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _restated(golden, tag, name, **defect):
    pre = "%s/%s/" % (tag, name)
    return gb.detect_bbox(golden[pre + "boxes"], float(golden[pre + "im_scale"]),
                          float(golden[pre + "dedup"]), tuple(golden[pre + "im_shape"]),
                          fpn=tag == "fpn", **defect), pre


def _differs(golden, tag, name, **defect):
    got, pre = _restated(golden, tag, name, **defect)
    keys = gb.RECORDED_FPN if tag == "fpn" else gb.RECORDED
    return [k for k in keys if got[k].shape != golden[pre + k].shape
            or got[k].tobytes() != golden[pre + k].astype(got[k].dtype).tobytes()]


def test_fixture_holds_the_cases_of_the_generator(golden):
    cases = gb.case_boxes()
    assert tuple(cases) == gb.CASES
    for tag in ("fpn", "single"):
        for name, (boxes, im_shape, _, dd) in cases.items():
            pre = "%s/%s/" % (tag, name)
            assert np.array_equal(golden[pre + "boxes"], boxes) and boxes.dtype == np.float32
            assert float(golden[pre + "dedup"]) == dd
            assert tuple(golden[pre + "im_shape"]) == im_shape
    assert float(golden["fpn/scaled/im_scale"]) == 1.6 and float(golden["fpn/n64/im_scale"]) == 1.0
    sizes = {n: len(c[0]) for n, c in cases.items()}
    assert (sizes["n1"], sizes["n5_equal"], sizes["n64"], sizes["n65"], sizes["n300"]) == \
        (1, 5, 64, 65, 300)
    assert len(golden["fpn/n5_equal/rois"]) == 1
    assert 180 <= len(golden["fpn/n300/rois"]) <= 230  # about a third are duplicates
    assert len(golden["fpn/dedup0/rois"]) == sizes["dedup0"]
    # below the quantum: rows 0, 3 and 4 share a hash, different boxes merged onto row 0
    inv = golden["fpn/below_quantum/inv_index"]
    assert inv[0] == inv[3] == inv[4] and inv[1] != inv[2]
    assert golden["fpn/below_quantum/index"][inv[0]] == 0


@pytest.mark.parametrize("tag", ("fpn", "single"))
@pytest.mark.parametrize("name", gb.CASES)
def test_restatement_equals_the_executed_reference_bit_for_bit(golden, tag, name):
    assert _differs(golden, tag, name) == []
    got, pre = _restated(golden, tag, name)
    assert got["scores"].dtype == golden[pre + "scores"].dtype == np.float32
    assert got["pred_boxes"].dtype == golden[pre + "pred_boxes"].dtype == np.float32
    assert got["rois"].dtype == golden[pre + "rois"].dtype == np.float32


def test_round_half_away_breaks_the_equality(golden):
    """np.round is half to even; a hash that rounds half away from zero groups the
    half_even case's rows differently."""
    bad = _differs(golden, "fpn", "half_even", half_away=True)
    assert "inv_index" in bad and "rois" in bad and "scores" in bad, bad
    assert any(_differs(golden, "single", n, half_away=True) for n in gb.CASES)


def test_last_occurrence_breaks_the_equality(golden):
    """np.unique's return_index is the FIRST row of each hash: taking the last one shows in
    the rows the head saw (merged boxes that differ) and in the decoded boxes."""
    bad = _differs(golden, "fpn", "below_quantum", last=True)
    assert "index" in bad and "rois" in bad and "pred_boxes" in bad, bad
    assert "index" in _differs(golden, "single", "n300", last=True)


def test_frames_restatement_pads_and_flags():
    boxes = np.zeros((3, 4, 4), np.float32)
    boxes[0, :3] = [[0, 0, 50, 50], [100, 100, 150, 150], [0, 0, 50, 50]]
    boxes[2, :2] = [[0, 0, 50, 50], [0, 0, 50, 50]]
    rois, ucounts, index, inv = gb.rois_from_boxes(boxes, [3, 0, 5], [1., 1., 1.], 0.0625)
    assert ucounts.tolist() == [2, 0, -1]
    assert index[0, :2].tolist() == [0, 1] and inv[0, :3].tolist() == [0, 1, 0]
    assert not rois[1:].any() and not index[1:].any() and not inv[1:].any()
    rois, ucounts, index, inv = gb.rois_from_boxes(boxes, [3, 0, 2], [1., 1., 1.], 0.0625)
    # the same boxes in two frames: column 0 differs, nothing merges across frames
    assert ucounts.tolist() == [2, 0, 1] and rois[0, 0, 0] == 0 and rois[2, 0, 0] == 2
    assert np.array_equal(rois[0, 0, 1:], rois[2, 0, 1:])


# --------------------------------------------------------------------------- #
# the C entries' refusals: all before the first launch                         #
# --------------------------------------------------------------------------- #
def test_c_entry_refusals_without_a_device():
    from vosdetectron_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    assert L.vd_rois_from_boxes_workspace(3, 64) == 0  # the keys live in LDS

    def rfb(boxes=p, counts=p, scale=p, dedup=0.0625, F=3, cap=64, rois=p, ucounts=p, index=p,
            inv=p):
        return L.vd_rois_from_boxes(boxes, counts, scale, dedup, F, cap, rois, ucounts, index,
                                    inv, None, 0, None)

    for name in ("boxes", "counts", "scale", "rois", "ucounts", "index", "inv"):
        assert rfb(**{name: None}) == _lib.VD_ERR_ARG, name
    assert rfb(F=-1) == _lib.VD_ERR_ARG
    assert rfb(dedup=-0.5) == _lib.VD_ERR_ARG and rfb(dedup=float("nan")) == _lib.VD_ERR_ARG
    assert rfb(cap=0) == _lib.VD_ERR_SHAPE and rfb(cap=4097) == _lib.VD_ERR_SHAPE
    assert rfb(F=0) == _lib.VD_OK

    def gather(boxes=p, scores=p, deltas=p, index=p, inv=p, counts=p, ucounts=p, F=3, cap=64,
               K=5, D=20, ro=p, so=p, do=p, co=p):
        return L.vd_gather_rows(boxes, scores, deltas, index, inv, counts, ucounts, F, cap, K, D,
                                ro, so, do, co, None)

    for name in ("boxes", "scores", "deltas", "index", "inv", "counts", "ucounts", "ro", "so",
                 "do", "co"):
        assert gather(**{name: None}) == _lib.VD_ERR_ARG, name
    for kw in ({"cap": 0}, {"cap": 4097}, {"F": 65536}, {"K": 0}, {"D": 0}):
        assert gather(**kw) == _lib.VD_ERR_SHAPE, kw
    assert gather(F=0) == _lib.VD_OK


# --------------------------------------------------------------------------- #
# config and pipeline rules                                                    #
# --------------------------------------------------------------------------- #
def test_config_accepts_fast_rcnn_and_reads_dedup_boxes(tmp_path):
    from vosdetectron_amd import config
    assert config.default_cfg().DEDUP_BOXES == 0.0625
    cfg = config.load_cfg(None, {"MODEL.FASTER_RCNN": False})
    assert cfg.MODEL.FASTER_RCNN is False and cfg.DEDUP_BOXES == 0.0625
    y = tmp_path / "fast.yaml"
    y.write_text("MODEL:\n  FASTER_RCNN: False\nDEDUP_BOXES: 0.1\nTRAIN:\n  SCALES: (600,)\n")
    cfg = config.load_cfg(str(y))
    assert cfg.MODEL.FASTER_RCNN is False and cfg.DEDUP_BOXES == 0.1
    y.write_text("TRAIN:\n  BBOX_NORMALIZE_TARGETS_PRECOMPUTED: True\n")
    with pytest.raises(NotImplementedError, match="TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED"):
        config.load_cfg(str(y))


def _fast_cfg(**over):
    from vosdetectron_amd import config
    o = {"MODEL.FASTER_RCNN": False, "FPN.FPN_ON": True, "FPN.MULTILEVEL_ROIS": True,
         "FPN.MULTILEVEL_RPN": True}
    o.update(over)
    return config.load_cfg(None, o)


class _Model:  # _setup reads nothing else of a model before it raises
    Mask_Head = Keypoint_Head = None


def test_model_builds_without_rpn_and_loads_a_state_dict_that_lacks_it():
    from vosdetectron_amd import config
    from vosdetectron_amd.modeling import Generalized_RCNN
    full = Generalized_RCNN(config.e2e_mask_rcnn_R_50_FPN_1x())
    cfg = config.e2e_mask_rcnn_R_50_FPN_1x()
    cfg.MODEL.FASTER_RCNN = False
    fast = Generalized_RCNN(cfg)
    assert hasattr(full, "RPN") and hasattr(full, "anchors_fpn2")
    assert not hasattr(fast, "RPN") and not hasattr(fast, "anchors_fpn2")
    sd = {k: v for k, v in full.state_dict().items() if not k.startswith("RPN.")}
    assert len(sd) < len(full.state_dict())
    fast.load_state_dict(sd, strict=True)  # nothing missing, nothing unexpected
    with pytest.raises(RuntimeError, match="RPN"):
        fast.load_state_dict(full.state_dict(), strict=True)


@pytest.mark.parametrize("which", ("ragged", "c4", "aug", "keypoint", "keypoint_aug"))
def test_other_pipelines_refuse_given_boxes_by_name(which):
    from vosdetectron_amd import c4, config, engine
    if which == "ragged":
        cls, cfg, args = engine.RaggedFramePipeline, _fast_cfg(), ((64, 64),)
    elif which == "c4":
        cls, cfg, args = c4.C4FramePipeline, _fast_cfg(**{"FPN.FPN_ON": False}), ()
    elif which == "aug":
        cfg = config.load_cfg(None, {"MODEL.FASTER_RCNN": False, "FPN.FPN_ON": True,
                                     "TEST.BBOX_AUG.ENABLED": True, "TEST.BBOX_AUG.H_FLIP": True},
                              test_aug=True)
        cls, args = engine.AugFramePipeline, ()
    else:
        o = {"MODEL.FASTER_RCNN": False, "FPN.FPN_ON": True, "MODEL.KEYPOINTS_ON": True,
             "MODEL.MASK_ON": False, "KRCNN.ROI_KEYPOINTS_HEAD": config.KEYPOINT_HEAD}
        if which == "keypoint_aug":
            o.update({"TEST.KPS_AUG.ENABLED": True, "TEST.KPS_AUG.H_FLIP": True})
        cfg = config.load_cfg(None, o, test_aug=which == "keypoint_aug")
        cls = engine.KeypointAugFramePipeline if which == "keypoint_aug" \
            else engine.KeypointFramePipeline
        args = ()
    with pytest.raises(NotImplementedError, match=cls.__name__):
        cls(_Model(), cfg, *args, device="cpu")


def test_box_proposals_value_errors():
    """With MODEL.FASTER_RCNN True the reference ignores the caller's boxes: ValueError;
    with it False they are required: ValueError.  Both before anything runs."""
    from vosdetectron_amd import config, engine

    def pipe(cls, faster):
        p = cls.__new__(cls)
        p.given_boxes = not faster
        return p

    frames = np.zeros((2, 8, 8, 3), np.uint8)
    for cls in (engine.FramePipeline, engine.VOSPipeline):
        with pytest.raises(ValueError, match="MODEL.FASTER_RCNN True"):
            pipe(cls, True)._check_box_proposals((None, None), frames)
        assert pipe(cls, True)._check_box_proposals(None, frames) is None
        with pytest.raises(ValueError, match="needs box_proposals"):
            pipe(cls, False)._check_box_proposals(None, frames)
        with pytest.raises(ValueError, match="device tensor"):
            pipe(cls, False)._check_box_proposals(
                (np.zeros((2, 4, 4), np.float32), np.zeros((2,), np.int32)), frames)
    for cls in (engine.RaggedFramePipeline, engine.AugFramePipeline,
                engine.KeypointFramePipeline, engine.KeypointAugFramePipeline):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            pipe(cls, True)._check_box_proposals((None, None), frames)
    assert config.default_cfg().MODEL.FASTER_RCNN is True
