"""OKS NMS without a GPU: the numpy restatement (tests/oks_ref.py) against the executed
reference's fixture (tests/golden/nms_oks.npz), the fixture's own conditions, the host
argument checks of vd_nms_oks_frames / vd_compute_oks (they return before any launch),
the ValueErrors of ops / keypoints / KeypointFramePipeline, and the config message.
Reference: lib/utils/keypoints.py:225-266, lib/core/test.py:864-870."""
import numpy as np
import pytest
import torch

from tests import oks_ref
from vosdetectron_amd import config as vcfg

f32 = np.float32
NAME = "e2e_keypoint_rcnn_R-50-FPN_1x"


@pytest.fixture(scope="module")
def fixture():
    return oks_ref.fixture_cases()


def test_fixture_cases_and_conditions(fixture):
    """The generator's conditions, asserted again on the committed file."""
    thresh, _, cases = fixture
    assert thresh == 0.3
    assert [c["n"] for c in cases] == [1, 2, 12, 16, 17, 64, 65, 100, 256, 300]
    assert [c["kind"] for c in cases].count("ties") == 1 and cases[2]["kind"] == "ties"
    for c in cases:
        n, kp, rois = c["n"], c["kp"], c["rois"]
        assert kp.shape == (n, 4, 17) and kp.dtype == f32 and rois.shape == (n, 4)
        assert not np.isnan(kp).any()
        flat = np.concatenate(c["ovr"]) if c["ovr"] else np.zeros(0)
        assert np.all(np.abs(flat - thresh) >= 1e-6), n
        ss = np.sort(c["scores"])
        gaps = np.diff(ss) / np.spacing(np.abs(ss[1:]))
        if c["kind"] == "ties":
            assert int((gaps == 0).sum()) == 2 and np.all(gaps[gaps != 0] >= 16)
        else:
            assert np.all(gaps >= 16), n
        if n >= 16:
            above = below = False
            for r in range(n):
                same = np.flatnonzero(c["cluster"] == c["cluster"][r])
                same = same[same != r]
                if len(same):
                    v = oks_ref.compute_oks(kp[r], rois[r], kp[same])
                    above |= bool((v > thresh + 1e-6).any())
                    below |= bool((v < thresh - 1e-6).any())
            assert above and below, n
            assert 1 < len(c["keep"]) < n


def test_restatement_matches_executed_reference(fixture):
    thresh, ref_vars, cases = fixture
    assert oks_ref.VARS.dtype == np.float64
    assert np.array_equal(oks_ref.VARS.view(np.uint64), ref_vars.view(np.uint64))
    for c in cases:
        sc = oks_ref.scores(c["kp"])
        assert sc.dtype == f32 and np.array_equal(sc.view(np.uint32), c["scores"].view(np.uint32))
        rec = []
        keep = oks_ref.nms_oks(c["kp"], c["rois"], thresh, record=rec)
        assert keep == c["keep"].tolist(), c["n"]
        assert len(rec) == len(c["ovr"])
        for a, b in zip(rec, c["ovr"]):
            assert a.dtype == np.float64 and a.shape == b.shape
            assert a.size == 0 or float(np.abs(a - b).max()) <= 1e-12


def test_tie_order_is_higher_index_first(fixture):
    """Rows 7 / 9 carry the logits of rows 2 / 4 and a pose 0.25 px beside them: the
    higher index is processed first and kept, the lower one dropped."""
    thresh, _, cases = fixture
    c = cases[2]
    sc = c["scores"]
    assert sc[2] == sc[7] and sc[4] == sc[9]
    order = oks_ref.processing_order(sc).tolist()
    assert order.index(7) + 1 == order.index(2) and order.index(9) + 1 == order.index(4)
    keep = c["keep"].tolist()
    for lo, hi in ((2, 7), (4, 9)):
        assert hi in keep and lo not in keep
    assert oks_ref.processing_order(np.array([1, 3, 3, 2, 3], f32)).tolist() == [4, 2, 1, 3, 0]


def test_restatement_frames_layout(fixture):
    """nms_oks_frames: prefix-sum row bases, the negative count passed through, zeros
    and -1 past the counts."""
    thresh, _, cases = fixture
    pick = [cases[1], cases[4]]
    D = 32
    counts = np.array([2, -3, 17, 0], np.int32)
    keyps = np.concatenate([c["kp"] for c in pick])
    dets = np.zeros((4, D, 5), f32)
    dets[0, :2, :4], dets[2, :17, :4] = pick[0]["rois"], pick[1]["rois"]
    dets[..., 4] = np.arange(4 * D, dtype=f32).reshape(4, D)
    cls = np.ones((4, D), np.int32)
    out = oks_ref.nms_oks_frames(keyps, dets, cls, counts, thresh)
    k0, k2 = pick[0]["keep"], pick[1]["keep"]
    assert out["counts"].tolist() == [len(k0), -3, len(k2), 0]
    assert out["keep"][2, :len(k2)].tolist() == k2.tolist() and np.all(out["keep"][1] == -1)
    assert np.array_equal(out["keyps"][:len(k0)], pick[0]["kp"][k0])
    assert np.array_equal(out["keyps"][len(k0):len(k0) + len(k2)], pick[1]["kp"][k2])
    assert not out["keyps"][len(k0) + len(k2):].any()
    assert np.array_equal(out["dets"][2, :len(k2)], dets[2, k2]) and not out["dets"][1].any()


def test_host_argument_errors_without_gpu():
    from vosdetectron_amd import _lib
    L = _lib.lib()
    fn = L.vd_nms_oks_frames
    p = 256  # any non-null address: validation returns before a launch

    def call(keyps=p, rows=8, K=17, dets=p, cls=p, cnt=p, F=2, D=256, keep=p, cout=p, dout=p,
             clsout=p, kout=p, scores=None):
        return fn(keyps, rows, K, dets, cls, cnt, F, D, 0.3, keep, cout, dout, clsout, kout,
                  scores, None)
    assert call(None, 0, 17, None, None, None, 0, 256, None, None, None, None, None) == _lib.VD_OK
    for name in ("keyps", "dets", "cls", "cnt", "keep", "cout", "dout", "clsout", "kout"):
        assert call(**{name: None}) == _lib.VD_ERR_ARG, name
    assert call(K=16) == _lib.VD_ERR_ARG and call(K=18) == _lib.VD_ERR_ARG
    assert call(D=513) == _lib.VD_ERR_SHAPE and call(D=100000) == _lib.VD_ERR_SHAPE
    assert call(D=0) == _lib.VD_ERR_ARG and call(F=-1) == _lib.VD_ERR_ARG
    assert call(rows=-1) == _lib.VD_ERR_ARG
    fn = L.vd_compute_oks
    assert fn(None, None, None, 0, 17, None, None) == _lib.VD_OK  # N == 0
    assert fn(None, p, p, 3, 17, p, None) == _lib.VD_ERR_ARG
    assert fn(p, None, p, 3, 17, p, None) == _lib.VD_ERR_ARG
    assert fn(p, p, None, 3, 17, p, None) == _lib.VD_ERR_ARG
    assert fn(p, p, p, 3, 17, None, None) == _lib.VD_ERR_ARG
    assert fn(p, p, p, 3, 16, p, None) == _lib.VD_ERR_ARG
    assert fn(p, p, p, -1, 17, p, None) == _lib.VD_ERR_ARG


def _frames_args(F=2, D=8, rows=6, K=17):
    return dict(keyps=torch.zeros(rows, 4, K), dets=torch.zeros(F, D, 5),
                classes=torch.ones(F, D, dtype=torch.int32),
                counts=torch.zeros(F, dtype=torch.int32))


def test_ops_value_errors_name_the_argument():
    """Every check runs on the host before a launch; the device check comes last, so CPU
    tensors that are otherwise valid raise it."""
    from vosdetectron_amd import ops
    ok = _frames_args()
    with pytest.raises(ValueError, match="keyps.*device"):
        ops.nms_oks_frames(**ok)
    with pytest.raises(ValueError, match=r"keyps: K = 16"):
        ops.nms_oks_frames(**dict(ok, keyps=torch.zeros(6, 4, 16)))
    with pytest.raises(ValueError, match="keyps must be rows x 4 x K"):
        ops.nms_oks_frames(**dict(ok, keyps=torch.zeros(6, 3, 17)))
    with pytest.raises(ValueError, match="keyps must be torch.float32"):
        ops.nms_oks_frames(**dict(ok, keyps=torch.zeros(6, 4, 17, dtype=torch.float64)))
    with pytest.raises(ValueError, match="keyps must be contiguous"):
        ops.nms_oks_frames(**dict(ok, keyps=torch.zeros(6, 17, 4).transpose(1, 2)))
    with pytest.raises(ValueError, match="dets must be F x D x 5"):
        ops.nms_oks_frames(**dict(ok, dets=torch.zeros(2, 8, 4)))
    with pytest.raises(ValueError, match="dets must be contiguous"):
        ops.nms_oks_frames(**dict(ok, dets=torch.zeros(2, 8, 10)[:, :, ::2]))
    with pytest.raises(ValueError, match="classes must be torch.int32"):
        ops.nms_oks_frames(**dict(ok, classes=torch.ones(2, 8, dtype=torch.int64)))
    with pytest.raises(ValueError, match="classes must be F x D"):
        ops.nms_oks_frames(**dict(ok, classes=torch.ones(2, 7, dtype=torch.int32)))
    with pytest.raises(ValueError, match="counts must be torch.int32"):
        ops.nms_oks_frames(**dict(ok, counts=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match="counts must be F"):
        ops.nms_oks_frames(**dict(ok, counts=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match=r"dets: D = 513"):
        ops.nms_oks_frames(**_frames_args(D=513))
    with pytest.raises(ValueError, match=r"keyps has 6 rows, the counts \[4, -1, 3\] need 7"):
        ops.nms_oks_frames(**_frames_args(F=3), counts_host=[4, -1, 3])
    with pytest.raises(TypeError, match="keyps"):
        ops.nms_oks_frames(**dict(ok, keyps=np.zeros((6, 4, 17), f32)))

    s, b, d = torch.zeros(4, 17), torch.zeros(4), torch.zeros(3, 4, 17)
    with pytest.raises(ValueError, match="src_keypoints.*device"):
        ops.compute_oks(s, b, d)
    with pytest.raises(ValueError, match=r"src_keypoints: K = 16"):
        ops.compute_oks(torch.zeros(4, 16), b, d)
    with pytest.raises(ValueError, match="src_roi must be a vector"):
        ops.compute_oks(s, torch.zeros(3), d)
    with pytest.raises(ValueError, match="dst_keypoints must be N x 4 x 17"):
        ops.compute_oks(s, b, torch.zeros(3, 4, 16))
    with pytest.raises(ValueError, match="dst_keypoints must be torch.float32"):
        ops.compute_oks(s, b, d.double())


def test_keypoints_entries_value_errors():
    from vosdetectron_amd import keypoints
    with pytest.raises(ValueError, match="kp_predictions must be n x 4 x 17"):
        keypoints.nms_oks(np.zeros((3, 4, 16), f32), np.zeros((3, 4), f32), 0.3)
    with pytest.raises(ValueError, match="rois must be 3 x >=4"):
        keypoints.nms_oks(np.zeros((3, 4, 17), f32), np.zeros((2, 4), f32), 0.3)
    with pytest.raises(ValueError, match=r"n = 513"):
        keypoints.nms_oks(torch.zeros(513, 4, 17), torch.zeros(513, 4), 0.3)
    with pytest.raises(ValueError, match="src_keypoints must be 4 x 17"):
        keypoints.compute_oks(np.zeros((4, 16)), np.zeros(4), np.zeros((2, 4, 17)), None)
    with pytest.raises(ValueError, match="dst_keypoints must be N x 4 x 17"):
        keypoints.compute_oks(np.zeros((4, 17)), np.zeros(4), np.zeros((2, 3, 17)), None)


def test_pipeline_switch_needs_person_only_config():
    """The check precedes every device allocation: no model or GPU is needed to hit it."""
    from vosdetectron_amd.engine import KeypointFramePipeline
    cfg = vcfg.get(NAME)
    assert cfg.MODEL.NUM_CLASSES != 2
    for v in (True, 0.3, 0.5):
        with pytest.raises(ValueError, match=r"NUM_CLASSES == 2"):
            KeypointFramePipeline(None, cfg, nms_oks=v, device="cpu")
    cfg.MODEL.NUM_CLASSES = 2
    with pytest.raises(ValueError, match="det_cap = 1024"):
        KeypointFramePipeline(None, cfg, nms_oks=True, det_cap=1024, device="cpu")


def test_config_key_still_rejected_and_points_to_the_argument():
    with pytest.raises(NotImplementedError, match=r"KRCNN\.NMS_OKS.*nms_oks=True"):
        vcfg.load_cfg(overrides={"KRCNN.NMS_OKS": True})
