"""Keypoint test-time augmentation (TEST.KPS_AUG) on the device.

1. vd_heatmaps_to_keypoints_aug: its combined maps equal the executed reference's
   (tests/golden/kps_aug.npz) bit for bit; the fused launch equals the plain decode of
   its own combined maps in all four rows, prob included (the code after the load is
   shared); against the numpy restatement (tests/kps_aug_ref.py, tests/keypoint_ref.py)
   the combination, x, y and logit are exact and prob is within the plain decode's
   rtol 1e-5 (tests/test_keypoints_gpu.py derives it); argument errors; R = 0.
2. KeypointAugFramePipeline on e2e_keypoint_rcnn_R-50-FPN_1x, 320 x 480 frames, batch 2,
   seed-0 weights, six keypoint views, with TEST.BBOX_AUG off and on: stage-wise on the
   step's own tensors, then the pipeline's contracts (off = KeypointFramePipeline,
   sync=False + complete, graph replay, nms_oks, the row ranges, the refusals).
Reference: lib/core/test.py:567-730, lib/utils/keypoints.py:90-100."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import aug_ref, keypoint_ref as kref, kps_aug_ref as kar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAME = "e2e_keypoint_rcnn_R-50-FPN_1x"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kps_aug.npz")
f32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_decode(got, ref, what=""):
    """x, y, logit bit for bit; prob within the plain decode's bound."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == np.float32
    perr = np.abs(got[:, 3] - ref[:, 3]) / ref[:, 3]
    print("%s decode: %d x %d keypoints, max relative prob error %.3g"
          % (what, ref.shape[0], ref.shape[2], float(perr.max()) if perr.size else 0.))
    for row, name in enumerate(("x", "y", "logit")):
        bad = np.argwhere(got[:, row] != ref[:, row])
        assert not len(bad), (what, name, bad[:5].tolist())
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=0)


# --------------------------------------------------------------------------- #
# 1. the kernel                                                                #
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def _golden_views(g, key):
    ts, tm, am = (int(x) for x in g["test_cfg"])
    return kar.views(ts, tm, dict(H_FLIP=True, SCALE_H_FLIP=True, MAX_SIZE=am,
                                  SCALES=tuple(int(s) for s in g[key])))


@pytest.mark.parametrize("name,key,heur,dep", [
    ("combined_HM_AVG_all", "aug_scales", "HM_AVG", False),
    ("combined_HM_AVG_dep", "aug_scales", "HM_AVG", True),
    ("combined_HM_MAX_all", "aug_scales", "HM_MAX", False),
    ("combined_HM_MAX_dep", "aug_scales", "HM_MAX", True),
    ("combined_HM_AVG_dep8", "aug_scales_8", "HM_AVG", True),
    ("combined_HM_MAX_dep8", "aug_scales_8", "HM_MAX", True)])
def test_golden_through_the_kernel(g, name, key, heur, dep):
    from vosdetectron_amd import ops
    v, ds, us = _golden_views(g, key)
    views = [_t(m) for m in g["view_heatmaps"][:len(v)]]
    keyps, comb = ops.heatmaps_to_keypoints_aug(
        views, [x[2] for x in v], ds, us, _t(g["boxes"]), 0, heur,
        float(g["area_th"]) if dep else None, want_combined=True)
    assert comb.dtype == torch.float32 and np.array_equal(comb.cpu().numpy(), g[name])
    _assert_decode(keyps, kref.heatmaps_to_keypoints(g[name], g["boxes"]), name)


def test_flip_heatmaps_is_the_references(g):
    from vosdetectron_amd import keypoints
    one = g["view_heatmaps"][0]
    got = keypoints.flip_heatmaps(one)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got, g["flipped_view0"])
    t = keypoints.flip_heatmaps(_t(one))
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), g["flipped_view0"])
    with pytest.raises(ValueError, match="heatmaps"):
        keypoints.flip_heatmaps(one[:, :5])


# one under 1 px (min_size path), one wider than 64 px and one wider than 128 px (two and
# three column strips), one tall, one small fractional; areas on both sides of 900
BOXES56 = np.asarray([(10.3, 20.7, 10.9, 21.2), (5, 6, 75.5, 31), (0, 0, 140.25, 20),
                      (33, 2, 40, 215.5), (12.25, 40.5, 30.75, 61.25)], f32)


@pytest.fixture(scope="module")
def maps56():
    rng = np.random.default_rng(31)
    return [_t((rng.standard_normal((5, 17, 56, 56)) * 3).astype(f32)) for _ in range(6)]


@pytest.mark.parametrize("V", [1, 2, 6])
@pytest.mark.parametrize("heur,area_th", [("HM_AVG", None), ("HM_AVG", 900.), ("HM_MAX", 900.)])
def test_fused_equals_two_step(maps56, V, heur, area_th):
    from vosdetectron_amd import ops
    hf = [False, True, False, True, False, True][:V]
    ds = [False, False, True, True, False, False][:V]
    us = [False, False, False, False, True, True][:V]
    boxes = _t(BOXES56)
    for min_size in (0, 3):
        keyps, comb = ops.heatmaps_to_keypoints_aug(maps56[:V], hf, ds, us, boxes, min_size,
                                                    heur, area_th, want_combined=True)
        two = ops.heatmaps_to_keypoints(comb, boxes, min_size)
        assert torch.equal(keyps, two), (V, heur, area_th, min_size)
        # without combined_out the decode is the same
        assert torch.equal(ops.heatmaps_to_keypoints_aug(maps56[:V], hf, ds, us, boxes,
                                                         min_size, heur, area_th), keyps)
    if V == 1:  # one unflipped view: the plain decode of the view itself, and its maps
        assert torch.equal(comb, maps56[0])
        assert torch.equal(keyps, ops.heatmaps_to_keypoints(maps56[0], boxes, 3))
    if V == 6 and area_th is not None:  # both box classes occur, so the rows differ in T
        area = kar.boxes_area(BOXES56)
        assert (area < 900).any() and (area >= 900).any()


@pytest.mark.parametrize("K", [17, 5])
@pytest.mark.parametrize("heur", ["HM_AVG", "HM_MAX"])
@pytest.mark.parametrize("dep", [False, True])
def test_against_restatement_odd_side(K, heur, dep):
    """M = 7 (odd: the reversed column of the centre is itself), K = 17 with the default
    permutation and K = 5 with an explicit one; 8 views, two below and one above, so the
    rows' divisors are 4, 6 and -- without size dependence -- 8."""
    from vosdetectron_amd import ops
    rng = np.random.default_rng(100 + K)
    M, R, V = 7, 9, 8
    maps = [(rng.standard_normal((R, K, M, M)) * 3).astype(f32) for _ in range(V)]
    maps[1][0, :, 2, 3] = -0.0
    hf = [False, True] * 4
    ds = [False, False, True, True, True, True, False, False]
    us = [False] * 6 + [True, True]
    xy = rng.uniform(0, 200, (R, 2))
    wh = rng.uniform(0.5, 90, (R, 2))
    boxes = np.hstack([xy, xy + wh]).astype(f32)
    boxes[0] = (3, 4, 32, 33)  # 30 x 30 = 900 = the threshold: large
    perm = None if K == 17 else [3, 4, 2, 0, 1]
    th = 900. if dep else None
    keyps, comb = ops.heatmaps_to_keypoints_aug([_t(m) for m in maps], hf, ds, us, _t(boxes), 2,
                                                heur, th, flip_perm=perm, want_combined=True)
    want, t_row = kar.combine(maps, hf, heur, ds, us, boxes, th, perm=perm)
    if dep:
        assert t_row[0] == 6 and set(t_row.tolist()) == {4, 6}
    assert np.array_equal(comb.cpu().numpy(), want)
    _assert_decode(keyps, kref.heatmaps_to_keypoints(want, boxes, 2), "M=7 K=%d" % K)


def test_python_argument_errors():
    from vosdetectron_amd import ops
    m = torch.zeros(2, 5, 7, 7, device=DEV)
    b = torch.zeros(2, 4, device=DEV)
    ok = dict(hflips=[False, True], ds=[False, False], us=[False, True], boxes=b)
    with pytest.raises(ValueError, match="flip_perm"):  # K != 17 needs a permutation
        ops.heatmaps_to_keypoints_aug([m, m], **ok)
    perm = [0, 2, 1, 4, 3]
    ops.heatmaps_to_keypoints_aug([m, m], flip_perm=perm, **ok)
    for bad in ([0, 2, 1, 4], [0, 2, 1, 4, 5], [0, 2, 1, 4, -1]):
        with pytest.raises(ValueError, match="flip_perm"):
            ops.heatmaps_to_keypoints_aug([m, m], flip_perm=bad, **ok)
    with pytest.raises(ValueError, match="views"):
        ops.heatmaps_to_keypoints_aug([m] * 33, [False] * 33, [False] * 33, [False] * 33, b,
                                      flip_perm=perm)
    with pytest.raises(ValueError, match="views"):
        ops.heatmaps_to_keypoints_aug([], [], [], [], b, flip_perm=perm)
    with pytest.raises(ValueError, match="identity"):
        ops.heatmaps_to_keypoints_aug([m, m], [False, False], [True, False], [False, False], b,
                                      flip_perm=perm)
    with pytest.raises(ValueError, match="identity"):
        ops.heatmaps_to_keypoints_aug([m, m], [False, False], [False, True], [False, True], b,
                                      flip_perm=perm)
    with pytest.raises(ValueError, match="heur"):
        ops.heatmaps_to_keypoints_aug([m, m], heur="HM_MEDIAN", flip_perm=perm, **ok)
    with pytest.raises(ValueError, match="area_th"):
        ops.heatmaps_to_keypoints_aug([m, m], area_th=0.1, flip_perm=perm, **ok)
    with pytest.raises(ValueError, match="hflips"):
        ops.heatmaps_to_keypoints_aug([m, m], [False], [False, False], [False, False], b,
                                      flip_perm=perm)
    with pytest.raises(ValueError, match=r"views\[1\]"):
        ops.heatmaps_to_keypoints_aug([m, m[:1]], flip_perm=perm, **ok)


def test_c_argument_errors_leave_out_untouched():
    """Every refusal of the C entry returns its code before anything is launched."""
    from vosdetectron_amd import _lib
    lib = _lib.lib()
    R, K, M = 2, 5, 7
    maps = torch.randn(R, K, M, M, device=DEV)
    boxes = torch.tensor([[0, 0, 10, 10], [5, 5, 50, 40]], dtype=torch.float32, device=DEV)
    out = torch.full((R, 4, K), -7.0, device=DEV)
    comb = torch.full((R, K, M, M), -7.0, device=DEV)

    def call(V=2, hf=0b10, ds=0, us=0b10, perm=(0, 2, 1, 4, 3), heur=0, th=-1.0, R=R, K=K, M=M,
             stride=4, min_size=0, views=None, nperm=True):
        ptrs = (ctypes.c_void_p * 32)(*([maps.data_ptr()] * 32 if views is None else views))
        p = (ctypes.c_int32 * 32)(*perm)
        return lib.vd_heatmaps_to_keypoints_aug(
            ptrs, V, hf, ds, us, p if nperm else None, heur, th, R, K, M, boxes.data_ptr(),
            stride, min_size, comb.data_ptr(), out.data_ptr(), None)

    ARG = _lib.VD_ERR_ARG
    cases = dict(
        v0=dict(V=0), v33=dict(V=33), hflip_bit_past_v=dict(hf=0b100), ds_bit_past_v=dict(ds=0b100),
        ds_identity=dict(ds=0b01, us=0), us_identity=dict(us=0b01), ds_and_us=dict(ds=0b10),
        perm_high=dict(perm=(0, 2, 1, 4, 5)), perm_negative=dict(perm=(0, 2, 1, -1, 3)),
        perm_null=dict(nperm=False), heur=dict(heur=2), heur_negative=dict(heur=-1),
        area_nan=dict(th=float("nan")), m0=dict(M=0), m65=dict(M=65), k0=dict(K=0),
        k33=dict(K=33), r_negative=dict(R=-1), stride=dict(stride=3), min_size=dict(min_size=-1),
        null_view=dict(views=[maps.data_ptr(), None] + [maps.data_ptr()] * 30))
    for name, kw in cases.items():
        assert call(**kw) == ARG, name
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((comb == -7.0).all())
    # a bad view list is refused even when there is nothing to do; a good one with R = 0
    # launches nothing
    assert call(R=0, V=0) == ARG
    assert call(R=0) == _lib.VD_OK
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((comb == -7.0).all())
    # and the same arguments unspoiled run
    assert call() == _lib.VD_OK
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any()) and not bool((comb == -7.0).any())


def test_zero_rows():
    from vosdetectron_amd import ops
    m = torch.zeros(0, 17, 56, 56, device=DEV)
    keyps, comb = ops.heatmaps_to_keypoints_aug([m, m], [False, True], [False, False],
                                                [False, False], torch.zeros(0, 4, device=DEV),
                                                want_combined=True)
    assert keyps.shape == (0, 4, 17) and comb.shape == (0, 17, 56, 56)


# --------------------------------------------------------------------------- #
# 2. the pipeline                                                              #
# --------------------------------------------------------------------------- #
FRAME_HW = (320, 480)
AUG = dict(ENABLED=True, H_FLIP=True, SCALES=(224, 416), MAX_SIZE=640, SCALE_H_FLIP=True)
KW = dict(frame_hw=FRAME_HW, batch=2, channels_last=True, device=DEV)


def _cfg(kps=True, box=False, classes=None, **kps_more):
    from vosdetectron_amd import config as vcfg
    cfg = vcfg.get(NAME)
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = FRAME_HW
    if classes:
        cfg.MODEL.NUM_CLASSES = classes
    if kps:
        cfg.TEST.KPS_AUG.update(AUG)
        cfg.TEST.KPS_AUG.update(kps_more)
    if box:
        cfg.TEST.BBOX_AUG.update(AUG)
    vcfg.check_supported(cfg, test_aug=True)
    return cfg


@pytest.fixture(scope="module")
def world():
    """The seed-0 model and the two frames, shared by every pipeline below."""
    import bench
    from vosdetectron_amd.weights import build_model
    model, sd = build_model(_cfg(kps=False), seed=0, device=DEV, channels_last=True)
    frames = torch.from_numpy(bench.synthetic_frames(2, 21, *FRAME_HW)).to(DEV)
    return model, sd, frames


@pytest.fixture(scope="module", params=[False, True], ids=["bbox_aug_off", "bbox_aug_on"])
def step(request, world):
    from vosdetectron_amd.engine import KeypointAugFramePipeline
    model, sd, frames = world
    cfg = _cfg(box=request.param)
    pipe = KeypointAugFramePipeline(model, cfg, cand_cap=4096, **KW)
    # warm-up step: the views' convolution shapes are not in the shipped MIOpen Find db,
    # so their first run searches, and the solver it runs may differ from the one found
    pipe.run(frames)
    out = pipe.run(frames, keep_intermediates=True)
    torch.cuda.synchronize()
    return cfg, pipe, out


def _rows(out, key="dets"):
    ks = out["counts_host"]
    return torch.cat([out[key][f, :k] for f, k in enumerate(ks)])


def _restated(pipe, out, area_th=None):
    hm = [out["views"][v]["kps_heatmaps"].cpu().numpy() for v in pipe.kps_views]
    return kar.combine(hm, [v[2] for v in pipe.kps_views], pipe.kps_heur, pipe.kps_ds,
                       pipe.kps_us, out["kps_boxes"].cpu().numpy(), area_th)


def test_pipeline_views_and_rois(step):
    from vosdetectron_amd import ops
    cfg, pipe, out = step
    ks = out["counts_host"]
    M = sum(ks)
    assert max(ks) > 0 and len(pipe.kps_views) == 6
    assert pipe.kps_views[0] == FRAME_HW + (False,) and pipe.kps_views[1] == FRAME_HW + (True,)
    assert len(pipe.box_views) == (6 if cfg.TEST.BBOX_AUG.ENABLED else 1)
    dets = _rows(out)
    assert torch.equal(out["kps_boxes"], dets[:, :4])
    d = out["dets"].cpu().numpy()
    flipped = d.copy()
    flipped[..., :4] = aug_ref.flip_boxes(d[..., :4].reshape(-1, 4), FRAME_HW[1]).reshape(
        d.shape[0], -1, 4)
    for v in pipe.kps_views:
        vd = out["views"][v]
        assert tuple(vd["kps_heatmaps"].shape) == (M, 17, 56, 56)
        assert tuple(vd["kps_feat"].shape) == (M, 256, 14, 14)
        want = ops.mask_rois(_t(flipped if v[2] else d), out["classes"], out["counts"],
                             pipe.geom[v].im_scale_d, pipe.mask_rows(2), cfg.FPN.ROI_MIN_LEVEL,
                             cfg.FPN.ROI_MAX_LEVEL)[0][:M]
        assert torch.equal(vd["kps_rois"], want), v
        box = (flipped if v[2] else d)
        rows = np.concatenate([box[f, :k, :4] for f, k in enumerate(ks)])
        np.testing.assert_allclose(vd["kps_rois"][:, 1:].cpu().numpy(),
                                   rows * pipe.geom[v].scale, rtol=1e-6)
    assert torch.equal(out["kps_rois"], out["views"][pipe.kps_views[0]]["kps_rois"])
    assert torch.equal(out["kps_feat"], out["views"][pipe.kps_views[0]]["kps_feat"])


def test_pipeline_view_heatmaps_vs_fp64(step, world):
    """Two rows of every view (the first and the last detection) through the float64
    restatement of the head on the view's own RoI features; the yardstick is torch's
    float32 error on the same chain, 4x allowed, as tests/test_keypoints_gpu.py's."""
    cfg, pipe, out = step
    model, sd, frames = world
    M = sum(out["counts_host"])
    pick = [0, M - 1]
    x = torch.cat([out["views"][v]["kps_feat"][pick] for v in pipe.kps_views]).cpu()
    got = torch.cat([out["views"][v]["kps_heatmaps"][pick] for v in pipe.kps_views])
    ref = kref.keypoint_head_outputs(sd, x, cfg, torch.float64)
    t32 = kref.keypoint_head_outputs(sd, x, cfg, torch.float32)
    scale = float(ref.abs().max())
    e, te = (got.double().cpu() - ref).abs() / scale, (t32.double() - ref).abs() / scale
    print("view heatmaps vs fp64: max %.3g mean %.3g of range; torch fp32: max %.3g mean %.3g"
          % (e.max(), e.mean(), te.max(), te.mean()))
    assert float(e.max()) <= 4 * float(te.max()) and float(e.mean()) <= 4 * float(te.mean())


def test_pipeline_combination_and_decode(step):
    cfg, pipe, out = step
    want, t_row = _restated(pipe, out)
    assert set(t_row.tolist()) == {6}
    assert np.array_equal(out["kps_heatmaps"].cpu().numpy(), want)
    # the views differ, and the flipped ones are stored as the network returned them
    hm = [out["views"][v]["kps_heatmaps"] for v in pipe.kps_views]
    assert not torch.equal(hm[0], hm[1]) and not torch.equal(out["kps_heatmaps"], hm[0])
    ref = kref.heatmaps_to_keypoints(want, out["kps_boxes"].cpu().numpy(),
                                     cfg.KRCNN.INFERENCE_MIN_SIZE)
    _assert_decode(out["keyps"], ref, "pipeline")
    assert tuple(out["keyps"].shape) == (sum(out["counts_host"]), 4, 17)


@pytest.mark.parametrize("heur", ["HM_AVG", "HM_MAX"])
def test_pipeline_size_dependent(step, world, heur):
    """SCALE_SIZE_DEP with AREA_TH one of the step's own box areas (a float32, so exact):
    the box at the median and every larger one drop the upscaled views, the rest the
    downscaled ones."""
    from vosdetectron_amd.engine import KeypointAugFramePipeline
    cfg0, pipe0, out0 = step
    model, sd, frames = world
    area = np.sort(kar.boxes_area(out0["kps_boxes"].cpu().numpy()))
    th = float(area[len(area) // 2])
    cfg = _cfg(box=bool(cfg0.TEST.BBOX_AUG.ENABLED), SCALE_SIZE_DEP=True, AREA_TH=th, HEUR=heur)
    pipe = KeypointAugFramePipeline(model, cfg, cand_cap=4096, **KW)
    out = pipe.run(frames, keep_intermediates=True)
    area = kar.boxes_area(out["kps_boxes"].cpu().numpy())
    print("AREA_TH %.9g: %d boxes below, %d at or above" % (th, (area < th).sum(),
                                                           (area >= th).sum()))
    if not ((area < th).any() and (area >= th).any()):
        pytest.skip("the step's detections do not fall on both sides of their median area: %s"
                    % np.sort(area))
    want, t_row = _restated(pipe, out, th)
    assert set(t_row.tolist()) == {4} and pipe.kps_area_th == th
    assert np.array_equal(out["kps_heatmaps"].cpu().numpy(), want)
    assert not np.array_equal(want, _restated(pipe, out)[0])
    ref = kref.heatmaps_to_keypoints(want, out["kps_boxes"].cpu().numpy(),
                                     cfg.KRCNN.INFERENCE_MIN_SIZE)
    _assert_decode(out["keyps"], ref, "size-dependent " + heur)


def test_both_augmentations_off_is_the_plain_pipeline(world):
    from vosdetectron_amd.engine import KeypointAugFramePipeline, KeypointFramePipeline
    model, sd, frames = world
    cfg = _cfg(kps=False)
    plain = KeypointFramePipeline(model, cfg, **KW).run(frames, keep_intermediates=True)
    out = KeypointAugFramePipeline(model, cfg, **KW).run(frames, keep_intermediates=True)
    assert out["counts_host"] == plain["counts_host"] and sum(plain["counts_host"]) > 0
    for k in ("dets", "classes", "counts", "rois", "cls_prob", "bbox_pred", "keyps", "kps_rois",
              "kps_heatmaps", "kps_feat", "kps_boxes", "kps_total"):
        assert torch.equal(out[k], plain[k]), k


def test_async_then_complete_equals_sync(step, world):
    cfg, pipe, eager = step
    model, sd, frames = world
    out = pipe.run(frames, sync=False)
    assert "counts_host" not in out and out["keyps"].shape[0] == pipe.mask_rows(2)
    pipe.complete(out)
    assert out["counts_host"] == eager["counts_host"] and "_pyrs" not in out
    for k in ("dets", "classes", "counts", "kps_rois", "keyps"):
        assert torch.equal(out[k], eager[k]), k
    assert pipe.complete(out) is out  # idempotent


def test_stage_marks_and_frame_keypoints(step, world):
    from vosdetectron_amd.engine import frame_keypoints
    cfg, pipe, eager = step
    model, sd, frames = world
    pipe.enable_timers()
    try:
        pipe.run(frames)
        marks = set(pipe.timer_summary())
    finally:
        pipe.enable_timers(False)
    want = {"conv_body", "misc_bbox", "im_detect_keypoints", "misc_keypoints"}
    if cfg.TEST.BBOX_AUG.ENABLED:
        want.add("union_add_view")
    assert want <= marks and "misc_oks_nms" not in marks, marks
    res = frame_keypoints(pipe, eager)
    ks = eager["counts_host"]
    kp = eager["keyps"].cpu().numpy()
    assert [len(r[1]) for r in res] == ks and np.array_equal(res[1][1][0], kp[ks[0]])


def test_graph_replay_equals_eager(step, world):
    cfg, pipe, eager = step
    model, sd, frames = world
    x = frames.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pipe.run(x, sync=False)  # warm on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        gout = pipe.run(x, sync=False)
    torch.cuda.synchronize()
    assert "counts_host" not in gout  # no host read inside the captured step
    for _ in range(2):
        for k in ("keyps", "dets", "counts"):
            gout[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        out = pipe.complete(dict(gout))
        assert out["counts_host"] == eager["counts_host"]
        for k in ("dets", "classes", "counts", "kps_rois", "keyps"):
            assert torch.equal(out[k], eager[k]), k


def test_row_ranges_give_identical_tensors(step, world):
    """The helper complete() uses for rows past the padded batch: one range and two."""
    cfg, pipe, eager = step
    model, sd, frames = world
    out = pipe.run(frames, sync=False)
    rows = pipe.mask_rows(2)
    assert rows % 128 == 0
    k_all, more_all, total = pipe._keypoints(out, out, rows, 0)
    a = pipe._keypoints(out, out, rows // 2, 0)
    b = pipe._keypoints(out, out, rows // 2, rows // 2)
    M = int(total.item())
    assert M == sum(eager["counts_host"]) and M > 1
    assert torch.equal(torch.cat([a[0], b[0]]), k_all)
    for k in ("kps_rois", "kps_feat", "kps_boxes"):
        assert torch.equal(torch.cat([a[1][k], b[1][k]]), more_all[k]), k
    assert torch.equal(k_all, out["keyps"]) and torch.equal(k_all[:M], eager["keyps"])
    # a range that starts inside the real rows: the overflow batch's shape
    c = pipe._keypoints(out, out, 64, M - 1)
    assert torch.equal(c[0][:1], eager["keyps"][M - 1:])
    pipe.complete(out)


def test_complete_runs_the_rows_past_the_padded_batch(step, world, monkeypatch):
    """A padded batch shorter than the detections: complete() sends the rest through
    every view again, and the per-view intermediates grow with them."""
    cfg, pipe, eager = step
    model, sd, frames = world
    M = sum(eager["counts_host"])
    cap = 64 if M > 64 else M // 2
    assert 0 < cap < M
    monkeypatch.setattr(pipe, "mask_rows", lambda F: cap)
    out = pipe.run(frames, keep_intermediates=True, sync=False)
    assert out["keyps"].shape[0] == cap and "_pyrs" in out
    pipe.complete(out)
    assert "_pyrs" not in out and out["counts_host"] == eager["counts_host"]
    for k in ("dets", "classes", "counts", "kps_rois", "kps_feat", "kps_boxes", "kps_heatmaps",
              "keyps"):
        assert out[k].shape == eager[k].shape, k
    for k in ("dets", "classes", "counts", "kps_rois", "kps_feat", "kps_boxes"):
        assert torch.equal(out[k], eager[k]), k
    for v in pipe.kps_views:
        for k in ("kps_rois", "kps_feat"):
            assert torch.equal(out["views"][v][k], eager["views"][v][k]), (v, k)
        assert out["views"][v]["kps_heatmaps"].shape == eager["views"][v]["kps_heatmaps"].shape
    # the combination and the decode hold on this run's own heatmaps
    want, _ = _restated(pipe, out)
    assert np.array_equal(out["kps_heatmaps"].cpu().numpy(), want)
    # the head's deconvolution may pick another algorithm for another batch size
    assert float((out["kps_heatmaps"] - eager["kps_heatmaps"]).abs().max()) <= 1e-4


def test_nms_oks_on_the_augmented_step(world):
    """Person as the only class: the outputs are ops.nms_oks_frames of the pre-NMS rows."""
    from vosdetectron_amd import ops
    from vosdetectron_amd.engine import KeypointAugFramePipeline
    from vosdetectron_amd.weights import build_model
    _, _, frames = world
    cfg = _cfg(classes=2)
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True)
    pipe = KeypointAugFramePipeline(model, cfg, nms_oks=True, **KW)
    pipe.run(frames)
    out = pipe.run(frames, keep_intermediates=True)
    pre = out["counts_pre_oks_host"]
    assert sum(pre) > 0 and pipe.oks_thresh == 0.3
    want, _ = _restated(pipe, out)
    assert np.array_equal(out["kps_heatmaps"].cpu().numpy(), want)
    padded = torch.zeros((pipe.mask_rows(2), 4, 17), device=DEV)
    padded[:sum(pre)] = out["keyps_pre_oks"]
    res = ops.nms_oks_frames(padded, out["dets_pre_oks"], out["classes_pre_oks"],
                             out["counts_pre_oks"], 0.3)
    assert out["counts_host"] == res.counts.cpu().tolist()
    assert torch.equal(out["dets"], res.dets) and torch.equal(out["classes"], res.classes)
    assert torch.equal(out["oks_keep"], res.keep)
    assert torch.equal(out["keyps"], res.keyps[:sum(out["counts_host"])])
    with pytest.raises(ValueError, match="NUM_CLASSES"):
        KeypointAugFramePipeline(world[0], _cfg(), nms_oks=True, **KW)


def test_refusals(world):
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import (AugFramePipeline, FramePipeline,
                                         KeypointAugFramePipeline, KeypointFramePipeline)
    model, sd, frames = world
    for cfg in (_cfg(), _cfg(kps=False, box=True), _cfg(box=True)):
        with pytest.raises(NotImplementedError, match="KeypointAugFramePipeline"):
            KeypointFramePipeline(model, cfg, **KW)
        with pytest.raises(NotImplementedError, match="KEYPOINTS_ON"):
            FramePipeline(model, cfg, **KW)
    with pytest.raises(NotImplementedError, match="FPN mask configs only") as e:
        AugFramePipeline(model, _cfg(), **KW)
    assert "KeypointAugFramePipeline" in str(e.value) and "not built" in str(e.value)
    with pytest.raises(ValueError, match="KEYPOINTS_ON"):
        KeypointAugFramePipeline(model, vcfg.get("e2e_mask_rcnn_R-50-FPN_1x"), **KW)
    # the heatmap budget: 6 views x 256 rows x (17 x 56 x 56 x 4 = 213248) bytes
    need = 6 * 256 * 213248
    KeypointAugFramePipeline(model, _cfg(), heatmap_budget_bytes=need, **KW)
    with pytest.raises(ValueError, match=r"6 views x 256 rows x .*213248.*= %d" % need):
        KeypointAugFramePipeline(model, _cfg(), heatmap_budget_bytes=need - 1, **KW)
    with pytest.raises(ValueError, match="pyramid_budget_bytes"):
        KeypointAugFramePipeline(model, _cfg(), pyramid_budget_bytes=1 << 20, **KW)
    with pytest.raises(ValueError, match="twice"):
        KeypointAugFramePipeline(model, _cfg(SCALES=(224, 224)), **KW)
