"""Aspect-ratio views of the test-time augmentation on the device:
vd_image_aspect_resize_to_blob against the numpy restatement (tests/aspect_ref.py),
vd_box_union_add_view_ar, the heads' RoIs and the mask combination against the executed
reference (tests/golden/tta_ar.npz, tools/gen_tta_ar_goldens.py), and AugFramePipeline /
KeypointAugFramePipeline with aspect-ratio views, stage-wise on the step's own tensors.
Reference: lib/core/test.py:243-253, 330-363, 448-456, 509-526, 618-628, 684-702."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aspect_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDE = 32
GUARD = 1024  # floats of NaN on either side of the blob


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frames(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _lut():
    from vosdetectron_amd import ops
    return _t(ops.pixel_lut(tuple(orc.PIXEL_MEANS.reshape(-1))))


# --------------------------------------------------------------------------- #
# 1. the blob                                                                  #
# --------------------------------------------------------------------------- #
def _blob_in_guards(frames, ar, hflip, scale, Hp, Wp, nhwc):
    """The op writing into the middle of a NaN-filled buffer -> (blob, the buffer)."""
    from vosdetectron_amd import ops
    F = frames.shape[0]
    shape = (F, Hp, Wp, 3) if nhwc else (F, 3, Hp, Wp)
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + n].view(shape)
    got = ops.image_aspect_resize_to_blob(_t(frames), _lut(), ar, scale, Hp, Wp, hflip=hflip,
                                          nhwc=nhwc, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out, buf


def _check_blob(frames, ar, hflip, target, max_size):
    H, W = frames.shape[1:3]
    ref, scale = aspect_ref.view_blob(frames, ar, hflip, target, max_size, STRIDE)
    Hp, Wp = ref.shape[2:]
    War = aspect_ref.aspect_width(W, ar)
    Hr, Wr = int(round(H * scale)), int(round(War * scale))
    assert not ref[:, :, Hr:].any() and not ref[:, :, :, Wr:].any()
    for nhwc in (False, True):
        out, buf = _blob_in_guards(frames, ar, hflip, scale, Hp, Wp, nhwc)
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
        got = out.permute(0, 3, 1, 2) if nhwc else out
        got = got.cpu().numpy()
        assert not np.isnan(got).any()  # every element written
        assert not got[:, :, Hr:].any() and not got[:, :, :, Wr:].any()  # the padding is zero
        bad = np.argwhere(got != ref)
        assert not len(bad), (ar, hflip, target, nhwc, len(bad), bad[:4].tolist())
    return scale


@pytest.mark.parametrize("hflip", [False, True], ids=["plain", "hflip"])
@pytest.mark.parametrize("ar", [0.5, 0.75, 1.37, 2.0])
def test_blob_equals_restatement(ar, hflip):
    """2 frames of 37 x 53 (odd sizes, no multiple of the stride): an upscaling and a
    downscaling TEST.SCALE, NCHW and NHWC, bit for bit; padding zero, guards untouched."""
    frames = _frames(2, 37, 53, 100)
    up = _check_blob(frames, ar, hflip, 48, 160)
    down = _check_blob(frames, ar, hflip, 20, 160)
    assert up > 1.0 > down and down != 0.5


@pytest.mark.parametrize("hflip", [False, True], ids=["plain", "hflip"])
def test_blob_area_path(hflip):
    """48 x 40 at ar 2.0 and TEST.SCALE 24: im_ar is 48 x 80 and im_scale exactly 0.5, the
    2 x 2 area path on synthesised bytes."""
    frames = _frames(1, 48, 40, 101)
    assert _check_blob(frames, 2.0, hflip, 24, 1333) == 0.5


@pytest.mark.parametrize("scale_to", [37, 48, 20])
def test_ratio_one_is_the_existing_op(scale_to):
    """ar = 1.0: stage 1 is the identity (coefficients 2048 / 0), so the op is
    vd_image_resize_to_blob; flipped, that op on frames.flip(2)."""
    from vosdetectron_amd import ops
    frames = _t(_frames(2, 37, 53, 102))
    scale = ops.target_scale(37, 53, scale_to, 160)
    Hr, Wr = ops.resized_hw(37, 53, scale)
    Hp, Wp = -(-Hr // STRIDE) * STRIDE, -(-Wr // STRIDE) * STRIDE
    lut = _lut()
    for nhwc in (False, True):
        want = ops.image_resize_to_blob(frames, lut, scale, Hp, Wp, nhwc=nhwc)
        got = ops.image_aspect_resize_to_blob(frames, lut, 1.0, scale, Hp, Wp, nhwc=nhwc)
        assert torch.equal(got, want)
        want = ops.image_resize_to_blob(frames.flip(2).contiguous(), lut, scale, Hp, Wp,
                                        nhwc=nhwc)
        got = ops.image_aspect_resize_to_blob(frames, lut, 1.0, scale, Hp, Wp, hflip=True,
                                              nhwc=nhwc)
        assert torch.equal(got, want)


def test_blob_python_argument_errors():
    from vosdetectron_amd import ops
    frames = _t(_frames(1, 37, 53, 103))
    with pytest.raises(ValueError, match="smaller"):
        ops.image_aspect_resize_to_blob(frames, _lut(), 2.0, 1.0, 64, 96)  # War = 106 > 96
    with pytest.raises(ValueError, match="no column"):
        ops.image_aspect_resize_to_blob(frames, _lut(), 0.001, 1.0, 64, 64)


# --------------------------------------------------------------------------- #
# 2. the executed reference through the kernels                                #
# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "tta_ar.npz"))


def _golden_union(g):
    from vosdetectron_amd import ops
    T, Rg, Kg = g["view_scores"].shape
    H, W = g["im"].shape[:2]
    u = ops.BoxUnion(T * Rg, 1, Kg, DEV)
    cnt = torch.tensor([Rg], dtype=torch.int32, device=DEV)
    for t, (_, _, hf, ar) in enumerate(g["bbox_calls"].tolist()):
        Wv = aspect_ref.aspect_width(W, ar) if ar else W
        assert [H, Wv] == g["bbox_im_shapes"][t].tolist()
        u.add_view(_t(g["view_rois"][t][None]), _t(g["view_scores"][t][None]),
                   _t(g["view_deltas"][t][None]), cnt,
                   torch.tensor([g["view_im_scale"][t]], dtype=torch.float32, device=DEV),
                   torch.tensor([[H, Wv]], dtype=torch.int32, device=DEV), bool(hf),
                   score_thresh=g["test_cfg"][0], bbox_reg_weights=tuple(g["weights"]),
                   x_inv=np.float32(1.0 / ar) if ar else None)
    return u


def test_golden_lists_through_add_view(gold):
    """add_view x 7 with score_thresh 0 keeps every row: the lists are boxes_c / scores_c
    of the reference's np.vstack, class by class, bit for bit."""
    from vosdetectron_amd import ops
    g = gold
    T, Rg, Kg = g["view_scores"].shape
    H, W = g["im"].shape[:2]
    u = ops.BoxUnion(T * Rg, 1, Kg, DEV)
    cnt = torch.tensor([Rg], dtype=torch.int32, device=DEV)
    for t, (_, _, hf, ar) in enumerate(g["bbox_calls"].tolist()):
        Wv = aspect_ref.aspect_width(W, ar) if ar else W
        u.add_view(_t(g["view_rois"][t][None]), _t(g["view_scores"][t][None]),
                   _t(g["view_deltas"][t][None]), cnt,
                   torch.tensor([g["view_im_scale"][t]], dtype=torch.float32, device=DEV),
                   torch.tensor([[H, Wv]], dtype=torch.int32, device=DEV), bool(hf),
                   score_thresh=0.0, bbox_reg_weights=tuple(g["weights"]),
                   x_inv=np.float32(1.0 / ar) if ar else None)
    torch.cuda.synchronize()
    cap = T * Rg
    # the workspace's first region: per (image, class) five planes of cand_cap floats
    cand = u.ws[:Kg * 5 * cap * 4].view(torch.float32).view(Kg, 5, cap).cpu().numpy()
    for j in range(1, Kg):
        assert np.array_equal(cand[j, :4].T, g["boxes_c"][:, 4 * j:4 * j + 4]), j
        assert np.array_equal(cand[j, 4], g["scores_c"][:, j]), j


@pytest.mark.parametrize("vote", ["plain", "vote"])
def test_golden_union_detections(gold, vote):
    g = gold
    thr, nms, per_im = g["test_cfg"]
    u = _golden_union(g)
    kw = dict(bbox_vote="AVG", bbox_vote_thresh=float(g["vote_cfg"][0])) if vote == "vote" else {}
    dets, dcls, dcnt = u.detections(nms, int(per_im), det_cap=64, **kw)
    want = g["det_%s_dets" % vote]
    n = int(dcnt[0].item())
    assert n == len(want) == int(per_im)
    assert np.array_equal(dets[0, :n].cpu().numpy(), want)
    assert np.array_equal(dcls[0, :n].cpu().numpy(), g["det_%s_cls" % vote])


@pytest.mark.parametrize("vote", ["plain", "vote"])
def test_old_entry_unchanged_on_tta_golden(vote):
    """vd_box_union_add_view (no x_inv) on tests/golden/tta.npz: the results it had."""
    from vosdetectron_amd import ops
    g = np.load(os.path.join(GOLDEN, "tta.npz"))
    T6, Rg, Kg = g["view_scores"].shape
    H, W = g["im"].shape[:2]
    thr, nms, per_im = g["test_cfg"]
    hw = torch.tensor([[H, W]], dtype=torch.int32, device=DEV)
    res = []
    for x_inv in (None, 1.0):  # ... and the new entry at x_inv = 1 is the old one
        u = ops.BoxUnion(T6 * Rg, 1, Kg, DEV)
        for t in range(T6):
            u.add_view(_t(g["view_rois"][t][None]), _t(g["view_scores"][t][None]),
                       _t(g["view_deltas"][t][None]),
                       torch.tensor([Rg], dtype=torch.int32, device=DEV),
                       torch.tensor([g["view_im_scale"][t]], dtype=torch.float32, device=DEV),
                       hw, bool(g["bbox_calls"][t][2]), score_thresh=thr,
                       bbox_reg_weights=tuple(g["weights"]), x_inv=x_inv)
        kw = dict(bbox_vote="AVG", bbox_vote_thresh=float(g["vote_cfg"][0])) \
            if vote == "vote" else {}
        dets, dcls, dcnt = u.detections(nms, int(per_im), det_cap=64, **kw)
        n = int(dcnt[0].item())
        assert n == int(per_im)
        assert np.array_equal(dets[0, :n].cpu().numpy(), g["det_%s_dets" % vote])
        assert np.array_equal(dcls[0, :n].cpu().numpy(), g["det_%s_cls" % vote])
        res.append(dets)
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("key,calls", [("mask_boxes", "mask_body_calls"),
                                       ("kps_boxes", "kps_body_calls")])
def test_head_rois_equal_restatement_and_golden(gold, key, calls):
    """engine.view_dets + vd_mask_rois at the view's geometry on the golden's detections:
    the boxes each view's head was handed by the reference, times the view's im_scale."""
    from vosdetectron_amd import engine, ops
    g = gold
    H, W = g["im"].shape[:2]
    dets = g["det_plain_dets"]
    M = len(dets)
    d = _t(dets[None])
    dcls = _t(g["det_plain_cls"][None].astype(np.int32))
    dcnt = torch.tensor([M], dtype=torch.int32, device=DEV)
    rows = [[96.0, 133.0, 0.0, 0.0]] + g[calls][:, :4].tolist()
    scales = g["mask_im_scale" if key == "mask_boxes" else "kps_im_scale"].tolist()
    seen = set()
    for t, (s, ms, hf, ar) in enumerate(rows):
        view = (int(s), int(ms), bool(hf)) + ((ar,) if ar else ())
        geom = engine._ViewGeom(view, H, W, STRIDE, 1, DEV)
        assert geom.scale == scales[t]
        assert geom.im_hw.cpu().tolist() == [[H, aspect_ref.aspect_width(W, ar) if ar else W]]
        vd = engine.view_dets(d, geom)
        assert np.array_equal(vd[0, :, :4].cpu().numpy(), g[key][t]), view
        assert torch.equal(vd[..., 4], d[..., 4]) and torch.equal(vd[..., 1], d[..., 1])
        rois = ops.mask_rois(vd, dcls, dcnt, geom.im_scale_d, 64, 2, 5)[0][:M].cpu().numpy()
        want = aspect_ref.head_rois(
            aspect_ref.head_boxes(dets[:, :4], W, ar or None, bool(hf)), scales[t])
        assert np.array_equal(rois, want), view
        seen.add((bool(ar), bool(hf)))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("heur", ["SOFT_AVG", "SOFT_MAX"])
def test_golden_masks_through_kernels(gold, heur):
    from vosdetectron_amd import ops
    g = gold
    vm = g["view_masks"]
    T, M, Kg, Rm, _ = vm.shape
    flips = [False] + [bool(r[2]) for r in g["mask_body_calls"].tolist()]
    acc = torch.empty((M * Kg, Rm, Rm), dtype=torch.float32, device=DEV)
    for t in range(T):
        ops.mask_aug_accumulate(acc, _t(vm[t].reshape(M * Kg, Rm, Rm)), flips[t], heur,
                                first=t == 0)
    got = ops.mask_aug_finish(acc, T, heur).cpu().numpy().reshape(M, Kg, Rm, Rm)
    assert np.array_equal(got, g["masks_c_" + heur])


# --------------------------------------------------------------------------- #
# 3. AugFramePipeline                                                          #
# --------------------------------------------------------------------------- #
FRAME_HW = (224, 288)
AR = 0.75
AUG = dict(ENABLED=True, H_FLIP=True, ASPECT_RATIOS=(AR,), ASPECT_RATIO_H_FLIP=True)


def _mask_cfg():
    from vosdetectron_amd import config as vcfg
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = 224, 288
    cfg.TEST.BBOX_AUG.update(AUG)
    cfg.TEST.MASK_AUG.update(AUG)
    vcfg.check_supported(cfg, test_aug=True, aspect_views=True)
    with pytest.raises(NotImplementedError, match="ASPECT_RATIOS"):
        vcfg.check_supported(cfg, test_aug=True)
    return cfg


@pytest.fixture(scope="module")
def tta():
    from vosdetectron_amd.engine import AugFramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = _mask_cfg()
    frames = np.stack([np.random.RandomState(1000 + i).randint(0, 256, FRAME_HW + (3,), np.uint8)
                       for i in range(2)])
    model, sd = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=frames[0])
    pipe = AugFramePipeline(model, cfg, frame_hw=FRAME_HW, batch=2, device=DEV,
                            channels_last=True, cand_cap=4096)
    pipe.run(_t(frames))  # warm-up: the views' convolution shapes are searched once
    out = pipe.run(_t(frames), keep_intermediates=True)
    torch.cuda.synchronize()
    return cfg, pipe, frames, out


def test_pipeline_views_and_blobs(tta):
    from vosdetectron_amd import ops
    cfg, pipe, frames, out = tta
    ident, hf = (224, 288, False), (224, 288, True)
    ar, ar_hf = (224, 288, False, AR), (224, 288, True, AR)
    assert pipe.box_views == [hf, ar, ar_hf, ident] and pipe.mask_views == [ident, hf, ar, ar_hf]
    g = pipe.geom[ar]
    War = aspect_ref.aspect_width(FRAME_HW[1], AR)
    assert War == 216 and g.im_hw.cpu().tolist() == [[224, War]] * 2 and g.flip_w == War
    assert g.x_inv == float(np.float32(1.0 / AR)) and pipe.geom[ident].x_inv is None
    assert g.scale == ops.target_scale(224, War, 224, 288)
    for v in (ar, ar_hf):
        gv = pipe.geom[v]
        blob = out["views"][v]["blob"]
        want = ops.image_aspect_resize_to_blob(_t(frames), pipe.lut, AR, gv.scale, gv.Hp, gv.Wp,
                                               hflip=v[2], nhwc=True).permute(0, 3, 1, 2)
        assert torch.equal(blob, want), v
        ref, scale = aspect_ref.view_blob(frames, AR, v[2], 224, 288, STRIDE)
        assert scale == gv.scale and np.array_equal(blob.cpu().numpy(), ref), v
    assert pipe.pyramid_bytes(g) == sum(-(-g.Hp // 2 ** l) * -(-g.Wp // 2 ** l)
                                        for l in pipe.roi_levels) * 256 * 4


def _oracle_union(cfg, pipe, out, f):
    tst, Kc = cfg.TEST, cfg.MODEL.NUM_CLASSES
    scores_ts, boxes_ts = [], []
    for v in pipe.box_views:
        o = out["views"][v]
        n = int(o["roi_counts"][f].item())
        post = o["rois"].shape[1]
        rois = o["rois"][f, :n].cpu().numpy()
        scores_ts.append(o["cls_prob"].view(-1, post, Kc)[f, :n].cpu().numpy())
        dl = o["bbox_pred"].view(-1, post, 4 * Kc)[f, :n].cpu().numpy()
        boxes_ts.append(aspect_ref.decode_view(
            rois, dl, np.float32(pipe.geom[v].scale), FRAME_HW[0], FRAME_HW[1],
            v[3] if len(v) > 3 else None, v[2], tuple(cfg.MODEL.BBOX_REG_WEIGHTS)))
    return orc.box_results_with_nms_and_limit(np.vstack(scores_ts), np.vstack(boxes_ts), Kc,
                                              tst.SCORE_THRESH, tst.NMS, tst.DETECTIONS_PER_IM)


def _check_step(cfg, pipe, out):
    """Detections against the CPU reference on the step's own per-view head outputs; each
    mask view's RoIs against the restatement; the combined masks against the in-order
    combination of the step's own per-view masks."""
    ks = out["counts_host"]
    for f in range(2):
        s_ref, b_ref, cls_boxes = _oracle_union(cfg, pipe, out, f)
        k = ks[f]
        assert k == len(s_ref) and k > 0
        dets = out["dets"][f, :k].cpu().numpy()
        assert np.array_equal(dets[:, :4], b_ref) and np.array_equal(dets[:, 4], s_ref)
        ref_cls = np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, len(cls_boxes))])
        assert np.array_equal(out["classes"][f, :k].cpu().numpy(), ref_cls)
    boxes = np.concatenate([out["dets"][f, :k, :4].cpu().numpy() for f, k in enumerate(ks)])
    masks_ts = []
    for v in pipe.mask_views:
        o = out["views"][v]
        b = aspect_ref.head_boxes(boxes, FRAME_HW[1], v[3] if len(v) > 3 else None, v[2])
        want = aspect_ref.head_rois(b, pipe.geom[v].scale)[:, 1:]
        assert np.array_equal(o["mask_rois"].cpu().numpy()[:, 1:], want), v
        m = o["masks"].cpu().numpy()
        masks_ts.append(m[:, :, ::-1] if v[2] else m)
    assert out["masks"].shape[0] == sum(ks)
    assert np.array_equal(out["masks"].cpu().numpy(), np.mean(masks_ts, axis=0))


def test_pipeline_stagewise(tta):
    cfg, pipe, frames, out = tta
    _check_step(cfg, pipe, out)
    # the aspect-ratio views contribute candidates of their own
    for v in pipe.box_views:
        assert int(out["views"][v]["roi_counts"].min()) > 0


def test_pipeline_graph_replay_equals_eager(tta):
    cfg, pipe, frames, eager = tta
    x = _t(frames)
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
    for k in ("masks", "dets", "counts"):
        gout[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    out = pipe.complete(dict(gout))
    assert out["counts_host"] == eager["counts_host"]
    for k in ("dets", "classes", "counts", "mask_rois", "masks"):
        assert torch.equal(out[k], eager[k]), k


def test_pipeline_refuses_a_view_under_two_columns(tta):
    from vosdetectron_amd.engine import AugFramePipeline
    cfg, pipe, frames, out = tta
    bad = _mask_cfg()
    bad.TEST.BBOX_AUG.ASPECT_RATIOS = (0.004,)
    with pytest.raises(ValueError, match="under 2"):
        AugFramePipeline(pipe.model, bad, frame_hw=FRAME_HW, batch=2, device=DEV,
                         channels_last=True)


# --------------------------------------------------------------------------- #
# 4. KeypointAugFramePipeline                                                  #
# --------------------------------------------------------------------------- #
def test_keypoint_pipeline_with_an_aspect_view():
    """One aspect-ratio keypoint view beside the identity view: the view's RoIs are the
    restatement's, and the fused combine-and-decode equals the plain decode of the
    torch-combined maps."""
    import bench
    from vosdetectron_amd import config as vcfg, ops
    from vosdetectron_amd.engine import KeypointAugFramePipeline
    from vosdetectron_amd.weights import build_model
    hw = (320, 480)
    cfg = vcfg.get("e2e_keypoint_rcnn_R-50-FPN_1x")
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = hw
    model, sd = build_model(cfg, seed=0, device=DEV, channels_last=True)
    cfg.TEST.KPS_AUG.update(dict(ENABLED=True, ASPECT_RATIOS=(1.5,)))
    frames = torch.from_numpy(bench.synthetic_frames(2, 21, *hw)).to(DEV)
    pipe = KeypointAugFramePipeline(model, cfg, frame_hw=hw, batch=2, channels_last=True,
                                    device=DEV)
    ident, ar = hw + (False,), hw + (False, 1.5)
    assert pipe.kps_views == [ident, ar] and pipe.kps_ds == pipe.kps_us == [False, False]
    pipe.run(frames)
    out = pipe.run(frames, keep_intermediates=True)
    torch.cuda.synchronize()
    ks = out["counts_host"]
    M = sum(ks)
    assert M > 0
    boxes = np.concatenate([out["dets"][f, :k, :4].cpu().numpy() for f, k in enumerate(ks)])
    g = pipe.geom[ar]
    assert g.im_hw.cpu().tolist() == [[320, 720]] * 2 and g.scale == ops.target_scale(
        320, 720, 320, 480)
    want = aspect_ref.head_rois(aspect_ref.head_boxes(boxes, hw[1], 1.5, False), g.scale)
    assert np.array_equal(out["views"][ar]["kps_rois"].cpu().numpy()[:, 1:], want[:, 1:])
    h0, h1 = (out["views"][v]["kps_heatmaps"] for v in (ident, ar))
    assert not torch.equal(h0, h1)
    comb = (h0 + h1) / 2  # np.mean of two float32 arrays: one rounded sum, an exact halving
    assert torch.equal(out["kps_heatmaps"], comb)
    two = ops.heatmaps_to_keypoints(comb, out["kps_boxes"], cfg.KRCNN.INFERENCE_MIN_SIZE)
    assert torch.equal(out["keyps"], two)
