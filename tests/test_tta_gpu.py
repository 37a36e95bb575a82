"""Test-time augmentation (TEST.BBOX_AUG / TEST.MASK_AUG) on the device:
vd_box_union_add_view / vd_box_union_detections, vd_mask_aug_accumulate / _finish and
engine.AugFramePipeline against tests/aug_ref.py (lib/core/test.py:193-363, 405-526 on
the oracle's numpy parts) and the oracle's box_results_with_nms_and_limit."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aug_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = (10., 10., 5., 5.)


def _record(name, data):
    """profiles/tta/<name>: a measured figure of this run (skipped on a read-only tree)."""
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "tta"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "tta", name), "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------- #
# 1. the executed reference (tests/golden/tta.npz) through the kernels         #
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("vote", ["plain", "vote"])
def test_golden_union_through_kernels(golden, vote):
    """The recorded per-view rois, scores and deltas through add_view x 6 + detections:
    dets, classes and counts bit-exact against the reference's own im_detect_bbox_aug +
    box_results_with_nms_and_limit, with and without box voting."""
    from vosdetectron_amd import ops
    g = golden("tta")
    T6, Rg, Kg = g["view_scores"].shape
    H, W = g["im"].shape[:2]
    thr, nms, per_im = g["test_cfg"]
    u = ops.BoxUnion(T6 * Rg, 1, Kg, DEV)
    hw = torch.tensor([[H, W]], dtype=torch.int32, device=DEV)
    for t in range(T6):
        u.add_view(_t(g["view_rois"][t][None]), _t(g["view_scores"][t][None]),
                   _t(g["view_deltas"][t][None]), torch.tensor([Rg], dtype=torch.int32, device=DEV),
                   torch.tensor([g["view_im_scale"][t]], dtype=torch.float32, device=DEV), hw,
                   bool(g["bbox_calls"][t][2]), score_thresh=thr,
                   bbox_reg_weights=tuple(g["weights"]))
    kw = dict(bbox_vote="AVG", bbox_vote_thresh=float(g["vote_cfg"][0])) if vote == "vote" else {}
    dets, dcls, dcnt = u.detections(nms, int(per_im), det_cap=64, **kw)
    want = g["det_%s_dets" % vote]
    n = int(dcnt[0].item())
    assert n == len(want) == int(per_im)
    assert np.array_equal(dets[0, :n].cpu().numpy(), want)
    assert np.array_equal(dcls[0, :n].cpu().numpy(), g["det_%s_cls" % vote])


@pytest.mark.parametrize("soft,vote", [("linear", None), ("gaussian", "IOU_AVG")])
def test_union_soft_nms_vs_oracle(golden, soft, vote):
    """TEST.SOFT_NMS (and voting on its rows) over the union of the fixture's first two
    views (one flipped; about 380 candidates per class), bit-exact against the oracle."""
    from vosdetectron_amd import ops
    g = golden("tta")
    Rg, Kg = g["view_scores"].shape[1:]
    H, W = g["im"].shape[:2]
    weights = tuple(float(w) for w in g["weights"])
    u = ops.BoxUnion(2 * Rg, 1, Kg, DEV)
    hw = torch.tensor([[H, W]], dtype=torch.int32, device=DEV)
    boxes_ts = []
    for t in range(2):
        hf = bool(g["bbox_calls"][t][2])
        u.add_view(_t(g["view_rois"][t][None]), _t(g["view_scores"][t][None]),
                   _t(g["view_deltas"][t][None]), torch.tensor([Rg], dtype=torch.int32, device=DEV),
                   torch.tensor([g["view_im_scale"][t]], dtype=torch.float32, device=DEV), hw, hf,
                   bbox_reg_weights=weights)
        boxes_ts.append(aug_ref.decode_view(g["view_rois"][t], g["view_deltas"][t],
                                            float(g["view_im_scale"][t]), g["im"].shape, hf,
                                            weights))
    sc, bx = aug_ref.union(list(g["view_scores"][:2]), boxes_ts)
    kw = dict(bbox_vote=vote, bbox_vote_thresh=0.5) if vote else {}
    dets, dcls, dcnt = u.detections(det_cap=512, soft_nms=soft, **kw)
    s, b, cls_boxes = orc.box_results_with_nms_and_limit(
        sc, bx, Kg, soft_nms_method=soft, bbox_vote=vote, bbox_vote_th=0.5)
    n = int(dcnt[0].item())
    assert n == len(s) and n > 0
    got = dets[0, :n].cpu().numpy()
    assert np.array_equal(got[:, :4], b) and np.array_equal(got[:, 4], s)
    assert np.array_equal(dcls[0, :n].cpu().numpy(),
                          np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, Kg)]))


@pytest.mark.parametrize("heur", ["SOFT_AVG", "SOFT_MAX"])
def test_golden_masks_through_kernels(golden, heur):
    """The recorded per-view masks (every class's plane as a row) through accumulate x 6
    + finish: bit-exact against the reference's own im_detect_mask_aug."""
    from vosdetectron_amd import ops
    g = golden("tta")
    vm = g["view_masks"]
    T6, M, Kg, Rm, _ = vm.shape
    flips = [False] + [bool(f) for _, _, f in g["body_calls"]]
    acc = torch.empty((M * Kg, Rm, Rm), dtype=torch.float32, device=DEV)
    for t in range(T6):
        ops.mask_aug_accumulate(acc, _t(vm[t].reshape(M * Kg, Rm, Rm)), flips[t], heur,
                                first=t == 0)
    got = ops.mask_aug_finish(acc, T6, heur).cpu().numpy().reshape(M, Kg, Rm, Rm)
    assert np.array_equal(got, g["masks_c_" + heur])


# --------------------------------------------------------------------------- #
# 2. synthetic union                                                           #
# --------------------------------------------------------------------------- #
IM_H, IM_W = 600, 901  # odd width: the flip's W - x - 1
T, R, K, NF = 3, 1000, 4, 2
SCALES = (0.5, 1.0, 1.7)
HFLIP = (False, True, False)


def _synthetic(ties):
    """T views of R proposals for two images.  Image 0: class 1 holds about 2500
    candidates above SCORE_THRESH (past class_nms_kernel's 2048 rows, five NMS blocks of
    512) in 40 clusters, so that suppression crosses block boundaries; class 2 holds
    none, class 3 one.  Image 1: about 600 class-1 candidates, roi_count 0 in view 1.
    ties: scores on a 1/256 grid (ties within and across views) and row 5 of view 2 a
    copy of row 5 of view 0 (same box, deltas and score in two views)."""
    rng = np.random.default_rng(11)
    rois = np.zeros((T, NF, R, 5), np.float32)
    cls = np.zeros((T, NF, R, K), np.float32)
    pred = rng.normal(0, 0.3, (T, NF, R, 4 * K)).astype(np.float32)
    counts = np.array([[R, R - 37], [R - 5, 0], [R, R]], np.int32)
    centres = rng.uniform([60, 60], [IM_W - 60, IM_H - 60], (40, 2))
    for t in range(T):
        for i in range(NF):
            c = centres[rng.integers(0, 40, R)] + rng.normal(0, 14, (R, 2))
            wh = rng.uniform(30, 160, (R, 2))
            box = np.hstack([c - wh / 2, c + wh / 2])
            box = np.clip(box, 0, [IM_W - 1, IM_H - 1, IM_W - 1, IM_H - 1])
            if HFLIP[t]:  # the view saw the flipped frame
                box = aug_ref.flip_boxes(box, IM_W)
            rois[t, i, :, 0] = i
            rois[t, i, :, 1:] = (box * SCALES[t]).astype(np.float32)
            hi = 0.3 if i == 0 else 0.07
            cls[t, i, :, 1] = rng.uniform(0, hi, R)
            cls[t, i, :, 2] = rng.uniform(0, 0.045, R)
            cls[t, i, :, 3] = rng.uniform(0, 0.04, R)
            cls[t, i, :, 0] = 1 - cls[t, i, :, 1:].sum(-1)
    cls[2, 0, 77, 3] = 0.8  # class 3 of image 0: one candidate, in the last view
    if ties:
        cls = (np.round(cls * 256) / 256).astype(np.float32)
        rois[2, 0, 5, 1:] = rois[0, 0, 5, 1:] / np.float32(SCALES[0]) * np.float32(SCALES[2])
        pred[2, 0, 5] = pred[0, 0, 5]
        cls[2, 0, 5] = cls[0, 0, 5] = np.float32([0.5, 0.25, 0., 0.])
    return rois, cls, pred, counts


def _union_reference(rois, cls, pred, counts, i, **kw):
    scores_ts, boxes_ts = [], []
    for t in range(T):
        n = counts[t, i]
        scores_ts.append(cls[t, i, :n])
        boxes_ts.append(aug_ref.decode_view(rois[t, i, :n], pred[t, i, :n],
                                            np.float32(SCALES[t]), (IM_H, IM_W, 3), HFLIP[t],
                                            WEIGHTS))
    sc, bx = aug_ref.union(scores_ts, boxes_ts)
    s, b, cls_boxes = orc.box_results_with_nms_and_limit(sc, bx, K, **kw)
    ref_cls = np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, K)] +
                             [np.zeros((0,))]).astype(np.int32)
    return s, b, ref_cls, (sc[:, 1:] >= 0.05).sum(0)


def _union_device(rois, cls, pred, counts, cand_cap, images=(0, 1), **kw):
    from vosdetectron_amd import ops
    F = len(images)
    u = ops.BoxUnion(cand_cap, F, K, DEV)
    sel = list(images)
    hw = torch.tensor([[IM_H, IM_W]] * F, dtype=torch.int32, device=DEV)
    for t in range(T):
        u.add_view(_t(rois[t, sel]), _t(cls[t, sel]), _t(pred[t, sel]), _t(counts[t, sel]),
                   torch.full((F,), SCALES[t], dtype=torch.float32, device=DEV), hw, HFLIP[t])
    cand = torch.zeros((F, K), dtype=torch.int32, device=DEV)
    dets, dcls, dcnt = u.detections(det_cap=512, cand_counts=cand, **kw)
    return dets.cpu().numpy(), dcls.cpu().numpy(), dcnt.cpu().numpy(), cand.cpu().numpy()


def _same(dets, dcls, n, ref):
    s, b, c = ref[:3]
    assert n == len(s), (n, len(s))
    assert np.array_equal(dets[:n, :4], b)
    assert np.array_equal(dets[:n, 4], s)
    assert np.array_equal(dcls[:n], c)


@pytest.fixture(scope="module", params=[False, True], ids=["distinct", "ties"])
def synthetic(request):
    data = _synthetic(request.param)
    refs = {vote: [_union_reference(*data, i, **kw) for i in range(NF)]
            for vote, kw in (("plain", {}),
                             ("vote", dict(bbox_vote="AVG", bbox_vote_th=0.9)))}
    return data, refs


@pytest.mark.parametrize("vote", ["plain", "vote"])
def test_union_vs_oracle(synthetic, vote):
    """add_view x 3 + detections at cand_cap 4096, bit-exact against the oracle's
    box_results_with_nms_and_limit on the np.vstack of the decoded views."""
    data, refs = synthetic
    kw = dict(bbox_vote="AVG", bbox_vote_thresh=0.9) if vote == "vote" else {}
    dets, dcls, dcnt, cand = _union_device(*data, 4096, **kw)
    n_cand = refs[vote][0][3]
    assert 2048 < n_cand[0] < 4096 and n_cand[1] == 0 and n_cand[2] == 1, n_cand
    for i in range(NF):
        assert np.array_equal(cand[i, 1:], refs[vote][i][3])
        _same(dets[i], dcls[i], dcnt[i], refs[vote][i])


def test_union_overflow_and_batch_invariance(synthetic):
    """cand_cap 1024: image 0's class-1 list overflows (count -1), image 1 is unharmed;
    image 0 alone (F = 1) gives the rows it gives in the batch of two."""
    data, refs = synthetic
    dets, dcls, dcnt, _ = _union_device(*data, 1024)
    assert dcnt[0] == -1
    _same(dets[1], dcls[1], dcnt[1], refs["plain"][1])
    d1, c1, n1, _ = _union_device(*data, 4096, images=(0,))
    _same(d1[0], c1[0], n1[0], refs["plain"][0])
    from vosdetectron_amd import ops
    with pytest.raises(ops._lib.VosdetError):
        ops.raise_on_failed_counts(dcnt.tolist())


def test_union_argument_errors():
    from vosdetectron_amd import _lib, ops
    with pytest.raises(ValueError):
        ops.BoxUnion(16385, 1, K, DEV)
    u = ops.BoxUnion(8192, 1, K, DEV)
    with pytest.raises(_lib.VosdetError, match="shape"):  # soft-NMS beyond its 4096 rows
        u.detections(soft_nms="linear")


# --------------------------------------------------------------------------- #
# 3. mask combination                                                          #
# --------------------------------------------------------------------------- #
def _view_masks(M, Tn, rng, plant):
    ms = [rng.uniform(0, 1, (M, 28, 28)).astype(np.float32) for _ in range(Tn)]
    if plant and M:
        for t, m in enumerate(ms):  # exact 0, 1 and 1e-20 at places that differ per view
            m[0, t % 28, 0] = 0.0
            m[0, (t + 3) % 28, 1] = 1.0
            m[0, (t + 5) % 28, 2] = 1e-20
            m[M - 1, 27, 27 - t] = 1.0
    return ms


@pytest.mark.parametrize("Tn", [1, 2, 5])
@pytest.mark.parametrize("M", [0, 1, 70])
@pytest.mark.parametrize("heur", ["SOFT_AVG", "SOFT_MAX", "LOGIT_AVG"])
def test_mask_combine(heur, M, Tn):
    """SOFT_AVG / SOFT_MAX bit-exact against np.mean / np.amax of the inverted views;
    LOGIT_AVG equal where an exact 1 among the inputs drives the result through inf, and
    elsewhere within 4 x the float32-vs-float64 error of the reference's own evaluation
    on these inputs (device logf / expf and numpy's SIMD forms are each 1-2 ulp and
    independent)."""
    from vosdetectron_amd import ops
    rng = np.random.default_rng(100 * M + Tn)
    flips = [bool((t * 3 + 1) % 2) if t else False for t in range(Tn)]  # mixed, identity first
    raw = _view_masks(M, Tn, rng, heur == "LOGIT_AVG")
    masks_ts = [aug_ref.invert_masks(m, f) for m, f in zip(raw, flips)]
    ref = aug_ref.combine_masks(masks_ts, heur)
    acc = torch.empty((M, 28, 28), dtype=torch.float32, device=DEV)
    for t in range(Tn):
        ops.mask_aug_accumulate(acc, _t(raw[t]), flips[t], heur, first=t == 0)
    got = ops.mask_aug_finish(acc, Tn, heur).cpu().numpy()
    assert ref.dtype == np.float32 and got.shape == ref.shape
    if heur != "LOGIT_AVG":
        assert np.array_equal(got, ref)
        return
    with np.errstate(divide="ignore"):
        mean_logit = np.mean([aug_ref.logit(y) for y in masks_ts], axis=0) if M else ref
    driven = ~np.isfinite(mean_logit)
    assert np.array_equal(got[driven], ref[driven])
    bound = 4 * aug_ref.logit_avg_float32_error(masks_ts)
    err = float(np.abs(got[~driven] - ref[~driven]).max()) if M else 0.0
    print("LOGIT_AVG M=%d T=%d: max |device - numpy| = %.3e, bound %.3e" % (M, Tn, err, bound))
    if M == 70 and Tn == 5:
        _record("logit_avg_error.json", {
            "what": "LOGIT_AVG, M = 70, T = 5, 28 x 28: 4 x max |numpy float32 - float64| of the "
                    "reference formula on the test's inputs (the test's bound), and the device's "
                    "max |difference| to numpy's float32 result",
            "bound": bound, "device_max_abs_diff": err})
    assert err <= bound, (err, bound)


# --------------------------------------------------------------------------- #
# 4. the pipeline, stage-wise                                                  #
# --------------------------------------------------------------------------- #
FRAME_HW = (224, 288)
AUG = dict(ENABLED=True, H_FLIP=True, SCALES=(160, 288), MAX_SIZE=384, SCALE_H_FLIP=True)


def _cfg(aug=True):
    from vosdetectron_amd import config as vcfg
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = 224, 288
    if aug:
        cfg.TEST.BBOX_AUG.update(AUG)
        cfg.TEST.MASK_AUG.update(AUG)
    vcfg.check_supported(cfg, test_aug=True)
    return cfg


def _frames():
    return np.stack([np.random.RandomState(1000 + i).randint(0, 256, FRAME_HW + (3,), np.uint8)
                     for i in range(2)])


@pytest.fixture(scope="module", params=[False, True], ids=["nchw", "nhwc"])
def tta(request):
    from vosdetectron_amd.engine import AugFramePipeline
    from vosdetectron_amd.weights import build_model
    cfg, frames = _cfg(), _frames()
    model, sd = build_model(cfg, device=DEV, channels_last=request.param,
                            calibrate_frame=frames[0])
    pipe = AugFramePipeline(model, cfg, frame_hw=FRAME_HW, batch=2, device=DEV,
                            channels_last=request.param, cand_cap=4096)
    # warm-up step: the views' convolution shapes are not in the shipped MIOpen Find db,
    # so their first run searches, and the solver it runs may differ from the one found
    pipe.run(_t(frames))
    out = pipe.run(_t(frames), keep_intermediates=True)
    return cfg, model, sd, pipe, frames, out


def test_pipeline_views_and_blobs(tta):
    cfg, model, sd, pipe, frames, out = tta
    assert len(pipe.box_views) == 6 and len(pipe.mask_views) == 6 and len(pipe.geom) == 6
    assert pipe.box_views[-1] == pipe.mask_views[0] == (224, 288, False)
    assert int(out["cand_counts"].max()) < pipe.cand_cap
    for v in pipe.box_views:
        blob = out["views"][v]["blob"].cpu().numpy()
        for f in range(2):
            im = frames[f][:, ::-1] if v[2] else frames[f]
            ref, im_scale, _ = orc.get_image_blob(np.ascontiguousarray(im), target_scale=v[0],
                                                  max_size=v[1], stride=cfg.FPN.COARSEST_STRIDE)
            assert im_scale == pipe.geom[v].scale
            assert np.array_equal(blob[f:f + 1], ref), (v, f)


def _oracle_union(cfg, pipe, out, f, views=None):
    """Decode + flip + vstack + box_results on the GPU's own per-view head outputs."""
    tst, Kc = cfg.TEST, cfg.MODEL.NUM_CLASSES
    scores_ts, boxes_ts = [], []
    for v in views or pipe.box_views:
        o = out["views"][v]
        n = int(o["roi_counts"][f].item())
        post = o["rois"].shape[1]
        rois = o["rois"][f, :n].cpu().numpy()
        sc = o["cls_prob"].view(-1, post, Kc)[f, :n].cpu().numpy()
        dl = o["bbox_pred"].view(-1, post, 4 * Kc)[f, :n].cpu().numpy()
        scores_ts.append(sc)
        boxes_ts.append(aug_ref.decode_view(rois, dl, np.float32(pipe.geom[v].scale),
                                            FRAME_HW + (3,), v[2],
                                            tuple(cfg.MODEL.BBOX_REG_WEIGHTS)))
    sc, bx = aug_ref.union(scores_ts, boxes_ts)
    return orc.box_results_with_nms_and_limit(sc, bx, Kc, tst.SCORE_THRESH, tst.NMS,
                                              tst.DETECTIONS_PER_IM)


def _check_detections(cfg, pipe, out):
    """Final dets bit-exact against the oracle's decode + flip + vstack + box_results on
    the run's own per-view head outputs."""
    for f in range(2):
        s_ref, b_ref, cls_boxes = _oracle_union(cfg, pipe, out, f)
        k = out["counts_host"][f]
        assert k == len(s_ref) and k > 0
        dets = out["dets"][f, :k].cpu().numpy()
        assert np.array_equal(dets[:, :4], b_ref) and np.array_equal(dets[:, 4], s_ref)
        ref_cls = np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, len(cls_boxes))])
        assert np.array_equal(out["classes"][f, :k].cpu().numpy(), ref_cls)


def _check_masks(pipe, out, heur="SOFT_AVG"):
    """Each mask view's mask_rois bit-exact against flip_boxes + the float64 product of
    the run's detections; the combined masks bit-exact against the in-order combination
    of the run's own per-view masks."""
    ks = out["counts_host"]
    boxes = np.concatenate([out["dets"][f, :k, :4].cpu().numpy() for f, k in enumerate(ks)])
    masks_ts = []
    for v in pipe.mask_views:
        o = out["views"][v]
        b = aug_ref.flip_boxes(boxes, FRAME_HW[1]) if v[2] else boxes
        ref = (b.astype(np.float64) * pipe.geom[v].scale).astype(np.float32)
        assert np.array_equal(o["mask_rois"].cpu().numpy()[:, 1:], ref), v
        masks_ts.append(aug_ref.invert_masks(o["masks"].cpu().numpy(), v[2]))
    assert out["masks"].shape[0] == sum(ks)
    assert np.array_equal(out["masks"].cpu().numpy(), aug_ref.combine_masks(masks_ts, heur))
    assert np.array_equal(out["mask_rois"].cpu().numpy(),
                          out["views"][pipe.mask_views[0]]["mask_rois"].cpu().numpy())


def test_pipeline_detections_stagewise(tta):
    cfg, model, sd, pipe, frames, out = tta
    _check_detections(cfg, pipe, out)


def test_pipeline_masks_stagewise(tta):
    cfg, model, sd, pipe, frames, out = tta
    _check_masks(pipe, out)


# Two runs of one step can be compared bit for bit only where the body repeats itself.
# With channels_last the whole step does.  In NCHW the body's convolutions do not: two
# FramePipeline runs on the same frames differ in every FPN level (measured on an MI355X:
# detections apart by about 3e-4 px), before any test-time-augmentation code runs.  There
# the same properties are asserted on one run's own tensors instead.
def test_pipeline_async_equals_sync(tta):
    """run(sync=False) + complete() is run(sync=True): nothing is read before complete(),
    complete() only trims the queued tensors, and the queued step passes the same
    stage-wise checks against its own per-view outputs as the synchronous one;
    channels_last: also bit-identical to the synchronous run."""
    cfg, model, sd, pipe, frames, out = tta
    o2 = pipe.run(_t(frames), keep_intermediates=True, sync=False)
    assert "counts_host" not in o2 and o2["masks"].shape[0] == pipe.mask_rows(2)
    queued = {k: o2[k].clone() for k in ("dets", "classes", "counts", "masks", "mask_rois")}
    pipe.complete(o2)
    M = sum(o2["counts_host"])
    assert o2["counts_host"] == queued["counts"].cpu().tolist()
    assert torch.equal(o2["dets"], queued["dets"]) and torch.equal(o2["classes"], queued["classes"])
    assert torch.equal(o2["masks"], queued["masks"][:M])
    assert torch.equal(o2["mask_rois"], queued["mask_rois"][:M])
    _check_detections(cfg, pipe, o2)
    _check_masks(pipe, o2)
    if pipe.channels_last:
        assert o2["counts_host"] == out["counts_host"]
        for k in ("dets", "classes", "masks", "mask_rois"):
            assert torch.equal(o2[k], out[k]), k


def test_complete_runs_the_rows_past_the_padded_mask_batch(tta, monkeypatch):
    """A padded mask batch shorter than the detections: complete() sends the rest through
    every mask view again, and the per-view intermediates grow with them.  Both layouts:
    the completed step passes the stage-wise checks on its own tensors, over all M rows.
    channels_last (where two runs of the body agree bit for bit, see above): detections,
    mask RoIs and mask RoI features are the full run's, the masks within 1e-5 (the mask
    head's GEMM may pick another algorithm for the other batch size)."""
    cfg, model, sd, pipe, frames, ref = tta
    M = sum(ref["counts_host"])
    cap = 64 if M > 64 else M // 2
    assert 0 < cap < M
    monkeypatch.setattr(pipe, "mask_rows", lambda F: cap)
    out = pipe.run(_t(frames), keep_intermediates=True, sync=False)
    assert out["masks"].shape[0] == cap and "_pyrs" in out
    pipe.complete(out)
    assert "_pyrs" not in out
    rows = sum(out["counts_host"])
    assert rows > cap
    for k in ("masks", "mask_rois", "mask_feat"):
        assert out[k].shape[0] == rows, k
    for v in pipe.mask_views:
        for k in ("masks", "mask_rois"):
            assert out["views"][v][k].shape[0] == rows, (v, k)
    _check_detections(cfg, pipe, out)
    _check_masks(pipe, out)
    if pipe.channels_last:
        assert out["counts_host"] == ref["counts_host"]
        for k in ("dets", "classes", "counts", "mask_rois", "mask_feat"):
            assert torch.equal(out[k], ref[k]), k
        assert out["masks"].shape == ref["masks"].shape
        assert float((out["masks"] - ref["masks"]).abs().max()) <= 1e-5
        for v in pipe.mask_views:
            o, r = out["views"][v], ref["views"][v]
            assert torch.equal(o["mask_rois"], r["mask_rois"]), v
            assert o["masks"].shape == r["masks"].shape
            assert float((o["masks"] - r["masks"]).abs().max()) <= 1e-5, v


def test_pipeline_without_aug_is_frame_pipeline(tta):
    """Both AUG keys off: the identity view alone through the union and mask-combine
    kernels is FramePipeline's step bit for bit -- vd_box_detections on the run's own
    head outputs gives the same detections, the combined masks are the view's masks;
    channels_last: also bit-identical to a FramePipeline run."""
    from vosdetectron_amd import ops
    from vosdetectron_amd.engine import AugFramePipeline, FramePipeline
    cfg, model, sd, pipe, frames, out = tta
    plain, tst = _cfg(aug=False), cfg.TEST
    kw = dict(frame_hw=FRAME_HW, batch=2, device=DEV, channels_last=pipe.channels_last)
    ap = AugFramePipeline(model, plain, **kw)
    assert ap.box_views == ap.mask_views == [(224, 288, False)]
    a = ap.run(_t(frames), keep_intermediates=True)
    Kc, post = plain.MODEL.NUM_CLASSES, a["rois"].shape[1]
    g = ap.geom[ap.box_views[0]]
    dets, dcls, dcnt = ops.box_detections(
        a["rois"], a["cls_prob"].view(2, post, Kc), a["bbox_pred"].view(2, post, 4 * Kc),
        a["roi_counts"], g.im_scale_t, ap.im_hw, tst.SCORE_THRESH, tst.NMS,
        tst.DETECTIONS_PER_IM, plain.MODEL.BBOX_REG_WEIGHTS, ap.det_cap)
    assert sum(a["counts_host"]) > 0 and dcnt.cpu().tolist() == a["counts_host"]
    assert torch.equal(dets, a["dets"]) and torch.equal(dcls, a["classes"])
    assert torch.equal(a["masks"], a["views"][ap.mask_views[0]]["masks"])
    _check_masks(ap, a)
    if pipe.channels_last:
        b = FramePipeline(model, plain, **kw).run(_t(frames))
        assert a["counts_host"] == b["counts_host"]
        for k in ("dets", "classes", "masks", "mask_rois"):
            assert torch.equal(a[k], b[k]), k


def test_other_pipelines_refuse_aug(tta):
    from vosdetectron_amd.engine import FramePipeline, RaggedFramePipeline
    cfg, model, sd, pipe, frames, out = tta
    with pytest.raises(NotImplementedError, match="AugFramePipeline"):
        FramePipeline(model, cfg, frame_hw=FRAME_HW, device=DEV)
    with pytest.raises(NotImplementedError, match="AugFramePipeline"):
        RaggedFramePipeline(model, cfg, (256, 320), device=DEV)


# --------------------------------------------------------------------------- #
# 5. against the independent CPU pipeline                                      #
# --------------------------------------------------------------------------- #
_CPU = {}


def _cpu_reference(cfg, sd, frames):
    """aug_ref on the CPU pipeline, once for both layouts (the synthetic weights are
    the same): per frame (scores, boxes, classes, masks, extra)."""
    if "ref" not in _CPU:
        from oracle.pipeline import RefCPUPipeline
        from vosdetectron_amd import config as vcfg
        from vosdetectron_amd.modeling import _stage_counts
        torch.set_num_threads(16)
        ref = aug_ref.AugRef(RefCPUPipeline(sd, block_counts=_stage_counts(cfg.MODEL.CONV_BODY),
                                            groups=cfg.RESNETS.NUM_GROUPS))
        box_views, mask_views = vcfg.aug_views(cfg)
        _CPU["ref"] = [ref(fr, box_views, mask_views, "SOFT_AVG") for fr in frames]
    return _CPU["ref"]


def _classes(cls_boxes):
    return np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, len(cls_boxes))] +
                          [np.zeros((0,))]).astype(np.int32)


def _share(got, ref):
    """Share of the reference detections (scores, boxes, classes) matched by class and
    IoU > 0.95 among `got` (engine_checks.match)."""
    from tests.engine_checks import match
    gs, gb, gc = got
    rs, rb, rc = ref
    z = np.zeros((max(len(gs), len(rs)), 1, 1), np.float32)
    matched, _ = match(np.hstack([gb, gs[:, None]]), gc, z, rs, rb, rc, z)
    return matched / max(len(rs), 1)


def test_pipeline_views_vs_cpu(tta):
    """Every view alone: box_results on the view's GPU head outputs (inverted to the
    frame) against aug_ref.box_view on the CPU, with e2e_vs_cpu's thresholds (counts
    within 2 %, at least 2; 98 % of the CPU detections matched)."""
    cfg, model, sd, pipe, frames, out = tta
    cpu = _cpu_reference(cfg, sd, frames)
    tst, Kc = cfg.TEST, cfg.MODEL.NUM_CLASSES
    for f in range(2):
        for i, v in enumerate(pipe.box_views):
            s, b, cb = _oracle_union(cfg, pipe, out, f, views=[v])
            sc, bx, _ = cpu[f][4]["per_view"][i]
            rs, rb, rcb = orc.box_results_with_nms_and_limit(sc, bx, Kc, tst.SCORE_THRESH,
                                                             tst.NMS, tst.DETECTIONS_PER_IM)
            assert abs(len(s) - len(rs)) <= max(2, 0.02 * len(rs)), (f, v, len(s), len(rs))
            share = _share((s, b, _classes(cb)), (rs, rb, _classes(rcb)))
            print("frame %d view %s: %d GPU / %d CPU detections, %.3f matched"
                  % (f, v, len(s), len(rs), share))
            assert share >= 0.98, (f, v, share)


def _view_differences(cfg, pipe, out, cpu, f):
    """GPU - CPU differences of the per-view union inputs on the proposals both have
    (RoIs equal within half a pixel): relative score differences of the entries at or
    above SCORE_THRESH and the absolute differences of their decoded boxes."""
    Kc, thr = cfg.MODEL.NUM_CLASSES, cfg.TEST.SCORE_THRESH
    rel, px = [], []
    for i, v in enumerate(pipe.box_views):
        o = out["views"][v]
        n = int(o["roi_counts"][f].item())
        post = o["rois"].shape[1]
        rois = o["rois"][f, :n, 1:].cpu().numpy()
        sc = o["cls_prob"].view(-1, post, Kc)[f, :n].cpu().numpy()
        dl = o["bbox_pred"].view(-1, post, 4 * Kc)[f, :n].cpu().numpy()
        bx = aug_ref.decode_view(np.hstack([np.zeros((n, 1), np.float32), rois]), dl,
                                 np.float32(pipe.geom[v].scale), FRAME_HW + (3,), v[2],
                                 tuple(cfg.MODEL.BBOX_REG_WEIGHTS))
        csc, cbx, ex = cpu[f][4]["per_view"][i]
        d = np.abs(rois[:, None, :] - ex["rois"][None, :, 1:]).max(-1)
        j = d.argmin(1)
        common = np.where(d[np.arange(n), j] < 0.5)[0]
        a, b = sc[common, 1:], csc[j[common], 1:]
        hit = b >= thr
        rel.append(np.abs(a - b)[hit] / b[hit])
        ab = bx[common].reshape(len(common), Kc, 4)[:, 1:]
        bb = cbx[j[common]].reshape(len(common), Kc, 4)[:, 1:]
        px.append(np.abs(ab - bb)[hit].ravel())
    return np.concatenate(rel), np.concatenate(px)


def test_pipeline_union_vs_cpu(tta):
    """The final result against aug_ref's.  The union is more sensitive to rounding than
    one view (T times the candidates compete in every NMS), so the threshold is set by
    the reference itself: the CPU union's input is perturbed by the measured GPU - CPU
    magnitude of the per-view scores and boxes (their 95th percentiles; uniform noise,
    fixed seed), and the GPU must match the CPU result at least as well as the perturbed
    CPU result matches it, minus 5 points (one draw is one sample).  Masks of matched
    pairs: the project's 1e-3 median."""
    from tests.engine_checks import match
    cfg, model, sd, pipe, frames, out = tta
    cpu = _cpu_reference(cfg, sd, frames)
    tst, Kc = cfg.TEST, cfg.MODEL.NUM_CLASSES
    record = {}
    for f in range(2):
        sc, bx, cl, masks, ex = cpu[f]
        rel, px = _view_differences(cfg, pipe, out, cpu, f)
        rel95, px95 = float(np.percentile(rel, 95)), float(np.percentile(px, 95))
        rng = np.random.default_rng(5)
        s_c, b_c = ex["scores_c"], ex["boxes_c"]
        s_p = (s_c * (1 + rng.uniform(-rel95, rel95, s_c.shape))).astype(np.float32)
        b_p = (b_c + rng.uniform(-px95, px95, b_c.shape)).astype(np.float32)
        ps, pb, pcb = orc.box_results_with_nms_and_limit(s_p, b_p, Kc, tst.SCORE_THRESH, tst.NMS,
                                                         tst.DETECTIONS_PER_IM)
        self_share = _share((ps, pb, _classes(pcb)), (sc, bx, cl))
        k = out["counts_host"][f]
        o = int(sum(out["counts_host"][:f]))
        gd = out["dets"][f, :k].cpu().numpy()
        gc = out["classes"][f, :k].cpu().numpy()
        gm = out["masks"][o:o + k].cpu().numpy()
        matched, mask_err = match(gd, gc, gm, sc, bx, cl, masks)
        share = matched / len(sc)
        record["frame%d" % f] = dict(score_rel_diff_p95=rel95, box_abs_diff_px_p95=px95,
                                     cpu_self_matched_share=self_share, gpu_matched_share=share,
                                     cpu_detections=len(sc), gpu_detections=int(k),
                                     median_mask_err=float(np.median(mask_err)))
        print("frame %d: %s" % (f, record["frame%d" % f]))
    record["layout"] = "nhwc" if pipe.channels_last else "nchw"
    _record("e2e.json", record)
    for f in range(2):
        r = record["frame%d" % f]
        assert r["gpu_matched_share"] >= r["cpu_self_matched_share"] - 0.05, r
        assert r["median_mask_err"] < 1e-3, r
