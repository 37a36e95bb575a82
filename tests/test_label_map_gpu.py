"""vd_label_maps (viz_mask_result on the device) against the executed reference
(tests/golden/label_map.npz), the numpy restatement (tests/label_map_ref.py) and the
device composition of vd_paste_masks planes painted with torch -- always torch.equal on
uint8, no tolerance -- inside guarded buffers, and through the engine."""
import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import label_map_ref as lm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _t(a):
    """A device copy (the shared inputs are read-only numpy arrays)."""
    return torch.from_numpy(np.array(a)).to(DEV)


LUT = ((np.arange(64) * 37 + 255) % 256).astype(np.uint8)  # class 0 -> 255, no identity
VALID = np.ones((3, lm.N), np.uint8)
VALID.reshape(-1)[::3] = 0  # a third of the rows, row (0, 0) -- the whole-frame box -- among them
VARIANTS = {"plain": {}, "valid": {"valid": VALID}, "lut": {"lut": LUT},
            "valid-lut": {"valid": VALID, "lut": LUT}}


def _call(masks, dets, classes, counts, h, w, thresh=lm.THRESH, gt_thresh=lm.GT_THRESH, lut=None,
          valid=None):
    from vosdetectron_amd import ops
    return ops.label_maps(_t(masks), _t(dets), _t(classes), _t(counts), h, w, thresh, gt_thresh,
                          0.5, lut, None if valid is None else _t(valid))


def _compose(masks, dets, classes, counts, h, w, thresh, gt_thresh, lut=None, valid=None):
    """The device composition: vd_paste_masks planes of each frame painted with torch in
    the defined order (ascending float32 score, equal scores by ascending row)."""
    from vosdetectron_amd import ops
    F = len(counts)
    label = torch.zeros((F, h, w), dtype=torch.uint8, device=DEV)
    gt = torch.zeros_like(label)
    start = 0
    for f, k in enumerate(int(c) for c in counts):
        if k == 0:
            continue
        d = _t(np.ascontiguousarray(dets[f, :k]))
        planes = ops.paste_masks(_t(masks[start:start + k]), d, h, w, 0.5)
        start += k
        ids = lm.ids_of(classes[f, :k], lut)
        v = None if valid is None else valid[f, :k]
        for i in lm.order_of(dets[f, :k, 4], thresh, v):
            on = planes[i] > 0
            label[f][on] = int(ids[i])
            if dets[f, i, 4] > np.float32(gt_thresh):
                gt[f][on] = int(ids[i])
    return label, gt


def test_golden_frame(golden):
    """label and gt equal the maps the reference's own viz_mask_result produced."""
    g = golden("label_map")
    h, w = (int(v) for v in g["im_hw"])
    n = len(g["dets"])
    label, gt = _call(g["masks"], g["dets"][None], g["classes"][None], np.array([n], np.int32),
                      h, w, float(g["thresh"]), float(g["rvt_cls_threshold"]))
    assert torch.equal(label[0].cpu(), torch.from_numpy(g["outImg"]))
    assert torch.equal(gt[0].cpu(), torch.from_numpy(g["rtv_gt"]))


def test_viz_mask_result_entry(golden):
    """The reference-named entry: (rtv_gt, rtv_bboxs, outImg) of the golden frame."""
    from vosdetectron_amd import vis
    g = golden("label_map")
    rtv_gt, rtv_bboxs, out_img = vis.viz_mask_result(
        _t(g["masks"]), _t(g["dets"]), _t(g["classes"]), g["im_hw"], float(g["thresh"]),
        float(g["rvt_cls_threshold"]))
    assert out_img.dtype == np.uint8 and np.array_equal(out_img, g["outImg"])
    assert np.array_equal(rtv_gt, g["rtv_gt"])
    rows = np.asarray([np.concatenate([[c], b]) for c, bl in enumerate(rtv_bboxs) for b in bl],
                      np.float32).reshape(-1, 5)
    assert len(rtv_bboxs) == 256 and np.array_equal(rows, g["rtv_bboxs"])
    # no detections: zero maps, empty lists
    e = vis.viz_mask_result(torch.zeros((0, 28, 28), device=DEV), torch.zeros((0, 5), device=DEV),
                            torch.zeros((0,), dtype=torch.int32, device=DEV), (5, 9), 0.25, 0.6)
    assert not e[0].any() and not e[2].any() and e[2].shape == (5, 9) and not any(e[1])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("r", [28, 14])
def test_frames_vs_restatement_and_composition(r, variant):
    """F = 3 with counts (24, 0, 7): the prefix offsets, an empty frame (zero maps), rows
    past a count (a confident whole-frame box) never painted; tied scores by the rule."""
    masks, dets, classes, counts, planes = lm.frames(r)
    kw = VARIANTS[variant]
    want = lm.reference(planes, dets, classes, counts, **kw)
    label, gt = _call(masks, dets, classes, counts, lm.H, lm.W, **kw)
    assert torch.equal(label.cpu(), torch.from_numpy(want[0])), variant
    assert torch.equal(gt.cpu(), torch.from_numpy(want[1])), variant
    assert not label[1].any() and not gt[1].any()
    assert (want[0][0] == 0).any() == ("valid" in kw)  # uncovered pixels once row 0 is masked
    cl, cg = _compose(masks, dets, classes, counts, lm.H, lm.W, lm.THRESH, lm.GT_THRESH, **kw)
    assert torch.equal(label, cl) and torch.equal(gt, cg), variant
    # gt = None: the same label, no second map
    only, none = _call(masks, dets, classes, counts, lm.H, lm.W, gt_thresh=None, **kw)
    assert none is None and torch.equal(only, label)


def test_lut_ids_and_classes_outside_it():
    """ids up to 255; a class at or beyond lut_n, above 255 without a lut, or negative
    writes 0 (it still covers what it is painted over)."""
    masks, dets, classes, counts, planes = lm.frames()
    cls = np.array(classes)
    cls[0, 2], cls[0, 8], cls[0, 12] = 300, -4, 1 << 20
    short = LUT[:10]  # classes 10 .. 18 of frame 0 lie beyond it
    assert LUT[0] == 255 and (cls[0] >= 10).any()
    for lut in (None, short):
        want = lm.reference(planes, dets, cls, counts, lut=lut)
        label, gt = _call(masks, dets, cls, counts, lm.H, lm.W, lut=lut)
        assert torch.equal(label.cpu(), torch.from_numpy(want[0]))
        assert torch.equal(gt.cpu(), torch.from_numpy(want[1]))
    zero = np.zeros_like(cls)
    label, _ = _call(masks, dets, zero, counts, lm.H, lm.W, lut=LUT)
    assert set(label[0].unique().tolist()) == {255}


def test_frame_smaller_than_one_tile():
    masks, dets, classes = lm.make(2)
    dets = np.array(dets)
    dets[:, :4] *= (9 / lm.W, 5 / lm.H, 9 / lm.W, 5 / lm.H)
    planes = lm.planes_of(masks, dets, 5, 9)
    want = lm.paint(planes, dets[:, 4], classes, lm.THRESH, lm.GT_THRESH)
    label, gt = _call(masks, dets[None], classes[None], np.array([lm.N], np.int32), 5, 9)
    assert tuple(label.shape) == (1, 5, 9) and want[0].any()
    assert torch.equal(label[0].cpu(), torch.from_numpy(want[0]))
    assert torch.equal(gt[0].cpu(), torch.from_numpy(want[1]))


@pytest.mark.parametrize("n", [256, 600])
def test_every_row_painted_into_one_tile(n):
    """n = cap small overlapping boxes, all painted and all meeting tile (0, 0): the
    candidate list at capacity (256) and over more than one chunk of the workgroup (600);
    the frame has a second tile column and row that the boxes barely reach."""
    rng = np.random.default_rng(n)
    r, h, w = 14, 40, 70
    masks = np.stack([lm.blob(rng, r) for _ in range(n)])
    c = np.stack([rng.uniform(4, 60, n), rng.uniform(4, 28, n)], 1)
    wh = rng.uniform(3, 12, (n, 2))
    dets = np.hstack([c - wh / 2, c + wh / 2, rng.permutation(np.linspace(0.3, 0.99, n))[:, None]])
    dets = dets.astype(np.float32)
    dets[n // 2:n // 2 + 20, 4] = dets[3, 4]  # a run of ties among them
    classes = rng.integers(1, 200, n).astype(np.int32)
    planes = lm.planes_of(masks, dets, h, w)
    assert len(lm.order_of(dets[:, 4], lm.THRESH)) == n
    want = lm.paint(planes, dets[:, 4], classes, lm.THRESH, lm.GT_THRESH)
    label, gt = _call(masks, dets[None], classes[None], np.array([n], np.int32), h, w)
    assert torch.equal(label[0].cpu(), torch.from_numpy(want[0]))
    assert torch.equal(gt[0].cpu(), torch.from_numpy(want[1]))
    assert len(np.unique(want[0])) > 20 and not want[0][:, 68:].any()


def test_thresholds_compare_in_float32():
    """All scores below thresh: zero maps.  A score equal to float32(thresh) is painted and
    the next float32 below it is not -- at 0.7, where float32(0.7) < 0.7, so a float64
    comparison would skip it; a score equal to float32(0.6) is not `> 0.6` in float32
    though it is in float64, so it stays out of gt."""
    masks, dets, classes, _, _ = lm.inputs()
    one = np.array([lm.N], np.int32)
    label, gt = _call(masks, dets[None], classes[None], one, lm.H, lm.W, thresh=0.99,
                      gt_thresh=0.5)
    assert not label.any() and not gt.any()
    t7, t6 = np.float32(0.7), np.float32(0.6)
    assert float(t7) < 0.7 and float(t6) > 0.6
    d = np.array(dets[:2])
    d[:, :4] = (-5, -4, 90, 41)
    m = np.full((2, lm.R, lm.R), 0.9, np.float32)
    cls = np.array([[3, 9]], np.int32)
    two = np.array([2], np.int32)
    d[:, 4] = (t7, np.nextafter(t7, np.float32(0)))
    label, _ = _call(m, d[None], cls, two, lm.H, lm.W, thresh=0.7)
    assert set(label.unique().tolist()) == {3}  # row 0 at the threshold; row 1 under it
    d[:, 4] = (np.nextafter(t7, np.float32(0)), np.nextafter(t7, np.float32(0)))
    label, _ = _call(m, d[None], cls, two, lm.H, lm.W, thresh=0.7)
    assert not label.any()
    d[:, 4] = (t6, np.nextafter(t6, np.float32(1)))
    label, gt = _call(m, d[None], cls, two, lm.H, lm.W, thresh=0.25, gt_thresh=0.6)
    assert set(label.unique().tolist()) == {9} and set(gt.unique().tolist()) == {9}
    d[:, 4] = (t6, np.float32(0.3))
    label, gt = _call(m, d[None], cls, two, lm.H, lm.W, thresh=0.25, gt_thresh=0.6)
    assert set(label.unique().tolist()) == {3} and not gt.any()


# --------------------------------------------------------------------------- guarded buffers
@pytest.fixture(scope="module")
def arena():
    return G.Arena(DEV, 16 << 20)


def _guarded(arena, masks, dets, classes, counts, valid, lut, with_gt, ws_fill, out_fill):
    """vd_label_maps with every buffer a carve of exactly its size; the workspace exactly
    vd_label_maps_workspace_size bytes."""
    from vosdetectron_amd._lib import check, lib
    F, cap = dets.shape[:2]

    def put(a, name):
        src = torch.from_numpy(np.array(a))
        v = arena.carve(a.shape, src.dtype, G.ZERO, "vd_label_maps " + name, key=name)
        v.copy_(src)
        return v

    m, d, c, n = put(masks, "masks"), put(dets, "dets"), put(classes, "classes"), \
        put(counts, "counts")
    v = put(valid, "valid") if valid is not None else None
    lt = put(lut, "lut") if lut is not None else None
    label = arena.carve((F, lm.H, lm.W), torch.uint8, out_fill, "vd_label_maps label", key="label")
    gt = arena.carve((F, lm.H, lm.W), torch.uint8, out_fill, "vd_label_maps gt", key="gt") \
        if with_gt else None
    wsb = lib().vd_label_maps_workspace_size(F, cap)
    ws = arena.carve((wsb,), torch.uint8, ws_fill, "vd_label_maps workspace (%d bytes)" % wsb,
                     key="ws", strip=wsb // F)
    check(lib().vd_label_maps(
        m.data_ptr(), masks.shape[-1], d.data_ptr(), c.data_ptr(), n.data_ptr(),
        v.data_ptr() if v is not None else None, F, cap, lm.H, lm.W, 0.5,
        float(np.float32(lm.THRESH)), float(np.float32(lm.GT_THRESH)),
        lt.data_ptr() if lt is not None else None, len(lut) if lut is not None else 0,
        label.data_ptr(), gt.data_ptr() if gt is not None else None, ws.data_ptr(), wsb,
        G.stream()), "vd_label_maps")
    return label, gt


@pytest.mark.parametrize("variant", ["plain", "valid-lut", "no-gt"])
def test_guarded_buffers_and_wild_counts(arena, variant):
    """counts = (30, -5, 7) at cap 24 -- one above cap, one negative -- address as (24, 0,
    7); masks holds exactly those 31 rows.  Workspace 0x00 / 0xFF / the leftover of a larger
    instance, outputs pre-filled 0x00 / 0xFF: no canary byte touched, every output byte
    written, the same maps every time."""
    masks, dets, classes, counts, planes = lm.frames()
    kw = dict(VARIANTS.get(variant, {}))
    want = lm.reference(planes, dets, classes, counts, **kw)
    wild = np.array([30, -5, 7], np.int32)
    with_gt = variant != "no-gt"
    big_cap = 40
    bd = np.zeros((3, big_cap, 5), np.float32)
    bd[:, :lm.N], bd[:, lm.N:] = dets, dets[:, :big_cap - lm.N]
    bc = np.concatenate([classes, classes[:, :big_cap - lm.N]], 1)
    bcounts = np.array([big_cap, 3, 7], np.int32)
    bm = np.concatenate([masks, masks])[:int(bcounts.sum())]
    bv = None if "valid" not in kw else np.ones((3, big_cap), np.uint8)

    def small(w, o):
        return _guarded(arena, masks, dets, classes, wild, kw.get("valid"), kw.get("lut"),
                        with_gt, w, o)

    def large(w, o):
        return _guarded(arena, bm, bd, bc, bcounts, bv, kw.get("lut"), with_gt, w, o)

    def verify(res, out_fill, tag):
        label, gt = res
        assert torch.equal(label.cpu(), torch.from_numpy(want[0])), tag
        if with_gt:
            assert torch.equal(gt.cpu(), torch.from_numpy(want[1])), tag

    G.sweep(arena, small, large, verify)


# --------------------------------------------------------------------------- engine
def _thresholds(scores):
    """thresh / gt_thresh from the step's own scores (random weights score low): the
    median and the upper quartile, so some rows are skipped and gt differs from label."""
    s = np.sort(np.asarray(scores, np.float32))
    assert len(s) >= 8, "the step found too few detections to test with"
    return float(s[len(s) // 2]), float(s[3 * len(s) // 4])


@pytest.fixture(scope="module")
def fpn_step():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.e2e_mask_rcnn_R_50_FPN_1x()
    cfg.TEST.SCALE = 480
    vcfg.check_supported(cfg)
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True)
    pipe = FramePipeline(model, cfg, frame_hw=(480, 640), batch=2, device=DEV,
                         channels_last=True)
    frames = np.stack([np.random.RandomState(900 + r).randint(0, 256, (480, 640, 3), np.uint8)
                       for r in range(2)])
    return cfg, pipe, torch.from_numpy(frames).to(DEV)


def test_engine_before_and_after_complete(fpn_step):
    """frame_label_maps on a run(sync=False) output equals the call after complete(), and
    both equal the painting of that step's own frame_segms RLEs decoded on the host."""
    from vosdetectron_amd import engine
    cfg, pipe, frames = fpn_step
    out = pipe.run(frames, sync=False)
    ks = out["counts"].cpu().tolist()  # the test's own read; `out` stays un-completed
    all_dets = out["dets"].cpu().numpy()
    thresh, gt_thresh = _thresholds(np.concatenate([all_dets[f, :k, 4] for f, k in enumerate(ks)]))
    assert "counts_host" not in out
    label, gt = engine.frame_label_maps(pipe, out, thresh, gt_thresh)
    assert "counts_host" not in out and tuple(label.shape) == (2, 480, 640)
    pipe.complete(out)
    label2, gt2 = engine.frame_label_maps(pipe, out, thresh, gt_thresh)
    assert torch.equal(label, label2) and torch.equal(gt, gt2)
    K = int(cfg.MODEL.NUM_CLASSES)
    segms = engine.frame_segms(pipe, out, K)
    classes = out["classes"].cpu().numpy()
    for f, k in enumerate(ks):
        nxt = [0] * K
        planes = np.zeros((k, 480, 640), np.uint8)
        for i in range(k):
            c = int(classes[f, i])
            planes[i] = lm.rle_decode(segms[f][c][nxt[c]])
            nxt[c] += 1
        want = lm.paint(planes, all_dets[f, :k, 4], classes[f, :k], thresh, gt_thresh)
        assert want[0].any() and (want[0] != want[1]).any()
        assert torch.equal(label[f].cpu(), torch.from_numpy(want[0])), f
        assert torch.equal(gt[f].cpu(), torch.from_numpy(want[1])), f
    lut = ((np.arange(K) * 7 + 3) % 256).astype(np.uint8)
    relabel, _ = engine.frame_label_maps(pipe, out, thresh, lut=lut)
    lab = label.cpu()
    assert torch.equal(relabel.cpu(), torch.where(lab == 0, lab, torch.from_numpy(lut)[lab.long()]))


def test_vos_label_maps_show_what_frame_results_returns():
    """TEST.NMS_WITH_MASK_IOU on: the map is the painting of exactly the (cls_boxes,
    cls_segms) that frame_results returns -- rows the mask-IoU NMS dropped are absent."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import VOSPipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_davis")
    cfg.TEST.SCALE = 240
    cfg.TEST.NMS_WITH_MASK_IOU = 0.5
    cfg.TEST.NUM_DET_PER_CLASS_POST = 1
    vcfg.check_supported(cfg)
    frame = np.random.RandomState(300).randint(0, 256, (240, 427, 3), np.uint8)
    model, _ = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=frame)
    pipe = VOSPipeline(model, cfg, frame_hw=(240, 427), batch=1, device=DEV, channels_last=True)
    out = pipe.run(torch.from_numpy(frame[None]).to(DEV))
    cls_boxes, cls_segms = pipe.frame_results(out)[0]
    boxes = np.concatenate([b for b in cls_boxes if len(b)])
    classes = np.concatenate([[j] * len(b) for j, b in enumerate(cls_boxes)]).astype(np.int32)
    assert 0 < len(boxes) < out["counts_host"][0], "the mask-IoU NMS dropped nothing"
    s = np.sort(out["dets"][0, :out["counts_host"][0], 4].cpu().numpy())
    thresh, gt_thresh = float(s[len(s) // 4]), float(s[len(s) // 2])
    planes = np.stack([lm.rle_decode(sg) for sl in cls_segms for sg in sl])
    want = lm.paint(planes, boxes[:, 4], classes, thresh, gt_thresh)
    label, gt = pipe.frame_label_maps(out, thresh, gt_thresh)
    assert want[0].any()
    assert torch.equal(label[0].cpu(), torch.from_numpy(want[0]))
    assert torch.equal(gt[0].cpu(), torch.from_numpy(want[1]))
    # without the filter the unkept rows would show
    from vosdetectron_amd import engine
    unfiltered, _ = engine.frame_label_maps(pipe, out, thresh, gt_thresh)
    every = lm.paint(np.stack([lm.rle_decode(r) for r in _all_rles(pipe, out)]),
                     out["dets"][0, :len(s), 4].cpu().numpy(),
                     out["classes"][0, :len(s)].cpu().numpy(), thresh, gt_thresh)
    assert torch.equal(unfiltered[0].cpu(), torch.from_numpy(every[0]))


def _all_rles(pipe, out):
    from vosdetectron_amd import segm
    k = out["counts_host"][0]
    return segm.encode_masks(out["masks"][:k], out["dets"][0, :k], pipe.H, pipe.W,
                             pipe.cfg.MRCNN.THRESH_BINARIZE)
