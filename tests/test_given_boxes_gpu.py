"""Detection from given boxes on the device: vd_rois_from_boxes and vd_gather_rows
against the executed reference (tests/golden/given_boxes.npz) and its numpy restatement
(tests/given_boxes_ref.py), bit for bit; inside guarded, poisoned buffers; and through
FramePipeline / VOSPipeline with MODEL.FASTER_RCNN False, chained with the oracle's
bbox_transform, clip and box_results_with_nms_and_limit as engine_checks.stagewise
compares stages."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import given_boxes_ref as gb
from tests import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "given_boxes.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pack(box_list, cap=None):
    """Frames of different row counts -> boxes [F,cap,4] (rows past a count are a planted
    box that would merge with nothing it should), counts [F]."""
    counts = np.array([len(b) for b in box_list], np.int32)
    cap = cap or max(1, int(counts.max()))
    boxes = np.full((len(box_list), cap, 4), 7.25, np.float32)
    for f, b in enumerate(box_list):
        boxes[f, :min(len(b), cap)] = b[:cap]
    return boxes, counts


def _run(boxes, counts, scales, dedup):
    from vosdetectron_amd import ops
    out = ops.rois_from_boxes(_dev(boxes), _dev(np.asarray(counts, np.int32)),
                              _dev(np.asarray(scales, np.float64)), dedup)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _same(got, want, what):
    for g, w, name in zip(got, want, ("rois", "ucounts", "index", "inv_index")):
        guarded.rows_equal(g, w.astype(g.dtype), "%s: %s" % (what, name))


# --------------------------------------------------------------------------- kernel
TRIPLES = (("n1", "n300", "n5_equal"), ("n64", "below_quantum", "n65"),
           ("half_even", "scaled", "n300"), ("dedup0", "dedup0", "dedup0"),
           ("dedup_tenth", "dedup_tenth", "dedup_tenth"))


@pytest.mark.parametrize("names", TRIPLES)
def test_fixture_cases_as_frames_of_one_call(golden, names):
    """F = 3: three fixture cases as the frames of one call.  Against the fixture (the
    executed reference; its level column is 0, the kernel's is the frame, and
    rint(f * DEDUP_BOXES) is 0 for f <= 2 at both quanta, so order and maps are equal)
    and against the restatement, padding included, bit for bit."""
    pre = ["fpn/%s/" % n for n in names]
    dd = float(golden[pre[0] + "dedup"])
    assert all(float(golden[p + "dedup"]) == dd for p in pre)
    boxes, counts = _pack([golden[p + "boxes"] for p in pre])
    scales = [float(golden[p + "im_scale"]) for p in pre]
    rois, ucounts, index, inv = got = _run(boxes, counts, scales, dd)
    for f, p in enumerate(pre):
        u, n = len(golden[p + "rois"]), int(counts[f])
        assert ucounts[f] == u, (names[f], ucounts[f], u)
        guarded.rows_equal(rois[f, :u, 1:], golden[p + "rois"][:, 1:], names[f] + ": rois")
        assert (rois[f, :u, 0] == f).all()
        assert np.array_equal(index[f, :u], golden[p + "index"]), names[f]
        assert np.array_equal(inv[f, :n], golden[p + "inv_index"]), names[f]
    _same(got, gb.rois_from_boxes(boxes, counts, scales, dd), "restatement")


def test_frames_do_not_merge_and_an_empty_frame_writes_nothing(golden):
    """The same boxes in frames 0 and 2 with a zero-count frame between: different batch
    indices, equal maps, nothing merged across frames, frame 1 untouched."""
    b = golden["fpn/n65/boxes"]
    boxes, counts = _pack([b, b[:0], b], cap=70)
    rois, ucounts, index, inv = got = _run(boxes, counts, [1., 1., 1.], 0.0625)
    u = len(golden["fpn/n65/rois"])
    assert ucounts.tolist() == [u, 0, u] and u < 65
    assert (rois[0, :u, 0] == 0).all() and (rois[2, :u, 0] == 2).all()
    guarded.rows_equal(rois[0, :u, 1:], rois[2, :u, 1:], "frames 0 and 2")
    assert np.array_equal(index[0], index[2]) and np.array_equal(inv[0], inv[2])
    assert not rois[1].any() and not index[1].any() and not inv[1].any()
    _same(got, gb.rois_from_boxes(boxes, counts, [1., 1., 1.], 0.0625), "restatement")
    # a large frame number enters the hash (rint(f / 16) > 0) and changes no map
    F = 40
    boxes, counts = _pack([b] * F, cap=65)
    got = _run(boxes, counts, [1.] * F, 0.0625)
    _same(got, gb.rois_from_boxes(boxes, counts, [1.] * F, 0.0625), "F = 40")
    assert np.array_equal(got[3][39], inv[0][:65]) and (got[0][39, :u, 0] == 39).all()


def _many(rng, n, dup):
    b = gb._random_boxes(rng, n, (900, 1400), dup)
    b[1::97] = b[0]  # one long run of equal rows
    return b


@pytest.mark.parametrize("cap,counts", ((64, (64, 63, 1)), (65, (65, 64, 33)),
                                        (4096, (4096, 4097, 1000))))
def test_capacities(cap, counts):
    """Full frames at cap = 64 (one wave of positions per 16 threads), 65 (padded to 128
    keys) and 4096 (every LDS key in use); a count of 4097 writes ucounts = -1 and
    nothing else."""
    rng = np.random.default_rng(cap)
    boxes = np.stack([np.vstack([_many(rng, min(c, cap), 0.4),
                                 np.zeros((cap - min(c, cap), 4), np.float32)])
                      for c in counts])
    scales = [1., 1.6, 0.75]
    rois, ucounts, index, inv = got = _run(boxes, counts, scales, 0.0625)
    want = gb.rois_from_boxes(boxes, counts, scales, 0.0625)
    _same(got, want, "cap %d" % cap)
    for f, c in enumerate(counts):
        if c > cap:
            assert ucounts[f] == -1
            assert not rois[f].any() and not index[f].any() and not inv[f].any()
        else:
            assert 0 < ucounts[f] < c or c == 1
    with pytest.raises(ValueError, match="cap"):
        _run(np.zeros((1, 4097, 4), np.float32), [1], [1.], 0.0625)


def test_failed_counts_raise_and_negative_counts_pass_through():
    from vosdetectron_amd import _lib, ops
    boxes = np.zeros((3, 8, 4), np.float32)
    _, ucounts, _, _ = _run(boxes, [9, -2, 3], [1., 1., 1.], 0.0625)
    assert ucounts.tolist() == [-1, -2, 1]
    with pytest.raises(_lib.VosdetError):
        ops.raise_on_failed_counts(ucounts.tolist())


def _gather_ref(boxes, scores, deltas, index, inv, counts, ucounts):
    F, cap = boxes.shape[:2]
    rows = np.zeros((F, cap, 5), np.float32)
    so, do = np.zeros_like(scores), np.zeros_like(deltas)
    co = np.zeros((F,), np.int32)
    for f in range(F):
        n, u = int(counts[f]), int(ucounts[f])
        co[f] = u if u < 0 else n
        if u < 0:
            continue
        v = inv[f, :n]
        rows[f, :n, 0] = f
        rows[f, :n, 1:] = boxes[f][index[f][v]]
        so[f, :n], do[f, :n] = scores[f][v], deltas[f][v]
    return rows, so, do, co


def test_gather_rows_is_the_reference_inverse_map(golden):
    """scores[inv_index], pred_boxes[inv_index] of test.py:186-189 in front of the decode:
    with the stand-in head on the distinct RoIs, the gathered scores are the fixture's
    final scores, and decoding the gathered box rows with the gathered deltas gives its
    pred_boxes, bit for bit.  A failed frame passes its code on and writes nothing."""
    from vosdetectron_amd import ops
    names = ("n300", "below_quantum", "scaled")
    pre = ["fpn/%s/" % n for n in names]
    boxes, counts = _pack([golden[p + "boxes"] for p in pre] + [np.zeros((400, 4), np.float32)],
                          cap=300)
    scales = [float(golden[p + "im_scale"]) for p in pre] + [1.]
    F, cap, K = 4, 300, gb.K
    rois, ucounts, index, inv = _run(boxes, counts, scales, 0.0625)
    assert ucounts[3] == -1
    scores = np.zeros((F, cap, K), np.float32)
    deltas = np.zeros((F, cap, 4 * K), np.float32)
    for f in range(3):  # the head sees the fixture's rows: level column 0
        r = rois[f, :ucounts[f]].copy()
        r[:, 0] = 0
        scores[f, :ucounts[f]], deltas[f, :ucounts[f]] = gb.standin_head(r)
    got = ops.gather_rows(_dev(boxes), _dev(scores), _dev(deltas), _dev(index), _dev(inv),
                          _dev(counts), _dev(ucounts))
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got]
    want = _gather_ref(boxes, scores, deltas, index, inv, counts, ucounts)
    for g, w, what in zip(got, want, ("box rows", "scores", "deltas", "counts")):
        guarded.rows_equal(g, w, what)
    assert got[3].tolist() == [300, 5, 80, -1]
    for f, p in enumerate(pre):
        n = int(counts[f])
        guarded.rows_equal(got[1][f, :n], golden[p + "scores"], names[f] + ": scores")
        pred = orc.clip_tiled_boxes(orc.bbox_transform(got[0][f, :n, 1:], got[2][f, :n],
                                                       gb.REG_WEIGHTS),
                                    tuple(golden[p + "im_shape"]))
        guarded.rows_equal(pred, golden[p + "pred_boxes"], names[f] + ": pred_boxes")


def test_ndarray_drop_ins(golden):
    from vosdetectron_amd import boxes as vboxes, ops
    for name in ("n300", "half_even", "dedup_tenth", "dedup0", "scaled"):
        p = "single/%s/" % name
        blob = ops.get_rois_blob(golden[p + "boxes"], float(golden[p + "im_scale"]))
        guarded.rows_equal(blob, gb.rois_blob(golden[p + "boxes"], float(golden[p + "im_scale"])),
                           name + ": get_rois_blob")
        r, index, inv = vboxes.dedup_boxes(blob, float(golden[p + "dedup"]))
        guarded.rows_equal(r, golden[p + "rois"], name + ": rois")
        assert index.dtype == inv.dtype == np.int64
        assert np.array_equal(index, golden[p + "index"]), name
        assert np.array_equal(inv, golden[p + "inv_index"]), name
    with pytest.raises(ValueError, match="column 0"):
        vboxes.dedup_boxes(np.ones((2, 5), np.float32))


# --------------------------------------------------------------------------- guarded
@pytest.fixture(scope="module")
def arena():
    return guarded.Arena(DEV, 8 << 20)


def test_rois_from_boxes_in_guarded_buffers(golden, arena):
    """Every buffer exact and between canaries, outputs pre-filled 0x00 and 0xFF, alone and
    after a larger instance ran in the same carves: no byte outside any buffer changes and
    the rows past the counts keep the prefill.  The reported workspace size is 0 and the
    wrapper passes none, so there is no workspace to poison: the sweep's workspace modes
    only decide whether the larger instance runs first."""
    from vosdetectron_amd import ops
    small_b, small_n = _pack([golden["fpn/n65/boxes"], np.zeros((0, 4), np.float32),
                              golden["fpn/half_even/boxes"], np.zeros((66, 4), np.float32)],
                             cap=65)
    large_b, large_n = _pack([golden["fpn/n300/boxes"]] * 3, cap=300)

    def call(boxes, counts, ws_fill, out_fill):
        F, cap = boxes.shape[:2]
        ins = []
        for a, name in ((boxes, "boxes"), (counts, "counts"),
                        (np.full((F,), 1.0, np.float64), "im_scale")):
            v = arena.carve(a.shape, torch.from_numpy(a).dtype, guarded.ZERO, name=name)
            v.copy_(torch.from_numpy(a))
            ins.append(v)
        outs = tuple(arena.carve(s, dt, out_fill, name=name, key=("out", name))
                     for s, dt, name in (((F, cap, 5), torch.float32, "rois"),
                                         ((F,), torch.int32, "ucounts"),
                                         ((F, cap), torch.int32, "index"),
                                         ((F, cap), torch.int32, "inv_index")))
        assert ops.rois_from_boxes_workspace(F, cap) == 0
        res = ops.rois_from_boxes(*ins, 0.0625, out=outs)
        return res, boxes, counts

    def verify(res, out_fill, tag):
        (rois, ucounts, index, inv), boxes, counts = res
        want = gb.rois_from_boxes(boxes, counts, np.ones(len(counts)), 0.0625)
        uc = ucounts.cpu().numpy()
        assert np.array_equal(uc, want[1]), (tag, uc, want[1])
        assert uc.tolist()[1] == 0 and uc.tolist()[3] == -1
        for f in range(len(counts)):
            u, n = max(int(uc[f]), 0), int(counts[f]) if uc[f] >= 0 else 0
            guarded.rows_equal(rois[f, :u].cpu().numpy(), want[0][f, :u], tag + ": rois")
            assert np.array_equal(index[f, :u].cpu().numpy(), want[2][f, :u]), tag
            assert np.array_equal(inv[f, :n].cpu().numpy(), want[3][f, :n]), tag
            guarded.assert_prefill(rois[f, u:], out_fill, "%s: rois of frame %d" % (tag, f))
            guarded.assert_prefill(index[f, u:], out_fill, "%s: index of frame %d" % (tag, f))
            guarded.assert_prefill(inv[f, n:], out_fill, "%s: inv_index of frame %d" % (tag, f))

    guarded.sweep(arena, lambda ws, of: call(small_b, small_n, ws, of),
                  lambda ws, of: call(large_b, large_n, ws, of), verify)


def test_gather_rows_in_guarded_buffers(golden, arena):
    from vosdetectron_amd import ops
    boxes, counts = _pack([golden["fpn/n65/boxes"], np.zeros((0, 4), np.float32),
                           golden["fpn/n64/boxes"], np.zeros((70, 4), np.float32)], cap=65)
    F, cap, K, D = 4, 65, 3, 12
    rois, ucounts, index, inv = _run(boxes, counts, [1.] * F, 0.0625)
    rng = np.random.default_rng(5)
    scores = rng.uniform(0, 1, (F, cap, K)).astype(np.float32)
    deltas = rng.normal(0, 1, (F, cap, D)).astype(np.float32)
    want = _gather_ref(boxes, scores, deltas, index, inv, counts, ucounts)
    for out_fill in guarded.FILLS:
        arena.reset()
        ins = []
        for a, name in ((boxes, "boxes"), (scores, "scores"), (deltas, "deltas"),
                        (index, "index"), (inv, "inv_index"), (counts, "counts"),
                        (ucounts, "ucounts")):
            v = arena.carve(a.shape, torch.from_numpy(a).dtype, guarded.ZERO, name=name)
            v.copy_(torch.from_numpy(a))
            ins.append(v)
        outs = tuple(arena.carve(s, dt, out_fill, name=name)
                     for s, dt, name in (((F, cap, 5), torch.float32, "box rows"),
                                         ((F, cap, K), torch.float32, "scores out"),
                                         ((F, cap, D), torch.float32, "deltas out"),
                                         ((F,), torch.int32, "counts out")))
        got = ops.gather_rows(*ins, out=outs)
        arena.check("gather_rows, outputs 0x%02X" % out_fill)
        assert got[3].cpu().numpy().tolist() == [65, 0, 64, -1]
        for f in range(F):
            n = int(counts[f]) if ucounts[f] >= 0 else 0
            for g, w, what in zip(got[:3], want[:3], ("box rows", "scores", "deltas")):
                guarded.rows_equal(g[f, :n].cpu().numpy(), w[f, :n], what)
                guarded.assert_prefill(g[f, n:], out_fill, "%s of frame %d" % (what, f))


# --------------------------------------------------------------------------- engine
FRAME_HW = (160, 260)  # TEST.SCALE 256 / MAX_SIZE 416: im_scale 1.6, a 256 x 416 blob
NBOX, NDUP, CAP = 40, 10, 48


def _step_boxes(seed, F=2):
    """NBOX boxes per frame of which NDUP repeat earlier rows, in a CAP-row buffer."""
    rng = np.random.default_rng(seed)
    box_list = []
    for _ in range(F):
        b = gb._random_boxes(rng, NBOX, FRAME_HW)
        dst = rng.choice(np.arange(5, NBOX), NDUP, replace=False)
        b[dst] = b[rng.integers(0, 5, NDUP)]
        box_list.append(b)
    boxes, counts = _pack(box_list, cap=CAP)
    return boxes, counts


@pytest.fixture(scope="module")
def fast_setup():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.e2e_mask_rcnn_R_50_FPN_1x()
    cfg.MODEL.FASTER_RCNN = False
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = 256, 416
    vcfg.check_supported(cfg)
    frames = np.stack([np.random.RandomState(70 + r).randint(0, 256, FRAME_HW + (3,), np.uint8)
                       for r in range(2)])
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True,
                           calibrate_frame=frames[0])
    assert not hasattr(model, "RPN")
    pipe = FramePipeline(model, cfg, frame_hw=FRAME_HW, batch=2, device=DEV, channels_last=True)
    assert pipe.im_scale == 1.6
    return cfg, pipe, torch.from_numpy(frames).to(DEV)


def _check_step(cfg, pipe, out, boxes, counts, im_hw3):
    """The RoIs the box head saw, the detections' input after the gather and dets /
    classes / counts against the restatement chained with the oracle, per frame."""
    tst, K = cfg.TEST, cfg.MODEL.NUM_CLASSES
    F, cap = boxes.shape[:2]
    want = gb.rois_from_boxes(boxes, counts, [pipe.im_scale] * F, cfg.DEDUP_BOXES)
    got = [out[k].cpu().numpy() for k in ("rois", "roi_counts", "box_index", "box_inv_index")]
    _same(got, want, "the RoIs the box head saw")
    sc_u = out["cls_prob"].view(F, cap, K).cpu().numpy()
    dl_u = out["bbox_pred"].view(F, cap, 4 * K).cpu().numpy()
    gather = _gather_ref(boxes, sc_u, dl_u, want[2], want[3], counts, want[1])
    for k, w in zip(("det_rois", "det_cls_prob", "det_bbox_pred", "det_roi_counts"), gather):
        guarded.rows_equal(out[k].cpu().numpy(), w, k)
    total = 0
    for f in range(F):
        n, u = int(counts[f]), int(want[1][f])
        index, inv = want[2][f, :u], want[3][f, :n]
        pred = orc.clip_tiled_boxes(orc.bbox_transform(boxes[f][index], dl_u[f, :u],
                                                       tuple(cfg.MODEL.BBOX_REG_WEIGHTS)), im_hw3)
        s_ref, b_ref, cls_boxes = orc.box_results_with_nms_and_limit(
            sc_u[f, :u][inv], pred[inv], K, tst.SCORE_THRESH, tst.NMS, tst.DETECTIONS_PER_IM,
            nms_cross_class=tst.NMS_CROSS_CLASS, num_det_per_class_pre=tst.NUM_DET_PER_CLASS_PRE)
        k = out["counts_host"][f]
        assert k == len(s_ref), (f, k, len(s_ref))
        dets = out["dets"][f, :k].cpu().numpy()
        assert np.array_equal(dets[:, :4], b_ref) and np.array_equal(dets[:, 4], s_ref), f
        c_ref = np.concatenate([np.full(len(cls_boxes[j]), j) for j in range(1, K)])
        assert np.array_equal(out["classes"][f, :k].cpu().numpy(), c_ref), f
        total += k
    return total


def test_engine_step_matches_the_chained_restatement(fast_setup):
    cfg, pipe, frames = fast_setup
    boxes, counts = _step_boxes(1)
    out = pipe.run(frames, keep_intermediates=True, box_proposals=(_dev(boxes), _dev(counts)))
    assert out["roi_counts"].cpu().tolist() == [NBOX - NDUP] * 2
    assert _check_step(cfg, pipe, out, boxes, counts, FRAME_HW + (3,)) > 0
    assert out["masks"].shape[0] == sum(out["counts_host"])
    # duplicated rows carry bit-identical scores, deltas and boxes into the detections
    inv = out["box_inv_index"].cpu().numpy()
    for f in range(2):
        for u in np.unique(inv[f, :NBOX]):
            rows = np.flatnonzero(inv[f, :NBOX] == u)
            for k in ("det_cls_prob", "det_bbox_pred", "det_rois"):
                t = out[k][f, rows].cpu().numpy()
                assert (t.view(np.int32) == t.view(np.int32)[0]).all(), (k, f, u)
    assert any(len(np.flatnonzero(inv[0, :NBOX] == u)) > 1 for u in np.unique(inv[0, :NBOX]))


def test_engine_rules(fast_setup):
    from vosdetectron_amd import _lib, config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    cfg, pipe, frames = fast_setup
    with pytest.raises(ValueError, match="needs box_proposals"):
        pipe.run(frames)
    boxes, counts = _step_boxes(2)
    with pytest.raises(ValueError, match=r"\(\[F,cap,4\], \[F\]\)"):
        pipe.run(frames, box_proposals=(_dev(boxes[:1]), _dev(counts)))
    over = counts.copy()
    over[1] = CAP + 1
    with pytest.raises(_lib.VosdetError, match=r"frame\(s\) \[1\]"):
        pipe.run(frames, box_proposals=(_dev(boxes), _dev(over)))
    faster = vcfg.e2e_mask_rcnn_R_50_FPN_1x()
    faster.TEST.SCALE, faster.TEST.MAX_SIZE = 256, 416
    p2 = FramePipeline.__new__(FramePipeline)
    p2.given_boxes = False
    with pytest.raises(ValueError, match="MODEL.FASTER_RCNN True"):
        p2._check_box_proposals((_dev(boxes), _dev(counts)), frames)


def test_async_step_and_graph_replay_with_other_boxes(fast_setup):
    """run(sync=False) + complete() equals run(); a captured step replayed after other
    boxes were written into its box_proposals equals the eager step on those boxes."""
    cfg, pipe, frames = fast_setup
    keys = ("dets", "classes", "counts", "rois", "roi_counts", "box_index", "box_inv_index",
            "det_rois", "det_cls_prob", "det_bbox_pred", "det_roi_counts", "masks")
    b1, n1 = _step_boxes(3)
    b2, n2 = _step_boxes(4)
    n2[1] = NBOX - 7
    eager1 = pipe.run(frames, box_proposals=(_dev(b1), _dev(n1)))
    eager2 = pipe.run(frames, box_proposals=(_dev(b2), _dev(n2)))
    queued = pipe.run(frames, sync=False, box_proposals=(_dev(b1), _dev(n1)))
    assert "counts_host" not in queued
    done = pipe.complete(queued)
    assert done["counts_host"] == eager1["counts_host"] and sum(done["counts_host"]) > 0
    for k in keys:
        assert torch.equal(done[k], eager1[k]), k
    sb, sn = _dev(b1), _dev(n1)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pipe.run(frames, sync=False, box_proposals=(sb, sn))  # warm on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        gout = pipe.run(frames, sync=False, box_proposals=(sb, sn))
    torch.cuda.synchronize()
    assert "counts_host" not in gout  # no host read inside the captured step
    for b, n, eager in ((b2, n2, eager2), (b1, n1, eager1)):
        sb.copy_(_dev(b))
        sn.copy_(_dev(n))
        g.replay()
        torch.cuda.synchronize()
        out = pipe.complete(dict(gout))
        assert out["counts_host"] == eager["counts_host"]
        for k in keys:
            assert torch.equal(out[k], eager[k]), k


def test_vos_step_on_the_previous_steps_kept_rows():
    """VOSPipeline with MODEL.FASTER_RCNN False: step 0 on given boxes, finalize() leaves
    its kept rows on the device, step 1 takes them as box_proposals with no host read
    between the steps; step 1 matches the chained restatement."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import VOSPipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_davis")
    cfg.MODEL.FASTER_RCNN = False
    cfg.TEST.SCALE = 240
    hw = (240, 427)
    frames = [np.random.RandomState(300 + i).randint(0, 256, hw + (3,), np.uint8)
              for i in range(2)]
    model, _ = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=frames[0])
    pipe = VOSPipeline(model, cfg, frame_hw=hw, batch=1, device=DEV, channels_last=True,
                       det_cap=128)
    pipe.reset()
    rng = np.random.default_rng(9)
    b0 = gb._random_boxes(rng, 60, hw, 0.25)[None]
    out0 = pipe.run(_dev(frames[0][None]), sync=False,
                    box_proposals=(_dev(b0), _dev(np.array([60], np.int32))))
    pipe.finalize(out0)
    prev = (pipe.prev_dets[:, :, :4].contiguous(), pipe.prev_counts.clone())
    out1 = pipe.run(_dev(frames[1][None]), sync=False, keep_intermediates=True,
                    box_proposals=prev)
    pipe.complete(out1)
    boxes, counts = prev[0].cpu().numpy(), prev[1].cpu().numpy()
    assert counts[0] == pipe.complete(out0)["counts_host"][0] > 0
    assert _check_step(cfg, pipe, out1, boxes, counts, hw + (3,)) > 0
