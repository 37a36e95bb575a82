"""The box-path kernels inside guarded, poisoned buffers (tests/guarded.py; DESIGN
section 2, item 10): NMS, the RPN proposal chain, collect / distribute, the level map,
the mask-head batch, box detections with their options and post-filter, and the TTA
box union.

Every case is one problem instance with a reference from the oracle (never a second
run of the kernel), run with its workspace carved at exactly the bytes its size
function reports and pre-filled with 0x00, with 0xFF and with what a preceding larger
instance left in the same carve, into outputs pre-filled with 0x00 and with 0xFF.
After every call: (a) every canary byte around every carve is intact; (b) counts and
rows below the count equal the reference bit for bit; (c) rows from the count on
still hold the prefill byte for byte.  tests/test_guarded_cpu.py shows that each case
reaches the branch it is there for."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import guarded as G
from tests import guarded_cases as GC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_t, _np, _stream, sweep, rows_equal = G.to_dev, G.to_np, G.stream, G.sweep, G.rows_equal


@pytest.fixture(scope="module")
def arena():
    return G.Arena(DEV, 96 << 20)


# --------------------------------------------------------------------------- NMS
def _nms(arena, d, thresh, ws_fill, out_fill):
    """vd_nms as ops.nms calls it, with keep_out, num_out and the workspace carved."""
    from vosdetectron_amd._lib import check, lib
    n = len(d)
    dets = _t(d) if n else None
    keep = arena.carve((max(n, 1),), torch.int64, out_fill, "vd_nms keep_out", key="keep")
    num = arena.carve((1,), torch.int32, out_fill, "vd_nms num_out", key="num")
    wsb = lib().vd_nms_workspace_size(n)
    ws = arena.carve((wsb,), torch.uint8, ws_fill, "vd_nms workspace (%d bytes)" % wsb, key="ws")
    check(lib().vd_nms(dets.data_ptr() if n else None, n, 5, float(np.float32(thresh)),
                       keep.data_ptr(), num.data_ptr(), ws.data_ptr(), wsb, _stream()), "vd_nms")
    return keep, num


@pytest.mark.parametrize("n", [0] + GC.nms_sizes())
def test_nms(arena, n):
    """n = 0 writes num_out alone; 63 / 64 / 65 straddle one mask word; the two n around
    the in-LDS resolve's limit (whose copy of the whole mask includes the words
    nms_build_mask_rows never writes); kNmsMaxN."""
    thr = 0.5
    d = GC.nms_dets(n) if n else np.zeros((0, 5), np.float32)
    ref = orc.nms(d, thr) if n else np.zeros(0, np.int64)
    if n > 64:
        assert 1 < len(ref) < n  # suppression happens and leaves rows past the count
    big = GC.nms_dets(min(GC.nms_constants()[0], 2 * n + 70), seed=1)

    def verify(res, out_fill, tag):
        keep, num = res
        assert int(num.item()) == len(ref), tag
        rows_equal(_np(keep[:len(ref)]), ref, tag)
        G.assert_prefill(keep[len(ref):], out_fill, "vd_nms keep_out rows >= count, " + tag)

    sweep(arena, lambda w, o: _nms(arena, d, thr, w, o), lambda w, o: _nms(arena, big, thr, w, o),
          verify)


# --------------------------------------------------------------------------- proposals
def _proposals(arena, monkeypatch, inputs, pre, post, nms, min_size, ws_fill, out_fill):
    from vosdetectron_amd import ops
    probs, deltas, anchors, scales, info = inputs
    N, L = probs[0].shape[0], len(probs)
    log = G.guarded_ws(monkeypatch, arena, ws_fill, reuse=True, strip=lambda nb: nb // (N * L))
    out = (arena.carve((N, L, post, 5), torch.float32, out_fill, "proposals rois", key="rois"),
           arena.carve((N, L, post), torch.float32, out_fill, "proposals probs", key="probs"),
           arena.carve((N, L), torch.int32, out_fill, "proposals counts", key="counts"))
    got = ops.generate_proposals([_t(p) for p in probs], [_t(d) for d in deltas],
                                 [_t(a) for a in anchors], list(scales), _t(info), pre, post,
                                 nms, min_size, out=out)
    assert all(g is o for g, o in zip(got, out)) and len(log) == 1
    return out, log


def _rpn_env(monkeypatch, env):
    for k in GC.RPN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name", [n for n in GC.RPN_CASES if n != GC.RPN_LEFTOVER])
def test_generate_proposals(arena, monkeypatch, name):
    """Two images with different im_info rows (the slot stride) through every slot
    layout: small split / unsplit, with and without the multi-workgroup select, the
    LDS mask build, no NMS, pre < 64, large by pre and by take-all, all scores tied,
    everything filtered (counts 0, no row written)."""
    levels, pre, post, nms, min_size, env, _ = GC.RPN_CASES[name]
    ref = GC.rpn_reference(name)
    src = GC.RPN_CASES[GC.RPN_LEFTOVER]
    offsets = []

    def small(w, o):
        _rpn_env(monkeypatch, env)
        out, log = _proposals(arena, monkeypatch, GC.rpn_inputs(name), pre, post, nms, min_size,
                              w, o)
        offsets.append(log[0])
        return out

    def large(w, o):
        _rpn_env(monkeypatch, env)
        out, log = _proposals(arena, monkeypatch, GC.rpn_inputs(GC.RPN_LEFTOVER), src[1], src[2],
                              src[3], src[4], w, o)
        offsets.append(log[0])
        assert int(out[2].min()) > 0

    def verify(res, out_fill, tag):
        rois, probs, counts = res
        cnt = _np(counts)
        for l in range(len(levels)):
            for i in range(2):
                r, p = ref[l][i]
                what = "%s level %d image %d, %s" % (name, l, i, tag)
                assert cnt[i, l] == len(r), (what, cnt[i, l], len(r))
                rows_equal(_np(rois[i, l, :len(r)]), r, what + " rois")
                rows_equal(_np(probs[i, l, :len(r)]), p, what + " probs")
                G.assert_prefill(rois[i, l, len(r):], out_fill, what + " rois rows >= count")
                G.assert_prefill(probs[i, l, len(r):], out_fill, what + " probs rows >= count")

    sweep(arena, small, large, verify)
    # the leftover runs did reuse the larger instance's workspace carve
    pairs = [(a, b) for a, b in zip(offsets, offsets[1:]) if a[1] > b[1]]
    assert len(pairs) >= 2 and all(a[2] == b[2] for a, b in pairs), offsets


def test_generate_proposals_refuses_the_unplannable_level(arena, monkeypatch):
    """pre_nms_topN = 0 on (15, 24, 24): take-all of 8640 anchors is past the large
    variant's kPreMaxL = 8192 rows.  The entry refuses it (VD_ERR_SHAPE) whatever the
    workspace, and writes nothing."""
    from vosdetectron_amd import _lib
    levels, pre, post, nms, min_size = GC.RPN_REFUSED
    monkeypatch.setitem(GC.RPN_CASES, "refused", GC.RPN_REFUSED + ({}, "random"))
    inputs = GC.rpn_inputs("refused")
    for out_fill in G.FILLS:
        arena.reset()
        _rpn_env(monkeypatch, {})
        G.guarded_ws(monkeypatch, arena, G.ONES)
        out = (arena.carve((2, 1, post, 5), torch.float32, out_fill, "refused rois"),
               arena.carve((2, 1, post), torch.float32, out_fill, "refused probs"),
               arena.carve((2, 1), torch.int32, out_fill, "refused counts"))
        from vosdetectron_amd import ops
        with pytest.raises(_lib.VosdetError, match="unsupported shape"):
            ops.generate_proposals([_t(inputs[0][0])], [_t(inputs[1][0])], [_t(inputs[2][0])],
                                   list(inputs[3]), _t(inputs[4]), pre, post, nms, min_size,
                                   out=out)
        arena.check("refused level")
        for o in out:
            G.assert_prefill(o, out_fill, "outputs of the refused call")


def test_generate_proposals_failed_select_leaves_the_rows(arena, monkeypatch):
    """The one-workgroup select (VOSDET_RPN_PRESEL=0) on the score map it cannot
    bracket: that image's count is -1 and none of its rows is written; the other
    image of the launch equals the oracle."""
    p, d, an, scale, info = GC.rpn_unbracketable()
    ref_r, ref_p = orc.generate_proposals(an, scale, p[:1], d[:1], info[:1], 1000, 300, 0.7, 0)
    src = GC.RPN_CASES[GC.RPN_LEFTOVER]
    env = {"VOSDET_RPN_PRESEL": "0"}
    offsets = []

    def small(w, o):
        _rpn_env(monkeypatch, env)
        out, log = _proposals(arena, monkeypatch, ([p], [d], [an], [scale], info), 1000, 300, 0.7,
                              0, w, o)
        offsets.append(log[0])
        return out

    def large(w, o):
        _rpn_env(monkeypatch, env)
        out, log = _proposals(arena, monkeypatch, GC.rpn_inputs(GC.RPN_LEFTOVER), src[1], src[2],
                              src[3], src[4], w, o)
        offsets.append(log[0])
        assert int(out[2].min()) > 0

    def verify(res, out_fill, tag):
        rois, probs, counts = res
        assert _np(counts).tolist() == [[len(ref_r)], [-1]], tag
        rows_equal(_np(rois[0, 0, :len(ref_r)]), ref_r, tag + " image 0 rois")
        rows_equal(_np(probs[0, 0, :len(ref_r)]), ref_p[:, 0], tag + " image 0 probs")
        G.assert_prefill(rois[0, 0, len(ref_r):], out_fill, tag + " image 0 rows >= count")
        G.assert_prefill(probs[0, 0, len(ref_r):], out_fill, tag + " image 0 probs >= count")
        G.assert_prefill(rois[1], out_fill, tag + " the failed image's rois")
        G.assert_prefill(probs[1], out_fill, tag + " the failed image's probs")

    sweep(arena, small, large, verify)
    pairs = [(a, b) for a, b in zip(offsets, offsets[1:]) if a[1] > b[1]]
    assert len(pairs) >= 2 and all(a[2] == b[2] for a, b in pairs), offsets


# --------------------------------------------------------------------------- collect etc.
def _collect_inputs():
    """Four images x three levels of capacity 40: totals 0, 1, 80 (> post = 50), and
    one image with a failed level (-1)."""
    rng = np.random.default_rng(41)
    N, L, cap = 4, 3, 40
    counts = np.array([[0, 0, 0], [0, 1, 0], [40, 30, 10], [12, -1, 3]], np.int32)
    xy = rng.uniform(0, 600, (N, L, cap, 2))
    wh = np.exp(rng.uniform(np.log(8), np.log(500), (N, L, cap, 2)))
    rois = np.concatenate([np.zeros((N, L, cap, 1)), xy, xy + wh], -1).astype(np.float32)
    rois[..., 0] = np.arange(N)[:, None, None]
    probs = (np.round(rng.uniform(0, 1, (N, L, cap)) * 64) / 64).astype(np.float32)  # ties
    return rois, probs, counts


def test_collect_distribute(arena):
    from vosdetectron_amd import ops
    rois, probs, counts = _collect_inputs()
    N, L, cap = probs.shape
    post = 50
    for out_fill in G.FILLS:
        arena.reset()
        out = (arena.carve((N, post, 5), torch.float32, out_fill, "collect rois"),
               arena.carve((N, post), torch.int32, out_fill, "collect levels"),
               arena.carve((N,), torch.int32, out_fill, "collect counts"))
        ops.collect_distribute(_t(rois), _t(probs), _t(counts), post, 2, 5, out=out)
        arena.check("collect_distribute")
        cr, clv, ccnt = out
        want_cnt = []
        for i in range(N):
            if (counts[i] < 0).any():
                want_cnt.append(-1)
                n = 0
            else:
                col = orc.collect([rois[i, l, :counts[i, l]] for l in range(L)],
                                  [probs[i, l, :counts[i, l], None] for l in range(L)], post)
                n = len(col)
                want_cnt.append(n)
                rows_equal(_np(cr[i, :n]), col, "image %d rois" % i)
                lv = orc.map_rois_to_fpn_levels(col[:, 1:5], 2, 5).astype(np.int32) - 2
                rows_equal(_np(clv[i, :n]), lv, "image %d levels" % i)
            G.assert_prefill(cr[i, n:], out_fill, "collect rois rows >= count, image %d" % i)
            G.assert_prefill(clv[i, n:], out_fill, "collect levels rows >= count, image %d" % i)
        assert _np(ccnt).tolist() == want_cnt == [0, 1, 50, -1]


def test_map_rois_to_fpn_levels(arena):
    from vosdetectron_amd._lib import check, lib
    rng = np.random.default_rng(43)
    R = 77
    xy = rng.uniform(0, 600, (R, 2))
    wh = np.exp(rng.uniform(np.log(2), np.log(900), (R, 2)))
    rois = np.hstack([np.zeros((R, 1)), xy, xy + wh]).astype(np.float32)
    want = orc.map_rois_to_fpn_levels(rois[:, 1:5], 2, 5).astype(np.int32)
    for out_fill in G.FILLS:
        arena.reset()
        out = arena.carve((R,), torch.int32, out_fill, "vd_map_rois_to_fpn_levels out")
        r = _t(rois)
        check(lib().vd_map_rois_to_fpn_levels(r.data_ptr(), 5, 1, R, 2, 5, 224., 4.,
                                              out.data_ptr(), _stream()), "levels")
        arena.check("map_rois_to_fpn_levels")
        rows_equal(_np(out), want, "levels")


def _mask_rois_reference(dets, classes, counts, scales, row0, rows, k_min, k_max):
    """im_detect_mask's _get_rois_blob + _add_multilevel_rois_for_test over the frames'
    detections, rows [row0, row0 + rows); past the total the padding row (frame 0, a
    zero box, level 0, class 1)."""
    F, D = classes.shape
    r, c = [], []
    for f in range(F):
        n = min(max(int(counts[f]), 0), D)
        b = (dets[f, :n, :4].astype(np.float64) * scales[f]).astype(np.float32)
        r.append(np.hstack([np.full((n, 1), f, np.float32), b]))
        c.append(classes[f, :n])
    r, c = np.concatenate(r), np.concatenate(c)
    lv = orc.map_rois_to_fpn_levels(r[:, 1:5], k_min, k_max).astype(np.int32) - k_min
    total = len(r)
    pad = max(row0 + rows - total, 0)
    r = np.concatenate([r, np.zeros((pad, 5), np.float32)])[row0:row0 + rows]
    lv = np.concatenate([lv, np.zeros(pad, np.int32)])[row0:row0 + rows]
    c = np.concatenate([c, np.ones(pad, np.int32)])[row0:row0 + rows]
    return r, lv, c.astype(np.int32), total


@pytest.mark.parametrize("row0,rows", [(0, 40), (7, 16), (30, 8)])
def test_mask_rois(arena, row0, rows):
    """Frames with 0, 1, more than det_cap (clamped) and -1 detections; the window
    [row0, row0 + rows) starts at 0, inside a frame, and past the total (all padding).
    The whole output is defined: the kernel writes the padding rows itself."""
    from vosdetectron_amd._lib import check, lib
    rng = np.random.default_rng(47)
    F, D = 5, 12
    counts = np.array([0, 1, D + 5, -1, 9], np.int32)
    xy = rng.uniform(0, 500, (F, D, 2))
    wh = np.exp(rng.uniform(np.log(4), np.log(400), (F, D, 2)))
    dets = np.concatenate([xy, xy + wh, rng.uniform(0, 1, (F, D, 1))], -1).astype(np.float32)
    classes = rng.integers(1, 81, (F, D)).astype(np.int32)
    scales = np.array([1.0, 1.6, 0.7, 1.0, 2.25 / 1.1], np.float64)
    want = _mask_rois_reference(dets, classes, counts, scales, row0, rows, 2, 5)
    assert want[3] == 22
    d, c, n, sc = _t(dets), _t(classes), _t(counts), _t(scales)
    for out_fill in G.FILLS:
        arena.reset()
        rois = arena.carve((rows, 5), torch.float32, out_fill, "vd_mask_rois rois")
        lvl = arena.carve((rows,), torch.int32, out_fill, "vd_mask_rois levels")
        cls = arena.carve((rows,), torch.int32, out_fill, "vd_mask_rois classes")
        total = arena.carve((1,), torch.int32, out_fill, "vd_mask_rois total")
        check(lib().vd_mask_rois(d.data_ptr(), c.data_ptr(), n.data_ptr(), F, D, sc.data_ptr(),
                                 row0, rows, 2, 5, 224., 4., rois.data_ptr(), lvl.data_ptr(),
                                 cls.data_ptr(), total.data_ptr(), _stream()), "vd_mask_rois")
        arena.check("vd_mask_rois row0 = %d" % row0)
        rows_equal(_np(rois), want[0], "rois")
        rows_equal(_np(lvl), want[1], "levels")
        rows_equal(_np(cls), want[2], "classes")
        assert int(total.item()) == want[3]


# --------------------------------------------------------------------------- detections
def _detections(arena, monkeypatch, name, ws_fill, out_fill, inputs=None, **kw):
    from vosdetectron_amd import ops
    N, R, K, _, per_im, det_cap, thr = GC.DET_CASES[name]
    rois, cls, pred, counts = inputs or GC.det_inputs(name)
    log = G.guarded_ws(monkeypatch, arena, ws_fill, reuse=True,
                       strip=lambda nb: nb // (3 * N * K))
    out = (arena.carve((N, det_cap, 5), torch.float32, out_fill, "detections dets", key="dets"),
           arena.carve((N, det_cap), torch.int32, out_fill, "detections classes", key="cls"),
           arena.carve((N,), torch.int32, out_fill, "detections counts", key="cnt"))
    hw = torch.tensor([list(GC.DET_IM)] * N, dtype=torch.int32, device=DEV)
    ops.box_detections(_t(rois), _t(cls), _t(pred), _t(counts), torch.ones(N, device=DEV), hw,
                       score_thresh=thr, dets_per_im=per_im, det_cap=det_cap, out=out, **kw)
    assert len(log) == 1
    return out


def _det_leftover(name):
    """A larger instance for the same carves: more proposals, one more class... of the
    same images (the workspace grows with R, N and K)."""
    N, R, K = GC.DET_CASES[name][:3]
    rng = np.random.default_rng(3)
    R2 = min(2048, R + 150) if R < 2048 else R
    rois = np.zeros((N, R2, 5), np.float32)
    xy = rng.uniform(0, 700, (N, R2, 2))
    rois[..., 1:3] = xy
    rois[..., 3:5] = xy + rng.uniform(8, 100, (N, R2, 2))
    cls = rng.uniform(0, 1, (N, R2, K + 1)).astype(np.float32)
    pred = rng.normal(0, 1, (N, R2, 4 * (K + 1))).astype(np.float32)
    return (N, R2, K + 1), (rois, cls, pred, np.full(N, R2, np.int32))


def _verify_detections(name, oracle_kw=None, exact_rows=True):
    N, K = GC.DET_CASES[name][0], GC.DET_CASES[name][2]
    refs = [GC.det_reference(name, i, **(oracle_kw or {})) for i in range(N)]

    def verify(res, out_fill, tag):
        dets, cls, cnt = res
        for i in range(N):
            s, b, c, _ = refs[i]
            what = "%s image %d, %s" % (name, i, tag)
            assert int(cnt[i].item()) == len(s), (what, int(cnt[i].item()), len(s))
            rows_equal(_np(dets[i, :len(s), :4]), b, what + " boxes")
            rows_equal(_np(dets[i, :len(s), 4]), s, what + " scores")
            rows_equal(_np(cls[i, :len(s)]), c, what + " classes")
            G.assert_prefill(dets[i, len(s):], out_fill, what + " dets rows >= count")
            G.assert_prefill(cls[i, len(s):], out_fill, what + " classes rows >= count")
    return verify


def _det_large(arena, monkeypatch, name, **opts):
    """The larger instance that leaves the leftover, through the same wrapper options."""
    from vosdetectron_amd import ops
    (N2, R2, K2), big = _det_leftover(name)

    def large(w, o):
        log = G.guarded_ws(monkeypatch, arena, w, reuse=True, strip=lambda nb: nb // (3 * N2 * K2))
        hw = torch.tensor([list(GC.DET_IM)] * N2, dtype=torch.int32, device=DEV)
        out = ops.box_detections(*[_t(x) for x in big], torch.ones(N2, device=DEV), hw,
                                 det_cap=64, **opts)
        assert int(out[2].min()) > 0 and len(log) == 1
    return large


@pytest.mark.parametrize("name", list(GC.DET_CASES))
def test_box_detections(arena, monkeypatch, name):
    """(N, R, K) of (2, 65, 3), (2, 1000, 5), (1, 2048, 2 -- kDetRMax): roi_count below
    R and 0 for one image, more survivors than dets_per_im = det_cap, nothing above the
    score threshold."""
    sweep(arena, lambda w, o: _detections(arena, monkeypatch, name, w, o),
          _det_large(arena, monkeypatch, name), _verify_detections(name))


@pytest.mark.parametrize("opts", [dict(soft_nms="linear"), dict(soft_nms="gaussian"),
                                  dict(bbox_vote="ID"), dict(bbox_vote="AVG"),
                                  dict(bbox_vote="IOU_AVG"),
                                  dict(soft_nms="linear", bbox_vote="AVG")],
                         ids=lambda o: "-".join("%s" % v for v in o.values()))
def test_box_detections_ex(arena, monkeypatch, opts):
    """vd_box_detections_ex: soft-NMS and box voting on the (2, 65, 3) case, the leftover
    from a larger instance through the same options."""
    name = "r65"
    okw = {}
    if "soft_nms" in opts:
        okw["soft_nms_method"] = opts["soft_nms"]
    if "bbox_vote" in opts:
        okw.update(bbox_vote=opts["bbox_vote"], bbox_vote_th=0.8)
    sweep(arena, lambda w, o: _detections(arena, monkeypatch, name, w, o, **opts),
          _det_large(arena, monkeypatch, name, **opts), _verify_detections(name, okw))


@pytest.mark.parametrize("cross,pre", [(0.3, 0), (0.0, 2), (0.5, 1)])
def test_detections_postfilter(arena, monkeypatch, cross, pre):
    """Cross-class NMS and NUM_DET_PER_CLASS_PRE compact the rows in place.  The rows
    past the count vd_box_detections reported keep the prefill.  The rows between the
    new and that old count are unspecified (they hold rows of the unfiltered list):
    every consumer in engine.py, c4.py and runner.py indexes the detections by the
    count, so only the defined region is compared there."""
    name = "r65"
    N = GC.DET_CASES[name][0]
    okw = dict(nms_cross_class=cross, num_det_per_class_pre=pre)
    before = [len(GC.det_reference(name, i)[0]) for i in range(N)]
    refs = [GC.det_reference(name, i, **okw) for i in range(N)]
    assert len(refs[0][0]) < before[0]

    def verify(res, out_fill, tag):
        dets, cls, cnt = res
        for i in range(N):
            s, b, c, _ = refs[i]
            assert int(cnt[i].item()) == len(s), tag
            rows_equal(_np(dets[i, :len(s), :4]), b, tag + " boxes")
            rows_equal(_np(dets[i, :len(s), 4]), s, tag + " scores")
            rows_equal(_np(cls[i, :len(s)]), c, tag + " classes")
            G.assert_prefill(dets[i, before[i]:], out_fill, tag + " dets rows >= the old count")
            G.assert_prefill(cls[i, before[i]:], out_fill, tag + " classes rows >= the old count")

    sweep(arena, lambda w, o: _detections(arena, monkeypatch, name, w, o, **okw),
          _det_large(arena, monkeypatch, name), verify)


# --------------------------------------------------------------------------- union
def _union(arena, monkeypatch, cand_cap, ws_fill, out_fill, det_cap=64):
    """BoxUnion over the two views (the second through vd_box_union_add_view_ar);
    _ws is patched before the object is constructed."""
    from vosdetectron_amd import ops
    u = GC.UNION
    rois, cls, pred, counts = GC.union_inputs()
    F, K = u["F"], u["K"]
    log = G.guarded_ws(monkeypatch, arena, ws_fill, reuse=True, strip=lambda nb: nb // (F * K))
    bu = ops.BoxUnion(cand_cap, F, K, DEV)
    assert len(log) == 1
    H = u["im"][0]
    for t in range(u["T"]):
        ar = u["ar"][t]
        hw = torch.tensor([[H, GC.union_view_width(t)]] * F, dtype=torch.int32, device=DEV)
        bu.add_view(_t(rois[t]), _t(cls[t]), _t(pred[t]), _t(counts[t]),
                    torch.full((F,), u["scales"][t], dtype=torch.float32, device=DEV), hw,
                    u["hflip"][t], x_inv=None if ar is None else np.float32(1.0 / ar))
        arena.check("add_view %d at cand_cap %d" % (t, cand_cap))
    out = (arena.carve((F, det_cap, 5), torch.float32, out_fill, "union dets", key="dets"),
           arena.carve((F, det_cap), torch.int32, out_fill, "union classes", key="cls"),
           arena.carve((F,), torch.int32, out_fill, "union counts", key="cnt"),
           arena.carve((F, K), torch.int32, out_fill, "union cand_counts", key="cand"))
    bu.detections(det_cap=det_cap, out=out[:3], cand_counts=out[3])
    return out


def test_box_union(arena, monkeypatch):
    """At big_cap every list fits: both images equal the oracle.  At cand_cap class 1 of
    image 0 overflows in the second view: that image's count is -1 and none of its
    rows is written; image 1 is unharmed.  The small cap runs in the carve the big one
    left (the leftover mode)."""
    u = GC.UNION
    refs = [GC.union_reference(i) for i in range(u["F"])]

    def verify_image(res, i, out_fill, tag):
        dets, cls, cnt, cand = res
        s, b, c, n_cand = refs[i]
        assert int(cnt[i].item()) == len(s), tag
        rows_equal(_np(dets[i, :len(s), :4]), b, tag + " boxes")
        rows_equal(_np(dets[i, :len(s), 4]), s, tag + " scores")
        rows_equal(_np(cls[i, :len(s)]), c, tag + " classes")
        G.assert_prefill(dets[i, len(s):], out_fill, tag + " dets rows >= count")
        G.assert_prefill(cls[i, len(s):], out_fill, tag + " classes rows >= count")
        assert _np(cand[i, 1:]).tolist() == n_cand.tolist(), tag

    def verify(res, out_fill, tag):
        dets, cls, cnt, cand = res
        assert int(cnt[0].item()) == -1, tag
        G.assert_prefill(dets[0], out_fill, tag + " the overflowed image's dets")
        G.assert_prefill(cls[0], out_fill, tag + " the overflowed image's classes")
        verify_image(res, 1, out_fill, tag)

    def large(w, o):
        res = _union(arena, monkeypatch, u["big_cap"], w, o)
        arena.check("big_cap")
        for i in range(u["F"]):
            verify_image(res, i, o, "big_cap image %d" % i)

    sweep(arena, lambda w, o: _union(arena, monkeypatch, u["cand_cap"], w, o), large, verify)
    for fill in G.FILLS:  # the fitting capacity on fresh fills too
        arena.reset()
        large(fill, G.ONES)


# --------------------------------------------------------------------------- soft-NMS, voting
@pytest.mark.parametrize("method", ["linear", "gaussian", "hard"])
def test_soft_nms_standalone(arena, method):
    """vd_soft_nms as ops.soft_nms calls it: out [n, 5], keep [n] and the count carved;
    rows the decay drops below the score threshold leave rows past the count."""
    from vosdetectron_amd import ops
    from vosdetectron_amd._lib import check, lib
    d = GC.nms_dets(65)
    d[:, 4] = np.linspace(0.0002, 0.9, 65, dtype=np.float32)
    ref_rows, ref_keep = orc.soft_nms(d, 0.5, 0.3, 0.001, method)
    assert 0 < len(ref_keep) < len(d)
    dt = _t(d)
    for out_fill in G.FILLS:
        arena.reset()
        out = arena.carve((65, 5), torch.float32, out_fill, "vd_soft_nms out")
        keep = arena.carve((65,), torch.int64, out_fill, "vd_soft_nms keep")
        num = arena.carve((1,), torch.int32, out_fill, "vd_soft_nms count")
        check(lib().vd_soft_nms(dt.data_ptr(), 65, 5, 0.5, float(np.float32(0.3)),
                                float(np.float32(0.001)), ops.SOFT_NMS_METHODS[method],
                                out.data_ptr(), keep.data_ptr(), num.data_ptr(), _stream()),
              "vd_soft_nms")
        arena.check("vd_soft_nms " + method)
        k = len(ref_keep)
        assert int(num.item()) == k
        rows_equal(_np(out[:k]), np.ascontiguousarray(ref_rows, np.float32), "soft_nms rows")
        rows_equal(_np(keep[:k]), np.asarray(ref_keep, np.int64), "soft_nms keep")
        G.assert_prefill(out[k:], out_fill, "vd_soft_nms out rows >= count")
        G.assert_prefill(keep[k:], out_fill, "vd_soft_nms keep rows >= count")


@pytest.mark.parametrize("method", ["ID", "AVG", "IOU_AVG"])
def test_box_voting_standalone(arena, method):
    """vd_box_voting as ops.box_voting calls it: every one of the n_top rows is defined."""
    from vosdetectron_amd import ops
    from vosdetectron_amd._lib import check, lib
    d = GC.nms_dets(65)
    top = d[orc.nms(d, 0.5)]
    want = orc.box_voting(top, d, 0.8, method, 1.0)
    tt, at = _t(top), _t(d)
    for out_fill in G.FILLS:
        arena.reset()
        out = arena.carve((len(top), 5), torch.float32, out_fill, "vd_box_voting out")
        check(lib().vd_box_voting(tt.data_ptr(), len(top), 5, at.data_ptr(), 65, 5,
                                  float(np.float32(0.8)), ops.bbox_vote_method(method, 1.0), 1.0,
                                  out.data_ptr(), _stream()), "vd_box_voting")
        arena.check("vd_box_voting " + method)
        rows_equal(_np(out), np.ascontiguousarray(want, np.float32), "voted rows")
