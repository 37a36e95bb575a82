"""keypoint_results' OKS NMS on the device (vd_nms_oks_frames / vd_compute_oks).

1. The kernels on the executed reference's fixture (tests/golden/nms_oks.npz), several
   frames per launch: keep, counts and scores exactly; the gathered rows bit for bit.
2. vd_compute_oks against every ovr vector the reference's loop evaluated, within 1e-12
   absolute: the argument of every exp is bit-identical by construction (float32
   differences and squares, two correctly rounded float64 divisions, an exact halving),
   both exps are good to a few ulp on values <= 1, so each term and the mean of 17 are
   within ~1e-15 -- three orders of slack, six below the fixture's decision margin.
3. KeypointFramePipeline(nms_oks=...): off is bit-equal to a pipeline built without the
   argument; on, the outputs equal the restatement (tests/oks_ref.py) run on the step's
   own pre-NMS tensors, at 0.3 and at a threshold picked from the data; frame_keypoints,
   graph replay and the result gather.
Reference: lib/utils/keypoints.py:225-266, lib/core/test.py:864-870."""
import numpy as np
import pytest
import torch

from tests import oks_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAME = "e2e_keypoint_rcnn_R-50-FPN_1x"
f32 = np.float32


@pytest.fixture(scope="module")
def fixture():
    thresh, _, cases = oks_ref.fixture_cases()
    return thresh, {c["n"]: c for c in cases}


def _pack(cases, frames, D, seed):
    """frames: per frame a case's n, 0 (empty) or a negative failure code.  Returns the
    host arrays of one launch; keyps carries five rows of junk past the total."""
    rng = np.random.default_rng(seed)
    F = len(frames)
    counts = np.asarray(frames, np.int32)
    dets = rng.uniform(0, 50, (F, D, 5)).astype(f32)  # junk past the counts, never read
    cls = rng.integers(1, 80, (F, D)).astype(np.int32)
    kps = []
    for f, n in enumerate(frames):
        if n > 0:
            dets[f, :n, :4] = cases[n]["rois"]
            kps.append(cases[n]["kp"])
    kps.append(rng.uniform(0, 100, (5, 4, 17)).astype(f32))
    return np.concatenate(kps), dets, cls, counts


LAUNCHES = {"d256": ([0, 1, 17, 100, -1, 65, 2, 12, 16, 64], 256),
            "d512": ([256, -2, 300], 512)}


@pytest.fixture(scope="module")
def launches(fixture):
    """Both launches run once: host inputs, the device result, the inputs after it."""
    from vosdetectron_amd import ops
    thresh, cases = fixture
    res = {}
    for i, (name, (frames, D)) in enumerate(LAUNCHES.items()):
        host = _pack(cases, frames, D, 40 + i)
        dev = [torch.from_numpy(a).to(DEV) for a in host]
        r = ops.nms_oks_frames(*dev, thresh=thresh)
        torch.cuda.synchronize()
        res[name] = (frames, D, host, {k: getattr(r, k).cpu().numpy() for k in r._fields},
                     [t.cpu().numpy() for t in dev])
    return res


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_frames_match_executed_reference(fixture, launches, name):
    thresh, cases = fixture
    frames, D, (keyps, dets, cls, counts), got, after = launches[name]
    for a, b in zip((keyps, dets, cls, counts), after):
        assert np.array_equal(a, b)  # the inputs are not modified
    assert got["keep"].shape == (len(frames), D) and got["keep"].dtype == np.int32
    src = dst = 0
    for f, n in enumerate(frames):
        if n <= 0:
            assert got["counts"][f] == n  # empty, or the failure code passed through
            assert np.all(got["keep"][f] == -1) and not got["dets"][f].any()
            assert not got["classes"][f].any() and not got["scores"][f].any()
            continue
        c = cases[n]
        keep = c["keep"]
        k = len(keep)
        assert got["counts"][f] == k, (n, got["counts"][f], k)
        assert got["keep"][f, :k].tolist() == keep.tolist(), n
        assert np.all(got["keep"][f, k:] == -1)
        assert np.array_equal(got["scores"][f, :n].view(np.uint32), c["scores"].view(np.uint32))
        assert not got["scores"][f, n:].any()
        assert np.array_equal(got["dets"][f, :k], dets[f, keep]) and not got["dets"][f, k:].any()
        assert np.array_equal(got["classes"][f, :k], cls[f, keep])
        assert not got["classes"][f, k:].any()
        assert np.array_equal(got["keyps"][dst:dst + k], keyps[src:src + n][keep])
        src += n
        dst += k
    assert got["keyps"].shape == keyps.shape and not got["keyps"][dst:].any()
    # the restatement of the whole launch agrees, output for output
    ref = oks_ref.nms_oks_frames(keyps, dets, cls, counts, thresh)
    for key in ("keep", "counts", "dets", "classes", "keyps", "scores"):
        assert np.array_equal(got[key], ref[key]), key


def test_tie_case_keeps_the_documented_order(fixture, launches):
    """Equal scores: the higher index is processed first (rows 7 / 9 carry the logits of
    rows 2 / 4 and a pose beside theirs, so exactly the later-processed one is dropped)."""
    thresh, cases = fixture
    frames, D, host, got, _ = launches["d256"]
    f = frames.index(12)
    keep = got["keep"][f, :got["counts"][f]].tolist()
    assert keep == cases[12]["keep"].tolist()
    assert 7 in keep and 9 in keep and 2 not in keep and 4 not in keep
    sc = got["scores"][f, :12]
    assert sc[2] == sc[7] and sc[4] == sc[9]


def test_rows_past_the_buffer_are_not_read(fixture):
    """A keyps buffer shorter than the counts' total (the pipeline's padded batch on an
    overflow step): the frames are cut to the rows present, nothing past them is read."""
    from vosdetectron_amd import ops
    thresh, cases = fixture
    keyps, dets, cls, counts = _pack(cases, [17, 16], 32, 7)
    short = keyps[:20]  # frame 1 has 3 of its 16 rows
    r = ops.nms_oks_frames(*[torch.from_numpy(a).to(DEV) for a in (short, dets, cls, counts)],
                           thresh=thresh)
    ref = oks_ref.nms_oks_frames(short, dets, cls, np.array([17, 3], np.int32), thresh)
    for key in ("keep", "counts", "dets", "classes", "keyps"):
        assert np.array_equal(getattr(r, key).cpu().numpy(), ref[key]), key
    with pytest.raises(ValueError, match="keyps has 20 rows"):
        ops.nms_oks_frames(*[torch.from_numpy(a).to(DEV) for a in (short, dets, cls, counts)],
                           counts_host=[17, 16])


def test_compute_oks_matches_every_recorded_vector(fixture):
    from vosdetectron_amd import keypoints, ops
    thresh, cases = fixture
    worst = 0.
    for n, c in cases.items():
        if not sum(len(v) for v in c["ovr"]):  # n = 1: one empty vector
            continue
        kp, rois = torch.from_numpy(c["kp"]).to(DEV), torch.from_numpy(c["rois"]).to(DEV)
        order = oks_ref.processing_order(c["scores"])
        outs = []
        for ovr in c["ovr"]:  # the reference's loop, its recorded decisions driving it
            rest = torch.from_numpy(order[1:].copy()).to(DEV)
            outs.append(ops.compute_oks(kp[order[0]], rois[order[0]], kp[rest]))
            assert outs[-1].dtype == torch.float64 and outs[-1].shape[0] == len(ovr)
            order = order[1:][ovr <= thresh]
        assert order.size == 0
        got = torch.cat(outs).cpu().numpy()
        err = float(np.abs(got - np.concatenate(c["ovr"])).max())
        worst = max(worst, err)
        assert err <= 1e-12, (n, err)
    print("compute_oks: max |device - executed reference| = %.3g" % worst)
    c = cases[17]
    out = keypoints.compute_oks(c["kp"][3], c["rois"][3], c["kp"][5:9], c["rois"][5:9])
    assert isinstance(out, np.ndarray) and out.dtype == np.float64
    assert float(np.abs(out - oks_ref.compute_oks(c["kp"][3], c["rois"][3], c["kp"][5:9])).max()) \
        <= 1e-12
    assert ops.compute_oks(torch.from_numpy(c["kp"][3]).to(DEV),
                           torch.from_numpy(c["rois"][3]).to(DEV),
                           torch.zeros(0, 4, 17, device=DEV)).shape == (0,)


def test_reference_named_nms_oks(fixture):
    from vosdetectron_amd import keypoints
    thresh, cases = fixture
    for n in (1, 12, 65, 300):
        c = cases[n]
        keep = keypoints.nms_oks(c["kp"], c["rois"], thresh)
        assert isinstance(keep, list) and all(type(i) is int for i in keep)
        assert keep == c["keep"].tolist()
    c = cases[100]
    t = keypoints.nms_oks(torch.from_numpy(c["kp"]).to(DEV), torch.from_numpy(c["rois"]).to(DEV),
                          thresh)
    assert t.is_cuda and t.dtype == torch.int64 and t.tolist() == c["keep"].tolist()
    assert keypoints.nms_oks(np.zeros((0, 4, 17), f32), np.zeros((0, 4), f32), thresh) == []


# --------------------------------------------------------------------------- #
def _pair_values(kp, rois):
    """compute_oks of every row against every other row of a frame (restatement)."""
    n = len(kp)
    v = [np.delete(oks_ref.compute_oks(kp[i], rois[i], kp), i) for i in range(n)]
    return np.concatenate(v) if v else np.zeros(0)


def _pick_threshold(kp, rois):
    """The midpoint of the widest gap between consecutive sorted pairwise values around
    their median: (threshold, margin).  "Around" is the central 80 % of the ranks.  The
    OKS of two unrelated poses is a mean of exp(-d^2 / ...) terms with d of the order of
    the box, so most pairwise values of a synthetic-weight step are astronomically small
    (on the seeded frames: median ~1e-58, 75th percentile ~1e-13, 90th ~1e-3), and a gap
    of 1e-9 between neighbours exists only from about the 80th percentile up; the
    window reaches the 90th so that the choice does not hang on one seed."""
    v = np.sort(_pair_values(kp, rois))
    lo, hi = len(v) // 10, 9 * len(v) // 10
    gaps = np.diff(v[lo:hi + 1])
    g = int(gaps.argmax())
    return float((v[lo + g] + v[lo + g + 1]) / 2), float(gaps[g] / 2)


@pytest.fixture(scope="module")
def oks_setup():
    """The R-50-FPN keypoint config with person as the only class, two 320 x 480 frames:
    the step without the argument, with nms_oks=None, at 0.3 and at a picked threshold."""
    import bench
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import KeypointFramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get(NAME)
    cfg.MODEL.NUM_CLASSES = 2
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True)
    kw = dict(frame_hw=(320, 480), batch=2, channels_last=True, device=DEV)
    frames = torch.from_numpy(bench.synthetic_frames(2, 21, 320, 480)).to(DEV)
    plain = KeypointFramePipeline(model, cfg, **kw).run(frames, keep_intermediates=True)
    none = KeypointFramePipeline(model, cfg, nms_oks=None, **kw).run(
        frames, keep_intermediates=True)
    pipe03 = KeypointFramePipeline(model, cfg, nms_oks=True, **kw)
    out03 = pipe03.run(frames, keep_intermediates=True)
    torch.cuda.synchronize()
    # the threshold for the second run, from the frame with the most detections
    pre = out03["counts_pre_oks_host"]
    f = int(np.argmax(pre))
    o = sum(pre[:f])
    kp = out03["keyps_pre_oks"][o:o + pre[f]].cpu().numpy()
    rois = out03["dets_pre_oks"][f, :pre[f], :4].cpu().numpy()
    thr, margin = _pick_threshold(kp, rois)
    pipe = KeypointFramePipeline(model, cfg, nms_oks=thr, **kw)
    out = pipe.run(frames, keep_intermediates=True)
    torch.cuda.synchronize()
    return dict(cfg=cfg, model=model, frames=frames, plain=plain, none=none, pipe03=pipe03,
                out03=out03, pipe=pipe, out=out, thr=thr, margin=margin, frame=f)


def test_pipeline_off_is_the_parent_step(oks_setup):
    plain, none = oks_setup["plain"], oks_setup["none"]
    assert set(plain) == set(none)
    assert not [k for k in plain if "oks" in k]
    assert plain["counts_host"] == none["counts_host"] and max(plain["counts_host"]) > 1
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, none[k]), k
    assert oks_setup["pipe03"].oks_thresh == 0.3


def _assert_step_equals_restatement(out, thr, plain):
    pre = out["counts_pre_oks_host"]
    assert pre == plain["counts_host"]
    # the pre-NMS tensors are the step without the NMS; the kps_* stay in that order
    for a, b in (("dets_pre_oks", "dets"), ("classes_pre_oks", "classes"),
                 ("counts_pre_oks", "counts"), ("keyps_pre_oks", "keyps"),
                 ("kps_rois", "kps_rois"), ("kps_boxes", "kps_boxes"),
                 ("kps_heatmaps", "kps_heatmaps"), ("kps_feat", "kps_feat")):
        assert torch.equal(out[a], plain[b]), a
    ref = oks_ref.nms_oks_frames(out["keyps_pre_oks"].cpu().numpy(),
                                 out["dets_pre_oks"].cpu().numpy(),
                                 out["classes_pre_oks"].cpu().numpy(),
                                 out["counts_pre_oks"].cpu().numpy(), thr)
    M = int(ref["counts"].sum())
    assert out["counts_host"] == ref["counts"].tolist()
    assert np.array_equal(out["counts"].cpu().numpy(), ref["counts"])
    assert np.array_equal(out["dets"].cpu().numpy(), ref["dets"])
    assert np.array_equal(out["classes"].cpu().numpy(), ref["classes"])
    assert np.array_equal(out["oks_keep"].cpu().numpy(), ref["keep"])
    assert tuple(out["keyps"].shape) == (M, 4, 17)
    assert np.array_equal(out["keyps"].cpu().numpy(), ref["keyps"][:M])
    return ref


def test_pipeline_at_reference_threshold(oks_setup):
    _assert_step_equals_restatement(oks_setup["out03"], 0.3, oks_setup["plain"])


def test_pipeline_at_picked_threshold(oks_setup):
    """Synthetic weights give near-random poses whose OKS is far below 0.3, so the second
    run's threshold comes from the data: some rows are suppressed, not all, and the
    decision margin is the widest available."""
    s = oks_setup
    print("picked threshold %.17g, margin %.3g" % (s["thr"], s["margin"]))
    assert s["margin"] >= 1e-9
    ref = _assert_step_equals_restatement(s["out"], s["thr"], s["plain"])
    f = s["frame"]
    n, k = s["out"]["counts_pre_oks_host"][f], int(ref["counts"][f])
    assert 1 < k < n, (k, n)


def test_frame_keypoints_groups_by_the_new_counts(oks_setup):
    from vosdetectron_amd.engine import frame_keypoints
    s = oks_setup
    out, ks = s["out"], s["out"]["counts_host"]
    res = frame_keypoints(s["pipe"], out)
    kp = out["keyps"].cpu().numpy()
    assert len(res) == 2 and kp.shape[0] == sum(ks) < sum(out["counts_pre_oks_host"])
    o = 0
    for f, k in enumerate(ks):
        assert [len(c) for c in res[f]] == [0, k]
        for i in range(k):
            assert np.array_equal(res[f][1][i], kp[o + i])
        o += k
    s["pipe"].enable_timers()
    s["pipe"].run(s["frames"])
    assert {"misc_keypoints", "misc_oks_nms"} <= set(s["pipe"].timer_summary())
    s["pipe"].enable_timers(False)


def test_pipeline_graph_replay_with_oks(oks_setup):
    s = oks_setup
    pipe, eager = s["pipe"], s["out"]
    x = s["frames"].clone()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        pipe.run(x, sync=False)  # warm on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=st):
        gout = pipe.run(x, sync=False)
    torch.cuda.synchronize()
    assert "counts_host" not in gout  # no host read inside the captured step
    for _ in range(2):
        for k in ("keyps", "dets", "classes", "counts", "oks_keep"):
            gout[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        out = pipe.complete(dict(gout))
        assert out["counts_host"] == eager["counts_host"]
        for k in ("dets", "classes", "counts", "keyps", "oks_keep", "kps_rois"):
            assert torch.equal(out[k], eager[k]), k


def test_complete_runs_the_rows_past_the_padded_batch_with_oks(oks_setup, monkeypatch):
    """A padded batch shorter than the detections, with nms_oks: complete() decodes the
    rest and runs the NMS again on the full set.  The pre-NMS rows are the full run's;
    the result is ops.nms_oks_frames of this run's own pre-NMS tensors, whatever
    algorithm the head's deconvolution picks for the other batch size."""
    from vosdetectron_amd import ops
    s = oks_setup
    pipe, full = s["pipe"], s["out"]
    M = sum(full["counts_pre_oks_host"])
    cap = 64 if M > 64 else M // 2
    assert 0 < cap < M
    monkeypatch.setattr(pipe, "mask_rows", lambda F: cap)
    out = pipe.run(s["frames"], keep_intermediates=True, sync=False)
    assert out["kps_rois"].shape[0] == cap and "counts_host" not in out
    pipe.complete(out)
    assert out["counts_pre_oks_host"] == full["counts_pre_oks_host"]
    for k in ("dets_pre_oks", "classes_pre_oks", "kps_rois"):
        assert torch.equal(out[k], full[k]), k
    assert out["keyps_pre_oks"].shape == full["keyps_pre_oks"].shape
    res = ops.nms_oks_frames(out["keyps_pre_oks"], out["dets_pre_oks"], out["classes_pre_oks"],
                             out["counts_pre_oks"], pipe.oks_thresh)
    assert out["counts_host"] == res.counts.cpu().tolist()
    assert torch.equal(out["dets"], res.dets) and torch.equal(out["classes"], res.classes)
    assert torch.equal(out["counts"], res.counts) and torch.equal(out["oks_keep"], res.keep)
    assert torch.equal(out["keyps"], res.keyps[:sum(out["counts_host"])])


def test_gather_of_the_post_nms_result(oks_setup):
    """No process group: the send slot is the result."""
    from vosdetectron_amd.runner import ResultGatherer, frame_keyps
    s = oks_setup
    out, pipe = s["out"], s["pipe"]
    g = ResultGatherer(2, pipe.det_cap, 28, 1, DEV, with_masks=False, keyps_k=17)
    v = g.gather_async(out["dets"], out["classes"], out["counts"],
                       keyps=out["keyps"]).finish(keyps_full=out["keyps"])
    assert torch.equal(v["dets"], out["dets"]) and torch.equal(v["counts"], out["counts"])
    assert torch.equal(v["classes"], out["classes"])
    o = 0
    for f, k in enumerate(out["counts_host"]):
        assert torch.equal(frame_keyps(v, 2, f), out["keyps"][o:o + k])
        o += k
