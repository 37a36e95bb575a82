"""Frames of different sizes in one pipeline step, on the GPU.

The reference's drivers (tools/infer_simple.py, test_net.py) run images of any
size; its im_list_to_blob (lib/utils/blob.py:86-114) places each prepared image
top-left in one zero blob.  Here:

* vd_image_resize_to_blob_ragged: every frame's slice equals the single-image
  get_image_blob in its top-left and is exactly zero elsewhere, bit for bit;
* vd_segm_rle_ragged: counts and strings of detections pasted into frames of
  different sizes equal the oracle's paste + rleEncode and vd_segm_rle per frame;
* RaggedFramePipeline: stage-wise and end-to-end parity per frame with the
  frame's own scale and im_info, a captured step replayed with other sizes,
  frame_segms with per-frame RLE sizes, and bound-filling frames against the
  single-size pipeline's blob."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.engine_checks import e2e_vs_cpu, stagewise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KEYS = ("dets", "classes", "counts", "rois", "roi_counts", "masks", "mask_rois", "mask_feat")

BLOB_SIZES = [(96, 160), (48, 80), (192, 320), (75, 53), (61, 97), (97, 161)]


# ------------------------------------------------------------------ 1. blob
@pytest.fixture(scope="module")
def blob_frames():
    frames = [np.random.RandomState(700 + i).randint(0, 256, hw + (3,), np.uint8)
              for i, hw in enumerate(BLOB_SIZES)]
    refs = [orc.get_image_blob(fr, 96, 160, 32) for fr in frames]
    return frames, refs


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("nhwc", [False, True])
def test_ragged_blob_vs_get_image_blob(blob_frames, order, nhwc):
    from vosdetectron_amd import ops
    frames, refs = blob_frames
    idx = list(range(len(frames)))
    if order == "reversed":
        idx = idx[::-1]
    fr = [frames[i] for i in idx]
    geo = ops.frame_geometry([f.shape[:2] for f in fr], 96, 160, 32)
    assert any(o % 2 for o in geo.offset)  # a frame at an odd byte offset
    Hb, Wb = 160, 160
    assert (max(h for h, _ in geo.padded), max(w for _, w in geo.padded)) == (Hb, Wb)
    packed = torch.from_numpy(np.concatenate([f.reshape(-1) for f in fr])).to(DEV)
    lut = torch.from_numpy(ops.pixel_lut()).to(DEV)
    shape = (len(fr), Hb, Wb, 3) if nhwc else (len(fr), 3, Hb, Wb)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    got = ops.image_resize_to_blob_ragged(packed, geo, lut, Hb, Wb, nhwc=nhwc, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    if nhwc:
        got = got.transpose(0, 3, 1, 2)
    for k, i in enumerate(idx):
        blob, scale, info = refs[i]
        assert scale == geo.scale[k] and np.array_equal(info, geo.im_info()[k:k + 1])
        Hp, Wp = blob.shape[2:]
        assert (Hp, Wp) == geo.padded[k]
        assert np.array_equal(got[k, :, :Hp, :Wp].view(np.uint32), blob[0].view(np.uint32)), i
        rest = got[k].copy()
        rest[:, :Hp, :Wp] = 0
        assert not rest.view(np.uint32).any(), i  # exactly +0.0 outside, no NaN left
    # without `out`, and the rows given as a device tensor (the captured form)
    rows = torch.from_numpy(geo.rows().view(np.uint8)).to(DEV)
    again = ops.image_resize_to_blob_ragged(packed, rows, lut, Hb, Wb, nhwc=nhwc)
    assert torch.equal(again, out)


# ------------------------------------------------------------------- 2. RLE
def _expanding_to_15():
    """A box whose (R + 2) / R expansion is exactly 15 x 15 for R = 28: the 30 x 30
    padded mask is resized by exactly 1/2 (OpenCV's INTER_AREA 2 x 2 mean)."""
    for x2 in np.arange(10, 20, 0.01, dtype=np.float32):
        b = np.array([[3.0, 4.0, 3.0 + x2, 4.0 + x2]], np.float32)
        e = orc.expand_boxes(b, 30. / 28).astype(np.int32)[0]
        if e[2] - e[0] + 1 == 15 and e[3] - e[1] + 1 == 15:
            return [3.0, 4.0, 3.0 + x2, 4.0 + x2, 1.0]
    raise AssertionError("no 15 x 15 expanded box found")


def test_ragged_segm_rle_vs_oracle_and_per_frame():
    from vosdetectron_amd import ops
    sizes = [(40, 50), (50, 40), (33, 47)]
    R = 28
    rng = np.random.default_rng(17)
    boxes, det_hw, frame_of = [], [], []
    for f, (H, W) in enumerate(sizes):
        x1, y1 = rng.uniform(0, W / 2), rng.uniform(0, H / 2)
        rows = [[0, 0, W - 1, H - 1, 1],                      # the whole frame
                [W - 12.4, H - 9.6, W + 6.0, H + 5.0, 1],    # past the right and bottom edge
                _expanding_to_15(),                           # the 2 x 2 area path
                [x1, y1, x1 + rng.uniform(3, W / 2), y1 + rng.uniform(3, H / 2), 1]]
        boxes += rows
        det_hw += [[H, W]] * len(rows)
        frame_of += [f] * len(rows)
    boxes = np.array(boxes, np.float32)
    det_hw = np.array(det_hw, np.int32)
    frame_of = np.array(frame_of)
    M = len(boxes)
    assert M == 12
    masks = rng.uniform(0, 1, (M, R, R)).astype(np.float32)
    masks[:, ::3] = 0.5   # values at the binarisation threshold
    masks[0] = 0.9        # all ones in a full-frame box: full-height columns of ones
    masks[4, :, -3:] = 0.9  # ones in the plane's last columns
    ref_counts, ref_rles = [], []
    for i in range(M):
        H, W = det_hw[i]
        plane = orc.paste_masks(masks[i:i + 1], boxes[i:i + 1], int(H), int(W))[0]
        rle, cnts = orc.rle_encode(plane)
        assert rle["size"] == [int(H), int(W)]
        ref_counts.append(cnts)
        ref_rles.append(rle["counts"])
    assert sum(ref_counts[0][1::2]) > 0.9 * 40 * 50  # the full-frame box: nearly all ones
    assert all(c.sum() == h * w for c, (h, w) in zip(ref_counts, det_hw))
    mt, bt = torch.from_numpy(masks).to(DEV), torch.from_numpy(boxes).to(DEV)
    need = max(len(c) for c in ref_counts)
    assert need > 3
    for cap, hw in ((None, det_hw), (3, torch.from_numpy(det_hw).to(DEV))):  # 3: the retry
        cnt, n = ops.segm_rle_counts_ragged(mt, bt, hw, 0.5, cap=cap)
        assert cnt.shape[1] >= need and (cap is None or cnt.shape[1] == need)
        strings = ops.rle_strings(cnt, n)
        cn, nn = cnt.cpu().numpy(), n.cpu().numpy()
        for i in range(M):
            assert np.array_equal(cn[i, :nn[i]], ref_counts[i]), i
            assert strings[i] == ref_rles[i], i
        # bit for bit the single-size entry run per frame
        for f, (H, W) in enumerate(sizes):
            sel = np.flatnonzero(frame_of == f)
            st = torch.from_numpy(sel).to(DEV)
            c1, n1 = ops.segm_rle_counts(mt[st], bt[st], H, W, 0.5)
            c1, n1 = c1.cpu().numpy(), n1.cpu().numpy()
            for k, i in enumerate(sel):
                assert n1[k] == nn[i] and np.array_equal(c1[k, :n1[k]], cn[i, :nn[i]]), i


def test_ragged_wrappers_validate_on_the_host():
    from vosdetectron_amd import ops
    m = torch.zeros((1, 28, 28), device=DEV)
    b = torch.tensor([[1., 1., 9., 9., 1.]], device=DEV)
    with pytest.raises(ValueError, match="8192"):
        ops.segm_rle_counts_ragged(m, b, [[24, 9000]])
    with pytest.raises(ValueError):
        ops.segm_rle_counts_ragged(m, b, [[0, 40]])
    with pytest.raises(ValueError):
        ops.segm_rle_counts_ragged(m, b, [[24, 40], [24, 40]])
    geo = ops.frame_geometry(BLOB_SIZES, 96, 160, 32)
    packed = torch.zeros((geo.nbytes,), dtype=torch.uint8, device=DEV)
    lut = torch.from_numpy(ops.pixel_lut()).to(DEV)
    with pytest.raises(ValueError, match="larger than the blob bound"):
        ops.image_resize_to_blob_ragged(packed, geo, lut, 128, 160)
    with pytest.raises(ValueError, match="packed buffer"):
        ops.image_resize_to_blob_ragged(packed[:-1], geo, lut, 160, 160)


# ---------------------------------------------------------------- 3-6. engine
SET_A = [(256, 416), (416, 256), (200, 300), (128, 200)]
SET_B = [(416, 256), (256, 416), (128, 200), (200, 300)]
BOUND = (416, 416)


def _frames(sizes, seed0):
    return [np.random.RandomState(seed0 + i).randint(0, 256, hw + (3,), np.uint8)
            for i, hw in enumerate(sizes)]


@pytest.fixture(scope="module")
def ragged_setup():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd import ops
    from vosdetectron_amd.engine import RaggedFramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = 256, 416
    # calibrated on a frame shaped like a batch slice: noise top-left, the zero
    # region (pixel means) elsewhere -- with the default calibration the zero
    # region drives every score to 1.0 and tie-breaking decides the result
    c = np.empty((416, 416, 3), np.uint8)
    c[:] = (103, 116, 123)
    c[:256, :416] = np.random.RandomState(0).randint(0, 256, (256, 416, 3), np.uint8)
    model, sd = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=c)
    frames = _frames(SET_A, 21)
    assert ops.blob_bound(SET_A, cfg) == BOUND
    pipe = RaggedFramePipeline(model, cfg, BOUND, batch=4, channels_last=True, device=DEV)
    batch = pipe.new_batch().load(frames)
    out = pipe.run(batch, keep_intermediates=True)
    torch.cuda.synchronize()
    return cfg, model, sd, pipe, frames, batch, out


def test_ragged_engine_stagewise(ragged_setup):
    """Every frame of the batch: proposals (clipped by the frame's own im_info row)
    and detections (divided by its own scale, clipped to its own size) bit-exact
    against the oracle on the GPU's own upstream tensors, RoIAlign within 1e-4."""
    cfg, model, sd, pipe, frames, batch, out = ragged_setup
    assert out["frame_hw"] == SET_A and tuple(out["feats"][-1].shape[-2:]) == (104, 104)
    assert "_pyrs" not in out
    for f, fr in enumerate(frames):
        stagewise(cfg, pipe, out, fr, f)
        k = out["counts_host"][f]
        d = out["dets"][f, :k].cpu().numpy()
        H, W = fr.shape[:2]
        assert k > 0 and (d[:, 2] <= W - 1).all() and (d[:, 3] <= H - 1).all()


def test_ragged_engine_end_to_end_vs_cpu(ragged_setup, monkeypatch):
    """The independent CPU pipeline fed the zero-padded blob with the frame's own
    scale and im_info (what im_list_to_blob gives the reference for this batch)."""
    cfg, model, sd, pipe, frames, batch, out = ragged_setup
    import oracle.pipeline as opl
    from oracle.pipeline import RefCPUPipeline
    real = orc.get_image_blob

    def padded_blob(im, *args, **kw):
        blob, scale, info = real(im, cfg.TEST.SCALE, cfg.TEST.MAX_SIZE, cfg.FPN.COARSEST_STRIDE)
        full = np.zeros((1, 3) + BOUND, np.float32)
        full[:, :, :blob.shape[2], :blob.shape[3]] = blob
        return full, scale, info

    monkeypatch.setattr(opl.orc, "get_image_blob", padded_blob)
    torch.set_num_threads(16)
    ref = RefCPUPipeline(sd)
    for f, fr in enumerate(frames):
        e2e_vs_cpu(out, ref(fr), f)


def _clone(out):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _assert_same(a, b, what):
    assert a["counts_host"] == b["counts_host"], what
    assert a["frame_hw"] == b["frame_hw"], what
    for k in KEYS:
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        assert torch.equal(x, y), (what, k, float((x.float() - y.float()).abs().max()))


def test_ragged_graph_replay_with_other_sizes(ragged_setup):
    """One step captured on a RaggedBatch (own stream, warm run first, as the
    benchmark captures its steps), replayed after load() put frames of other sizes
    there: bit-identical to an eager run of those frames -- nothing about the
    frame sizes is baked in at capture."""
    cfg, model, sd, pipe, frames_a, _, _ = ragged_setup
    frames_b = _frames(SET_B, 41)
    gb = pipe.new_batch().load(frames_a)
    pipe.complete(pipe.run(gb, sync=False))  # eager warm-up step
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pipe.run(gb, sync=False)  # warm on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        gout = pipe.run(gb, sync=False)
    torch.cuda.synchronize()
    eb = pipe.new_batch()
    for name, fr, sizes in (("other sizes", frames_b, SET_B), ("first set again", frames_a, SET_A)):
        gb.load(fr)
        g.replay()
        rep = pipe.complete(dict(gout))
        torch.cuda.synchronize()
        rep = _clone(rep)
        ref = pipe.run(eb.load(fr), sync=True)
        torch.cuda.synchronize()
        assert ref["frame_hw"] == sizes and sum(ref["counts_host"]) > 0
        _assert_same(rep, ref, name)


def test_ragged_frame_segms(ragged_setup):
    """frame_segms on the ragged output (one vd_segm_rle_ragged launch) equals
    segm.segm_results called per frame with that frame's size."""
    from vosdetectron_amd import segm
    from vosdetectron_amd.engine import frame_segms
    cfg, model, sd, pipe, frames, batch, out = ragged_setup
    got = frame_segms(pipe, out)
    assert len(got) == len(frames)
    start = 0
    for f, fr in enumerate(frames):
        k = out["counts_host"][f]
        H, W = fr.shape[:2]
        want = segm.segm_results(out["dets"][f, :k], out["classes"][f, :k],
                                 out["masks"][start:start + k], H, W,
                                 thresh=cfg.MRCNN.THRESH_BINARIZE)
        start += k
        assert got[f] == want, f
        rles = [r for c in got[f] for r in c]
        assert len(rles) == k and all(r["size"] == [H, W] for r in rles)


# ------------------------------------------------------ 7. bound-filling frames
def test_bound_filling_frames_match_the_single_size_blob(ragged_setup):
    """Frames whose own padded size is the bound: each slice of the ragged blob is
    bit-identical to the batch-1 FramePipeline's make_blob of that frame."""
    from vosdetectron_amd.engine import FramePipeline, RaggedFramePipeline
    cfg, model = ragged_setup[0], ragged_setup[1]
    sizes = [(256, 416), (250, 410), (128, 208), (128, 208)]
    frames = _frames(sizes, 61)
    pipe = RaggedFramePipeline(model, cfg, (256, 416), batch=4, channels_last=True, device=DEV)
    batch = pipe.new_batch().load(frames)
    blob = pipe.make_blob(batch)
    assert tuple(blob.shape) == (4, 3, 256, 416)
    assert batch.im_info.cpu().tolist() == [[256.0, 416.0, float(np.float32(s))]
                                            for s in (1.0, 416 / 410, 2.0, 2.0)]
    for f, fr in enumerate(frames):
        one = FramePipeline(model, cfg, frame_hw=fr.shape[:2], batch=1, channels_last=True,
                            device=DEV)
        assert (one.Hp, one.Wp) == (256, 416)
        want = one.make_blob(torch.from_numpy(fr[None]).to(DEV))
        assert torch.equal(blob[f:f + 1], want), f
        assert torch.equal(batch.im_info[f:f + 1], one.im_info)
        assert torch.equal(batch.im_scale_d[f:f + 1], one.im_scale_d)
        assert torch.equal(batch.im_scale_t[f:f + 1], one.im_scale_t)
        assert torch.equal(batch.im_hw[f:f + 1], one.im_hw)
    with pytest.raises(ValueError, match="larger than the blob bound"):
        batch.load(_frames([(416, 256)] + sizes[1:], 61))
    with pytest.raises(ValueError, match="holds 4 frames"):
        batch.load(frames[:3])
