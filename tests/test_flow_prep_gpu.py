"""vd_flow_to_levels on the GPU: raw (.flo-layout) flow -> the blob-resolution flow
and the five FlowAlign level flows in one launch, against the numpy restatement
(tests/flow_prep_ref.py); its capture in a hipGraph; and VOSPipeline.run(raw_flow=)
against the existing flow= path on the dynamic VOS model."""
import json

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import flow_prep_ref as fref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
STRIDES = fref.STRIDES

# raw H x W, scale, resized, blob -- what each row catches:
CASES = {
    "pad_1.0": ((70, 100), 1.0, (70, 100), (128, 128)),    # blocks half image, half padding
    "up_1.6": ((45, 80), 1.6, (72, 128), (128, 128)),      # up-scaling taps, clamped edges
    "area_0.5": ((141, 203), 0.5, (70, 102), (128, 128)),  # area path, odd edges, half-to-even
    "down_0.48": ((150, 267), 0.48, (72, 128), (128, 128)),  # down-scaling other than 0.5
    "nopad_1.0": ((128, 192), 1.0, (128, 192), (128, 192)),  # no padding, Hp != Wp
}
F = 3
_REF = {}


def _case(name):
    """(raw, scale, Hp, Wp, blob reference, {k: float64 level}) -- computed once."""
    if name not in _REF:
        (H, W), s, hw_r, (Hp, Wp) = CASES[name]
        assert fref.resized_hw(H, W, s) == hw_r
        rng = np.random.default_rng(sorted(CASES).index(name) + 40)
        raw = rng.uniform(-6, 6, (F, H, W, 2)).astype(np.float32)
        raw[..., 1] = raw[..., 1] * 0.5 + 1.25  # u != v
        blob = fref.flow_blob(raw, s, Hp, Wp)
        raw.setflags(write=False)
        blob.setflags(write=False)
        _REF[name] = (raw, s, Hp, Wp, blob, {k: fref.level(blob, k) for k in STRIDES})
    return _REF[name]


def _run(raw, s, Hp, Wp, **kw):
    from vosdetectron_amd import ops
    levels, blob = ops.flow_to_levels(torch.from_numpy(np.array(raw)).to(DEV), s, Hp,
                                      Wp, **kw)
    return [l.cpu().numpy() for l in levels], (None if blob is None else blob.cpu().numpy())


@pytest.mark.parametrize("name", sorted(CASES))
def test_blob_bitexact_and_levels_within_bound(name):
    """Blob output bit-identical to the restatement, padding included; every level
    element within the a-priori float32 bound of the float64 block sum (a
    condition, not a measurement).  The kernel's and the existing conv path's
    maximum errors are printed per level (FLOWPREP_ERR lines; no threshold)."""
    raw, s, Hp, Wp, blob_ref, lv_ref = _case(name)
    levels, blob = _run(raw, s, Hp, Wp, want_blob=True)
    assert blob.shape == blob_ref.shape and blob.dtype == np.float32
    assert np.array_equal(blob.view(np.uint32), blob_ref.view(np.uint32))
    rec = {"case": name, "kernel_max_err": {}, "conv_max_err": {}, "bound_min_margin": {}}
    for k, got in zip(STRIDES, levels):
        assert got.shape == (F, 2, Hp // k, Wp // k) and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - lv_ref[k])
        bound = fref.level_bound(blob_ref, k)
        conv = np.abs(orc.flow_downsample(blob_ref, 1.0 / k).astype(np.float64) - lv_ref[k])
        rec["kernel_max_err"][k] = float(err.max())
        rec["conv_max_err"][k] = float(conv.max())
        rec["bound_min_margin"][k] = float((bound - err).min())
    print("FLOWPREP_ERR " + json.dumps(rec))
    for k, got in zip(STRIDES, levels):
        err = np.abs(got.astype(np.float64) - lv_ref[k])
        assert np.all(err <= fref.level_bound(blob_ref, k)), (k, float(err.max()))
        pad = fref.block_sum(np.abs(blob_ref), k) == 0  # blocks entirely in the padding
        assert not got[pad].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_levels_do_not_depend_on_the_launch(name):
    """Level outputs bit-identical with the blob output requested or not, for F = 3
    against the same frames one at a time, and for single levels requested alone."""
    raw, s, Hp, Wp, _, _ = _case(name)
    base, none = _run(raw, s, Hp, Wp)
    assert none is None
    with_blob, _ = _run(raw, s, Hp, Wp, want_blob=True)
    for a, b in zip(base, with_blob):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for f in range(F):
        one, _ = _run(raw[f:f + 1], s, Hp, Wp)
        for a, b in zip(base, one):
            assert np.array_equal(a[f:f + 1].view(np.uint32), b.view(np.uint32))
    for i, k in enumerate(STRIDES):
        alone, _ = _run(raw, s, Hp, Wp, strides=(k,))
        assert len(alone) == 1
        assert np.array_equal(alone[0].view(np.uint32), base[i].view(np.uint32))
    rev, _ = _run(raw, s, Hp, Wp, strides=(64, 8))  # returned in the order asked for
    assert np.array_equal(rev[0], base[4]) and np.array_equal(rev[1], base[1])


def test_constant_field_is_exact():
    """A constant field (a, b) at scale 1 gives exactly (a/k, b/k) in every full
    block and the covered fraction of it in a block straddling the image edge."""
    a, b = 2.75, -1.5
    H, W, Hp, Wp = 96, 160, 128, 192
    raw = np.empty((2, H, W, 2), np.float32)
    raw[..., 0], raw[..., 1] = a, b
    levels, _ = _run(raw, 1.0, Hp, Wp)
    for k, got in zip(STRIDES, levels):
        ys = np.clip(H - np.arange(Hp // k) * k, 0, k) / k
        xs = np.clip(W - np.arange(Wp // k) * k, 0, k) / k
        cover = ys[:, None] * xs[None, :]
        assert np.array_equal(got[:, 0], np.broadcast_to(cover * (a / k), got[:, 0].shape)), k
        assert np.array_equal(got[:, 1], np.broadcast_to(cover * (b / k), got[:, 1].shape)), k


def test_bad_blob_size_raises():
    from vosdetectron_amd import _lib, ops
    raw = torch.zeros((1, 70, 100, 2), device=DEV)
    with pytest.raises(ValueError):
        ops.flow_to_levels(raw, 1.0, 96, 128)
    # the C entry itself answers with an error status, before any launch
    out = torch.zeros((1, 2, 24, 32), device=DEV)
    st = _lib.lib().vd_flow_to_levels(raw.data_ptr(), 1, 70, 100, 1.0, 70, 100, 96, 128,
                                      out.data_ptr(), None, None, None, None, None, None)
    assert st == _lib.VD_ERR_SHAPE
    assert not out.any()


def test_graph_capture_replays_with_new_flow():
    """The op alone captured in a hipGraph (one kernel node) and replayed after the
    input buffer is overwritten with another flow equals the eager result."""
    from vosdetectron_amd import ops
    raw_a, s, Hp, Wp, _, _ = _case("up_1.6")
    raw_b = np.ascontiguousarray(raw_a[::-1] * np.float32(0.75))
    buf = torch.from_numpy(np.array(raw_a)).to(DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.flow_to_levels(buf, s, Hp, Wp, want_blob=True)  # warm on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        g_levels, g_blob = ops.flow_to_levels(buf, s, Hp, Wp, want_blob=True)
    torch.cuda.synchronize()
    buf.copy_(torch.from_numpy(raw_b))
    g.replay()
    torch.cuda.synchronize()
    e_levels, e_blob = ops.flow_to_levels(torch.from_numpy(raw_b).to(DEV), s, Hp, Wp,
                                          want_blob=True)
    assert torch.equal(g_blob, e_blob)
    for a, b in zip(g_levels, e_levels):
        assert torch.equal(a, b)
    assert not torch.equal(g_blob, torch.from_numpy(fref.flow_blob(raw_a, s, Hp, Wp)).to(DEV))


# ------------------------------------------------------------------ pipeline
FRAME_HW, BATCH = (120, 200), 2  # TEST.SCALE 144: scale 1.2, resized 144 x 240, blob 192 x 256
FLOW_AMP = 6.0
EDGE_MARGIN = 1e-4  # px: over 4x the loosest level bound (FlowAlign's border test is discontinuous)


def _displaced_margin(blob_flow):
    """Smallest distance, over the five levels, of a displaced coordinate from the
    limits 0 and W-1 (H-1) at which FlowAlign switches to zero, from the float64
    level flows.  A component whose block lies entirely in the blob's zero padding
    is left out: there both paths hold exactly 0 (the kernel writes 0, the conv
    sums zeros), the coordinate is the same integer in both runs and no rounding
    can move it across a limit -- and the padding columns always contain the
    position W-1 itself."""
    m = np.inf
    for k in STRIDES:
        lv = fref.level(blob_flow, k)  # B x 2 x h x w: x then y displacement
        live = fref.block_sum(np.abs(blob_flow), k) > 0
        h, w = lv.shape[-2:]
        px = np.arange(w)[None, None, :] + lv[:, 0]
        py = np.arange(h)[None, :, None] + lv[:, 1]
        for p, lim, ok in ((px, w - 1, live[:, 0]), (py, h - 1, live[:, 1])):
            if ok.any():
                m = min(m, float(np.abs(p[ok]).min()), float(np.abs(p[ok] - lim).min()))
    return m


def _pipeline_flow(H, W):
    """A smooth field of about +-4.5 px (so every level is displaced) plus +-1.5 px
    of seeded noise."""
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    u = 4.5 * np.sin(2 * np.pi * (xx + 0.3 * yy))
    v = 4.5 * np.cos(2 * np.pi * (yy - 0.2 * xx)) * 0.8
    raw = np.stack([np.stack([u, v], -1), np.stack([-v, 0.6 * u + 1.0], -1)])
    raw = raw + np.random.default_rng(11).uniform(-1.5, 1.5, raw.shape)
    return raw.astype(np.float32)


@pytest.fixture(scope="module")
def vos_flow_setup():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import VOSPipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_davis")
    cfg.MODEL.CONV_BODY = "FPN.fpn_ResNet50_conv5_body"  # the flow path does not depend on depth
    cfg.TEST.SCALE = 144
    H, W = FRAME_HW
    frames = [np.random.RandomState(700 + i).randint(0, 256, (BATCH, H, W, 3), np.uint8)
              for i in range(2)]
    model, _ = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=frames[0][0])
    pipe = VOSPipeline(model, cfg, frame_hw=FRAME_HW, batch=BATCH, device=DEV, channels_last=True)
    assert pipe.im_scale == 1.2 and (pipe.Hr, pipe.Wr) == (144, 240)
    assert (pipe.Hp, pipe.Wp) == (192, 256)
    raw = _pipeline_flow(H, W)
    assert raw.shape == (BATCH, H, W, 2) and 5.0 < np.abs(raw).max() < FLOW_AMP + 1.0
    blob = fref.flow_blob(raw, pipe.im_scale, pipe.Hp, pipe.Wp)
    return cfg, model, pipe, frames, raw, blob


def test_temporal_fusion_level_flows_equal_data_flow(vos_flow_setup):
    """Plumbing: temporal_fusion(level_flows=L) with L from the model's own
    conv_flow_downsample modules equals temporal_fusion(data_flow=blob) bit for bit."""
    cfg, model, pipe, frames, raw, blob = vos_flow_setup
    flow = torch.from_numpy(blob).to(DEV)
    fr = [torch.from_numpy(f).to(DEV) for f in frames]
    with torch.no_grad():
        model.clean_hidden_states()
        model.temporal_fusion(model.Conv_Body(pipe.make_blob(fr[0])))  # step 1: no flow
        state = [h.clone() for h in model.hidden_states]
        feats = model.Conv_Body(pipe.make_blob(fr[1]))
        L = [m.conv_flow_downsample(flow).contiguous() for m in model.FlowAligns]

        def step2(**kw):  # the same step 2 from the same state and features
            model.hidden_states = [h.clone() for h in state]
            return model.temporal_fusion(feats, **kw)

        step2(data_flow=flow)  # every conv of the step has run once at these shapes
        outs = [step2(data_flow=flow), step2(level_flows=L)]
        with pytest.raises(ValueError):
            step2(data_flow=flow, level_flows=L)
        no_flow = step2()
    model.clean_hidden_states()
    print("FLOWPREP_PLUMB max |diff| per level:",
          [float((a - b).abs().max()) for a, b in zip(*outs)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][4], no_flow[4])  # the flow warped something


def _cls_prob_on(pipe, pyramid, rois):
    """The step's box head (FramePipeline._run: FPN RoIAlign, Box_Head, Box_Outs) on
    the given pyramid and RoI list."""
    from vosdetectron_amd import ops
    cfg, model = pipe.cfg, pipe.model
    flat = rois.reshape(-1, 5).contiguous()
    lvl = ops.map_rois_to_fpn_levels(flat, cfg.FPN.ROI_MIN_LEVEL, cfg.FPN.ROI_MAX_LEVEL)
    lvl = (lvl - cfg.FPN.ROI_MIN_LEVEL).to(torch.int32)
    fast = pipe.channels_last and getattr(model.Box_Head, "nhwc_ready", False)
    fr = cfg.FAST_RCNN
    feat = ops.roi_align_fpn(pyramid, pipe.roi_scales, flat, lvl, fr.ROI_XFORM_RESOLUTION,
                             fr.ROI_XFORM_SAMPLING_RATIO,
                             roi_order=ops.xcd_roi_order(flat, lvl),
                             out_layout="nhwc" if fast else "nchw")
    with torch.no_grad():
        x = model.Box_Head.mlp_nhwc(feat) if fast else model.Box_Head.mlp(feat)
        return model.Box_Outs(x)[0]


def test_raw_flow_run_matches_blob_flow_run(vos_flow_setup):
    """run(frames, raw_flow=raw) against run(frames, flow=blob of the restatement)
    over two steps of two sequences: hidden states and cls_prob after step 2 agree
    within 2e-5 of the output's range (the ConvGRU tolerance of test_vos_gpu.py as
    the README states it).  The seed keeps every displaced coordinate at least
    EDGE_MARGIN px from FlowAlign's discontinuous limits -- asserted, not assumed.

    cls_prob row i belongs to proposal i, and the proposal list is a discrete
    function of the RPN maps (sort + NMS): measured here, the two runs' hidden
    states differ by <= 1.4e-5 (<= 7e-6 of the range) and their RPN maps by 6e-6,
    which reorders the 2 x 1000 proposals from row 364 on (15 rows keep the same
    box), so the row-wise cls_prob difference is 0.36 .. 0.64 -- between different
    boxes.  The flow= path run twice does exactly the same to itself (hidden
    states 1.1e-5, 14 rows keep their box, row-wise 0.49: the convolutions of a
    2-frame step are not run-to-run deterministic), so this is not the raw-flow
    path's doing.  The row-wise figure is printed and asserted whenever the two
    proposal lists are identical; when they are not, every row of cls_prob is
    compared on one RoI list instead: the box head of each run's pyramid on run
    B's proposals, all rows, the same 2e-5 of the range."""
    cfg, model, pipe, frames, raw, blob = vos_flow_setup
    margin = _displaced_margin(blob)
    assert margin > EDGE_MARGIN, margin
    fr = [torch.from_numpy(f).to(DEV) for f in frames]
    res = {}
    for mode in ("raw", "blob"):
        pipe.reset()
        pipe.run(fr[0])
        kw = ({"raw_flow": torch.from_numpy(raw).to(DEV)} if mode == "raw"
              else {"flow": torch.from_numpy(blob).to(DEV)})
        out = pipe.run(fr[1], keep_intermediates=True, **kw)
        res[mode] = ([h.clone() for h in model.hidden_states], out["cls_prob"].clone(),
                     out["rois"].clone(), [p.clone() for p in out["pyramid"]])
    pipe.reset()
    rec = {"edge_margin_px": margin, "hidden_abs_diff": [], "hidden_range": []}
    for a, b in zip(res["raw"][0], res["blob"][0]):
        rec["hidden_abs_diff"].append(float((a - b).abs().max()))
        rec["hidden_range"].append(float(b.max() - b.min()))
    ca, cb = res["raw"][1], res["blob"][1]
    assert ca.shape == cb.shape
    rng_c = float(cb.max() - cb.min())
    same_rois = torch.equal(res["raw"][2], res["blob"][2])
    rec["cls_prob_range"] = rng_c
    rec["cls_prob_rowwise_abs_diff"] = float((ca - cb).abs().max())
    rec["proposal_rows_identical"] = int((res["raw"][2] == res["blob"][2]).all(-1).sum())
    rec["proposal_rows"] = int(res["blob"][2].numel() // 5)
    on_a = _cls_prob_on(pipe, res["raw"][3], res["blob"][2])
    on_b = _cls_prob_on(pipe, res["blob"][3], res["blob"][2])
    rec["cls_prob_common_rois_abs_diff"] = float((on_a - on_b).abs().max())
    rec["cls_prob_recomputed_vs_step"] = float((on_b - cb).abs().max())
    print("FLOWPREP_PIPE " + json.dumps(rec))
    # the flow did something: the warped run differs from a run without flow
    pipe.reset()
    pipe.run(fr[0])
    pipe.run(fr[1])
    assert float((model.hidden_states[4] - res["blob"][0][4]).abs().max()) > 1e-3
    pipe.reset()
    for d, r in zip(rec["hidden_abs_diff"], rec["hidden_range"]):
        assert d <= 2e-5 * r, rec
    assert on_a.shape == cb.shape
    assert rec["cls_prob_recomputed_vs_step"] <= 2e-5 * rng_c, rec  # the helper is the step's head
    if same_rois:
        assert rec["cls_prob_rowwise_abs_diff"] <= 2e-5 * rng_c, rec
    assert rec["cls_prob_common_rois_abs_diff"] <= 2e-5 * rng_c, rec


def _no_launch(*a, **kw):
    raise AssertionError("vd_flow_to_levels launched although nothing reads its result")


def test_raw_flow_argument_errors_and_static_config(vos_flow_setup, monkeypatch):
    cfg, model, pipe, frames, raw, blob = vos_flow_setup
    from vosdetectron_amd import ops
    from vosdetectron_amd.engine import VOSPipeline
    fr = torch.from_numpy(frames[0]).to(DEV)
    rf = torch.from_numpy(raw).to(DEV)
    pipe.reset()
    with pytest.raises(ValueError, match="raw_flow"):
        pipe.run(fr, flow=torch.from_numpy(blob).to(DEV), raw_flow=rf)
    with pytest.raises(ValueError, match="raw_flow"):
        pipe.run(fr, raw_flow=rf[:, :-1])
    with pytest.raises(ValueError, match="raw_flow"):
        pipe.run(fr, raw_flow=rf[:1])
    assert all(h is None for h in model.hidden_states)  # nothing ran
    # the first frame of a sequence has no hidden state to warp: no launch either
    with monkeypatch.context() as mp:
        mp.setattr(ops, "flow_to_levels", _no_launch)
        pipe.run(fr, raw_flow=rf)
        with pytest.raises(AssertionError, match="launched"):
            pipe.run(fr, raw_flow=rf)  # the second frame does read it
    pipe.reset()
    # the static model ignores the flow: same result with raw_flow as without
    # (the model reads the same cfg object: DYNAMIC_MODEL False is the static config,
    # whose module tree differs only by the unused FlowAligns)
    dyn = cfg.CONVGRU.DYNAMIC_MODEL
    cfg.CONVGRU.DYNAMIC_MODEL = False
    try:
        static = VOSPipeline(model, cfg, frame_hw=FRAME_HW, batch=BATCH, device=DEV,
                             channels_last=True)
        # nothing reads the flow, so no launch: with ops.flow_to_levels made to fail,
        # the step with raw_flow is the very code path of the step without.  (Bit
        # equality of two runs is not asserted: the convolutions of a 2-frame step are
        # not run-to-run deterministic; the pyramids agree within the ConvGRU tolerance.)
        monkeypatch.setattr(ops, "flow_to_levels", _no_launch)
        a = static.run(fr, raw_flow=rf, keep_intermediates=True)
        b = static.run(fr, keep_intermediates=True)
        for x, y in zip(a["feats"], b["feats"]):
            assert float((x - y).abs().max()) <= 2e-5 * float(y.max() - y.min())
        assert a["cls_prob"].shape == b["cls_prob"].shape
        assert all(h is None for h in model.hidden_states)
        with pytest.raises(ValueError, match="raw_flow"):  # still checked
            static.run(fr, raw_flow=rf[:1])
    finally:
        cfg.CONVGRU.DYNAMIC_MODEL = dyn
        pipe.reset()
