"""Keypoint R-CNN on the device.

1. vd_heatmaps_to_keypoints against the numpy restatement (tests/keypoint_ref.py):
   x, y and logit bit for bit; prob within rtol 1e-5 -- device expf differs from
   libm's by at most 2 ulp per term, and the restatement's pairwise float32 sum of
   at most 3e5 positive terms adds at most log2(n) * 2^-24 ~ 1.1e-6 (the kernel sums
   in float64), so 1e-5 is about a 5x margin.
2. Keypoint_Head + Keypoint_Outs against the torch CPU float64 restatement, with
   torch's own float32 error on the same chain as the yardstick (4x allowed: the
   Winograd transforms amplify rounding).
3. KeypointFramePipeline on the e2e_keypoint_rcnn_R-50-FPN_1x config: the stage
   inputs and outputs chained on the GPU's own upstream tensors, frame_keypoints,
   graph capture, and the mask config's output unchanged (no keyps).
Reference: lib/utils/keypoints.py:103-157, lib/modeling/keypoint_rcnn_heads.py,
lib/core/test.py:97-107, 529-564, 858-874."""
import numpy as np
import pytest
import torch

from tests import keypoint_ref as kref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
NAME = "e2e_keypoint_rcnn_R-50-FPN_1x"
f32 = np.float32


def _decode_inputs():
    """M = 56, K = 17: eight boxes on seeded normal logits x 3, then four special maps."""
    rng = np.random.default_rng(11)
    M, K = 56, 17
    boxes = [(10.3, 20.7, 10.9, 21.2),       # both sides < 1: a 1 x 1 map
             (100, 50, 156, 106),            # exactly 56 x 56: the identity scale
             (7, 9, 27, 40),                 # 20 x 31: a downscale
             (0, 0, 3, 200),                 # 3 x 200
             (33, 600, 333, 605),            # 300 x 5
             (12.25, 40.5, 125.75, 297.75),  # 113.5 x 257.25
             (0, 0, 640, 480),               # ten column strips
             (-13.7, -4.2, 55.1, 90.9)]      # negative and fractional offsets
    maps = (rng.standard_normal((len(boxes), K, M, M)) * 3).astype(f32)
    # the maximum in a corner (replicate clamping), one corner per keypoint
    corner = (rng.standard_normal((K, M, M)) * 3).astype(f32)
    for k in range(K):
        corner[k, (0, 0, M - 1, M - 1)[k % 4], (0, M - 1, 0, M - 1)[k % 4]] = 50.
    # two equal maxima 5 columns apart on a 56 x 56 box: the first wins
    twin = (rng.standard_normal((K, M, M)) * 3).astype(f32)
    for k in range(K):
        twin[k, 3 * k, 10 + k] = twin[k, 3 * k, 15 + k] = 40.
    const = np.full((K, M, M), -2.5, f32)
    big = np.where(rng.random((K, M, M)) < 0.5, f32(-80), f32(80)).astype(f32)
    maps = np.concatenate([maps, corner[None], twin[None], const[None], big[None]])
    boxes += [(5.5, 6.5, 95.5, 76.5), (200, 300, 256, 356), (1, 2, 78, 35), (40, 40, 104, 88)]
    return maps, np.asarray(boxes, f32)


@pytest.fixture(scope="module")
def decode_case():
    from vosdetectron_amd import ops
    maps, boxes = _decode_inputs()
    ref = kref.heatmaps_to_keypoints(maps, boxes)
    got = ops.heatmaps_to_keypoints(torch.from_numpy(maps).to(DEV), torch.from_numpy(boxes).to(DEV))
    torch.cuda.synchronize()
    return maps, boxes, ref, got


def _assert_decode(got, ref, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == np.float32
    perr = np.abs(got[:, 3] - ref[:, 3]) / ref[:, 3]
    print("%s decode: %d x %d keypoints, max relative prob error %.3g"
          % (what, ref.shape[0], ref.shape[2], float(perr.max())))
    for row, name in enumerate(("x", "y", "logit")):
        bad = np.argwhere(got[:, row] != ref[:, row])
        assert not len(bad), (what, name, bad[:5].tolist(),
                              got[:, row][tuple(bad[0])], ref[:, row][tuple(bad[0])])
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=0)


def test_decode_matches_restatement(decode_case):
    maps, boxes, ref, got = decode_case
    _assert_decode(got, ref, "M=56")
    # what the special rows are there for
    M = 56
    assert np.all(ref[0, 0] == f32(0.5 * np.float64(f32(1)) + np.float64(f32(10.3))))  # 1 x 1
    for k in range(17):  # identity scale: the heatmap's own argmax and value
        yi, xi = divmod(int(maps[1, k].argmax()), M)
        assert ref[1, 0, k] == f32(xi + 0.5 + 100) and ref[1, 2, k] == maps[1, k, yi, xi]
        assert ref[9, 0, k] == f32(10 + k + 0.5 + 200) and ref[9, 2, k] == f32(40)  # first twin
    # the constant map: 77 x 33 tap weights do not sum to exactly 1, so the resized map
    # is constant only to rounding -- the same decode for every keypoint all the same
    assert np.all(ref[10] == ref[10][:, :1]) and np.all(np.abs(ref[10, 2] + 2.5) < 1e-5)


def test_decode_small_map_min_size():
    from vosdetectron_amd import ops
    rng = np.random.default_rng(5)
    maps = (rng.standard_normal((5, 3, 8, 8)) * 3).astype(f32)
    boxes = np.asarray([(0, 0, 3.2, 40.5), (10, 10, 15, 15), (4.5, 2.5, 70.5, 21.25),
                        (0.3, 0.6, 0.9, 1.1), (100, 200, 116, 216)], f32)
    assert [kref.map_size(b, 16)[2:] for b in boxes] == \
        [(16, 41), (16, 16), (66, 19), (16, 16), (16, 16)]
    ref = kref.heatmaps_to_keypoints(maps, boxes, 16)
    got = ops.heatmaps_to_keypoints(torch.from_numpy(maps).to(DEV),
                                    torch.from_numpy(boxes).to(DEV), 16)
    _assert_decode(got, ref, "M=8 min_size=16")
    assert not np.array_equal(ref, kref.heatmaps_to_keypoints(maps, boxes, 0))


def test_decode_box_strides_identical_bits(decode_case):
    """[R, 4] boxes, a [R, 5] detection array read in place, and the [:, 1:5] view of
    a RoI array give the same bits, prob included; so does a second call."""
    from vosdetectron_amd import keypoints, ops
    maps, boxes, ref, got = decode_case
    mt = torch.from_numpy(maps).to(DEV)
    R = len(boxes)
    dets = torch.cat([torch.from_numpy(boxes), torch.rand(R, 1)], 1).to(DEV)
    rois = torch.cat([torch.zeros(R, 1), torch.from_numpy(boxes)], 1).to(DEV)
    assert dets.stride(0) == 5 and rois[:, 1:5].stride(0) == 5
    for b in (dets, rois[:, 1:5], torch.from_numpy(boxes).to(DEV)):
        assert torch.equal(ops.heatmaps_to_keypoints(mt, b), got)
    # the reference-named entry point: numpy in, numpy out
    out = keypoints.heatmaps_to_keypoints(maps[:3], boxes[:3])
    assert isinstance(out, np.ndarray) and np.array_equal(out, got[:3].cpu().numpy())
    assert ops.heatmaps_to_keypoints(mt[:0], dets[:0]).shape == (0, 4, 17)
    with pytest.raises(ValueError):
        ops.heatmaps_to_keypoints(torch.zeros(1, 3, 65, 65, device=DEV),
                                  torch.zeros(1, 4, device=DEV))


# --------------------------------------------------------------------------- #
def _errs(got, ref):
    e = (got.double().cpu() - ref).abs()
    s = float(ref.abs().max())
    return float(e.max()) / s, float(e.mean()) / s


@pytest.fixture(scope="module")
def head_case():
    """Keypoint_Head + Keypoint_Outs with seeded weights on the device, 64 seeded RoI
    maps, and the CPU restatement's float64 and float32 results on them (once)."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.modeling import KeypointOutputs, RoiPoseHeadV1convX
    from vosdetectron_amd.weights import synthetic_state_dict
    cfg = vcfg.get(NAME)

    class Heads(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.Keypoint_Head = RoiPoseHeadV1convX(256, None, None, cfg)
            self.Keypoint_Outs = KeypointOutputs(self.Keypoint_Head.dim_out, cfg)

    m = Heads()
    sd = synthetic_state_dict(m, seed=0)
    g = torch.Generator().manual_seed(2)
    for k in sd:  # non-zero biases; a gain that keeps the activations near unit scale
        if k.endswith(".bias") and "upsample" not in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
        elif "conv_fcn" in k:
            sd[k] = sd[k] * 2 ** 0.5
    m.load_state_dict(sd)
    m.eval().to(DEV)
    m.Keypoint_Head.conv_fcn.to(memory_format=torch.channels_last)
    m.Keypoint_Head.prepare()
    x = torch.randn(64, 256, 14, 14, generator=g)
    ref = kref.keypoint_head_outputs(sd, x, cfg, torch.float64)
    t32 = kref.keypoint_head_outputs(sd, x, cfg, torch.float32)
    return m, x, ref, t32


@pytest.mark.parametrize("batch,route", [(64, "wino_2d"), (256, "wino_2d")])
def test_head_accuracy_vs_fp64(head_case, batch, route):
    """The 64 maps alone and as the first 64 of a 256-map batch, the size of a 2-frame
    step, from which conv3x3_route would hand the convs to the F(4x4) kernel.
    Yardstick: torch's float32 error against float64 on the same chain; 4x allowed.

    Measured on an MI355X (max / mean error over the output range):
      torch float32 (the yardstick)   7.19e-07 / 8.70e-08
      64 maps, F(2x2) 2-D mosaic      1.71e-06 / 2.07e-07   (2.4x / 2.4x)
      256 maps, F(4x4) grid           8.36e-06 / 1.02e-06   (11.6x / 11.8x: outside)
    F(4x4,3x3)'s transforms (entries up to 8) amplify float32 rounding by about an
    order of magnitude and eight chained convs keep it, so the head does not take the
    F(4x4) route conv3x3_route offers from 256 maps up (RoiPoseHeadV1convX.wino4): both
    batch sizes run F(2x2), and the second case holds the larger batch to the bound."""
    from vosdetectron_amd import modeling
    m, x, ref, t32 = head_case
    xb = torch.cat([x] + [torch.roll(x, i, 1) for i in range(1, batch // 64)])
    modeling.ROUTE_COUNTS.clear()
    with torch.no_grad():
        x_nhwc = xb.to(DEV).permute(0, 2, 3, 1).contiguous()
        got = m.Keypoint_Outs(m.Keypoint_Head.head_nhwc(x_nhwc))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (batch, 17, 56, 56)
    assert modeling.ROUTE_COUNTS == {route: 8}, modeling.ROUTE_COUNTS
    mx, mean = _errs(got[:64], ref)
    tmx, tmean = _errs(t32, ref)
    print("keypoint head (%s) vs fp64: max %.3g mean %.3g of range; torch fp32: max %.3g "
          "mean %.3g" % (route, mx, mean, tmx, tmean))
    assert mx <= 4 * tmx and mean <= 4 * tmean, (mx, mean, tmx, tmean)


# --------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def kp_setup():
    import bench
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import KeypointFramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get(NAME)
    model, sd = build_model(cfg, seed=0, device=DEV, channels_last=True)
    pipe = KeypointFramePipeline(model, cfg, frame_hw=(320, 480), batch=2, channels_last=True,
                                 device=DEV)
    frames_np = bench.synthetic_frames(2, 21, 320, 480)
    frames = torch.from_numpy(frames_np).to(DEV)
    out = pipe.run(frames, keep_intermediates=True)
    torch.cuda.synchronize()
    return cfg, model, pipe, frames, out


def test_pipeline_outputs(kp_setup):
    from oracle import oracle as orc
    from tests.engine_checks import LEVEL_SCALES
    from vosdetectron_amd.engine import frame_keypoints
    cfg, model, pipe, frames, out = kp_setup
    ks = out["counts_host"]
    M = sum(ks)
    assert max(ks) > 0, ks
    assert "masks" not in out and not hasattr(model, "Mask_Head")
    assert tuple(out["keyps"].shape) == (M, 4, 17)
    assert tuple(out["kps_heatmaps"].shape) == (M, 17, 56, 56)
    assert tuple(out["kps_feat"].shape) == (M, 256, 14, 14)
    # the decode's boxes are the stored detections, in batch order
    dets = torch.cat([out["dets"][f, :k, :4] for f, k in enumerate(ks)])
    assert torch.equal(out["kps_boxes"], dets)
    # keypoint RoIAlign on the pipeline's own pyramid and RoIs vs the oracle
    kc = cfg.KRCNN
    o = 0
    for f, k in enumerate(ks):
        if k:
            blobs = [t[f:f + 1].cpu().numpy() for t in out["feats"][1:]]
            kr = out["kps_rois"][o:o + k].cpu().numpy().copy()
            assert np.all(kr[:, 0] == f)
            kr[:, 0] = 0
            ret = orc.distribute(kr, prefix="keypoint_rois")
            want = orc.roi_feature_transform(blobs, ret, "keypoint_rois",
                                             kc.ROI_XFORM_RESOLUTION, LEVEL_SCALES,
                                             kc.ROI_XFORM_SAMPLING_RATIO)
            np.testing.assert_allclose(out["kps_feat"][o:o + k].cpu().numpy(), want,
                                       rtol=1e-4, atol=1e-4)
        o += k
    # the decode on the pipeline's own heatmaps and boxes
    ref = kref.heatmaps_to_keypoints(out["kps_heatmaps"].cpu().numpy(),
                                     out["kps_boxes"].cpu().numpy(),
                                     kc.INFERENCE_MIN_SIZE)
    _assert_decode(out["keyps"], ref, "pipeline")
    # keypoint_results' grouping
    res = frame_keypoints(pipe, out)
    assert len(res) == 2
    kp = out["keyps"].cpu().numpy()
    o = 0
    for f, k in enumerate(ks):
        assert len(res[f]) == cfg.MODEL.NUM_CLASSES
        assert [len(c) for c in res[f]] == [k if j == 1 else 0 for j in range(len(res[f]))]
        for i in range(k):
            assert res[f][1][i].shape == (4, 17) and np.array_equal(res[f][1][i], kp[o + i])
        o += k
    assert set(pipe.enable_timers().timers) == set()
    pipe.run(frames)
    assert {"im_detect_keypoints", "misc_keypoints", "misc_bbox"} <= set(pipe.timer_summary())
    pipe.enable_timers(False)


def test_pipeline_graph_replay(kp_setup):
    cfg, model, pipe, frames, eager = kp_setup
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


def test_unbuilt_pipelines_raise(kp_setup):
    from vosdetectron_amd.c4 import C4FramePipeline
    from vosdetectron_amd.engine import (FramePipeline, KeypointFramePipeline,
                                         RaggedFramePipeline, VOSPipeline)
    from vosdetectron_amd import config as vcfg
    cfg, model, pipe, frames, out = kp_setup
    with pytest.raises(NotImplementedError, match="KEYPOINTS_ON"):
        RaggedFramePipeline(model, cfg, blob_hw=(320, 480), batch=2, channels_last=True, device=DEV)
    for cls in (FramePipeline, VOSPipeline, C4FramePipeline):
        with pytest.raises(NotImplementedError, match="KEYPOINTS_ON"):
            cls(model, cfg, frame_hw=(320, 480), batch=2, channels_last=True, device=DEV)
    with pytest.raises(ValueError):
        KeypointFramePipeline(model, vcfg.get("e2e_mask_rcnn_R-50-FPN_1x"), device=DEV)


def test_mask_config_output_has_no_keyps():
    import bench
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True)
    assert not hasattr(model, "Keypoint_Head")
    pipe = FramePipeline(model, cfg, frame_hw=(320, 480), batch=1, channels_last=True, device=DEV)
    out = pipe.run(torch.from_numpy(bench.synthetic_frames(1, 21, 320, 480)).to(DEV))
    torch.cuda.synchronize()
    assert not [k for k in out if k.startswith("keyps") or k.startswith("kps_")]
    assert out["masks"].shape[0] == sum(out["counts_host"]) and out["masks"].shape[1:] == (28, 28)
