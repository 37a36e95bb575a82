"""Output-only kernels inside guarded carves (tests/guarded.py; DESIGN section 2, item
10): no workspace, so what is checked is containment -- no byte outside the output --
and that the output equals the present reference of the op and so does not depend on
what the output held before (0x00 / 0xFF prefill)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import aug_ref
from tests import guarded as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_t, _np, _stream, sweep, rows_equal = G.to_dev, G.to_np, G.stream, G.sweep, G.rows_equal


@pytest.fixture(scope="module")
def arena():
    return G.Arena(DEV, 16 << 20)


def _frames(F, H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (F, H, W, 3), np.uint8)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_image_to_blob(arena, nhwc):
    """Two 37 x 53 frames at scale 1 into the 64 x 64 blob of stride 32: the padding
    is part of the output (zeros), so the whole carve is defined."""
    from vosdetectron_amd import ops
    fr = _frames(2, 37, 53, 1)
    ref = np.concatenate([orc.get_image_blob(f, 37, 53, 32)[0] for f in fr])
    assert ref.shape == (2, 3, 64, 64)
    lut = _t(ops.pixel_lut())
    for fill in G.FILLS:
        arena.reset()
        out = arena.carve((2, 64, 64, 3) if nhwc else (2, 3, 64, 64), torch.float32, fill,
                          "image_to_blob out")
        assert ops.image_to_blob(_t(fr), lut, 64, 64, nhwc=nhwc, out=out) is out
        arena.check("image_to_blob")
        rows_equal(_np(out.permute(0, 3, 1, 2).contiguous() if nhwc else out), ref, "blob")


@pytest.mark.parametrize("target", [48, 20], ids=["up", "down"])
def test_image_resize_to_blob(arena, target):
    from vosdetectron_amd import ops
    fr = _frames(2, 37, 53, 2)
    refs = [orc.get_image_blob(f, target, 1000, 32) for f in fr]
    ref = np.concatenate([r[0] for r in refs])
    scale = refs[0][1]
    Hp, Wp = ref.shape[2:]
    lut = _t(ops.pixel_lut())
    for fill in G.FILLS:
        for nhwc in (False, True):
            arena.reset()
            out = arena.carve((2, Hp, Wp, 3) if nhwc else (2, 3, Hp, Wp), torch.float32, fill,
                              "image_resize_to_blob out")
            ops.image_resize_to_blob(_t(fr), lut, scale, Hp, Wp, nhwc=nhwc, out=out)
            arena.check("image_resize_to_blob")
            rows_equal(_np(out.permute(0, 3, 1, 2).contiguous() if nhwc else out), ref, "blob")


def test_nchw_to_nhwc(arena):
    from vosdetectron_amd import ops
    x = np.random.default_rng(3).standard_normal((2, 5, 7, 9)).astype(np.float32)
    for fill in G.FILLS:
        arena.reset()
        out = arena.carve((2, 7, 9, 5), torch.float32, fill, "nchw_to_nhwc out")
        ops.nchw_to_nhwc(_t(x), out=out)
        arena.check("nchw_to_nhwc")
        rows_equal(_np(out), np.ascontiguousarray(x.transpose(0, 2, 3, 1)), "nhwc")


@pytest.mark.parametrize("layout", [0, 1], ids=["nchw", "nhwc"])
def test_flow_align(arena, layout):
    """vd_flow_align_forward as ops.flow_align calls it, on an odd 6 x 7 map: C = 12 (3
    of 64 lanes active), displacements that land exactly on a pixel, on the last row /
    column, and far outside."""
    from vosdetectron_amd._lib import check, lib
    rng = np.random.default_rng(2126)
    f = rng.standard_normal((2, 12, 6, 7)).astype(np.float32)
    fl = rng.uniform(-2.5, 2.5, (2, 2, 6, 7)).astype(np.float32)
    fl[:, :, ::3] = np.round(fl[:, :, ::3])
    fl[:, 0, 1, 2], fl[:, 1, 1, 2] = 4.0, 0.25      # lands exactly on W - 1
    fl[:, 0, 2, 1], fl[:, 1, 2, 1] = 0.25, 3.0      # exactly on H - 1
    fl[:, 0, 3, 4], fl[:, 1, 3, 4] = 1e9, -1e9      # far outside
    ref = orc.flow_align(f, fl)
    B, C, H, W = f.shape
    ft = _t(f.transpose(0, 2, 3, 1)) if layout else _t(f)
    flt = _t(fl)
    for fill in G.FILLS:
        arena.reset()
        out = arena.carve((B, H, W, C) if layout else (B, C, H, W), torch.float32, fill,
                          "vd_flow_align_forward out")
        check(lib().vd_flow_align_forward(ft.data_ptr(), flt.data_ptr(), B, C, H, W, layout,
                                          out.data_ptr(), _stream()), "vd_flow_align_forward")
        arena.check("flow_align")
        rows_equal(_np(out.permute(0, 3, 1, 2).contiguous() if layout else out), ref, "aligned")


@pytest.mark.parametrize("heur", ["SOFT_AVG", "SOFT_MAX"])
def test_mask_aug_accumulate_finish(arena, heur):
    """The accumulator is the carve; the first view overwrites whatever it held."""
    from vosdetectron_amd import ops
    rng = np.random.default_rng(5)
    M, R, flips = 3, 28, [False, True, False]
    raw = [rng.uniform(0, 1, (M, R, R)).astype(np.float32) for _ in flips]
    ref = aug_ref.combine_masks([aug_ref.invert_masks(m, f) for m, f in zip(raw, flips)], heur)
    for fill in G.FILLS:
        arena.reset()
        acc = arena.carve((M, R, R), torch.float32, fill, "mask_aug accumulator")
        for t, (m, f) in enumerate(zip(raw, flips)):
            ops.mask_aug_accumulate(acc, _t(m), f, heur, first=t == 0)
        ops.mask_aug_finish(acc, len(flips), heur)
        arena.check("mask_aug")
        rows_equal(_np(acc), np.ascontiguousarray(ref, np.float32), "combined masks")


# --------------------------------------------------------------------------- allocated inside
# The wrappers below allocate their outputs themselves.  Under G.guarded_alloc every
# tensor they allocate is a carve, so the C entry gets the wrapper's own argument list
# with pointers into the arena.
def _both_fills(arena, monkeypatch, run, check):
    """run() under output prefills 0x00 and 0xFF: canaries intact, check(outputs) against
    the reference, and the two runs' outputs the same bits."""
    seen = []
    for fill in G.FILLS:
        arena.reset()
        log = G.guarded_alloc(monkeypatch, arena, fill)
        outs = run()
        arena.check("outputs 0x%02X" % fill)
        assert log, "the wrapper allocated nothing inside the arena"
        assert all(any(o.data_ptr() == v.data_ptr() for v in log) for o in outs
                   if o is not None and o.numel())
        check(outs)
        seen.append([None if o is None else o.clone() for o in outs])
    for a, b in zip(*seen):
        if a is not None:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                "the output depends on what the buffer held"


def _assert_decode(got, ref):
    """As tests/test_keypoints_gpu.py: x, y and the logit exact, the probability to 1e-5."""
    got = _np(got)
    assert got.shape == ref.shape and got.dtype == np.float32
    for row in range(3):
        assert np.array_equal(got[:, row], ref[:, row]), row
    np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-5, atol=0)


def test_heatmaps_to_keypoints(arena, monkeypatch):
    """The M = 8, min_size = 16 case of tests/test_keypoints_gpu.py, and R = 0."""
    from tests import keypoint_ref as kref
    from vosdetectron_amd import ops
    rng = np.random.default_rng(5)
    maps = (rng.standard_normal((5, 3, 8, 8)) * 3).astype(np.float32)
    boxes = np.asarray([(0, 0, 3.2, 40.5), (10, 10, 15, 15), (4.5, 2.5, 70.5, 21.25),
                        (0.3, 0.6, 0.9, 1.1), (100, 200, 116, 216)], np.float32)
    ref = kref.heatmaps_to_keypoints(maps, boxes, 16)
    mt, bt = _t(maps), _t(boxes)
    _both_fills(arena, monkeypatch, lambda: [ops.heatmaps_to_keypoints(mt, bt, 16)],
                lambda outs: _assert_decode(outs[0], ref))
    arena.reset()
    G.guarded_alloc(monkeypatch, arena, G.ONES)
    assert ops.heatmaps_to_keypoints(mt[:0], bt[:0], 16).shape == (0, 4, 3)
    arena.check("R = 0")


def test_heatmaps_to_keypoints_aug(arena, monkeypatch):
    """M = 7, K = 5, eight views with size dependence, as tests/test_kps_aug_gpu.py; the
    combined maps and the keypoints are both the wrapper's own tensors."""
    from tests import keypoint_ref as kref, kps_aug_ref as kar
    from vosdetectron_amd import ops
    K, M, R, V = 5, 7, 9, 8
    rng = np.random.default_rng(100 + K)
    maps = [(rng.standard_normal((R, K, M, M)) * 3).astype(np.float32) for _ in range(V)]
    hf = [False, True] * 4
    ds = [False, False, True, True, True, True, False, False]
    us = [False] * 6 + [True, True]
    xy = rng.uniform(0, 200, (R, 2))
    boxes = np.hstack([xy, xy + rng.uniform(0.5, 90, (R, 2))]).astype(np.float32)
    boxes[0] = (3, 4, 32, 33)
    perm = [3, 4, 2, 0, 1]
    want, _ = kar.combine(maps, hf, "HM_AVG", ds, us, boxes, 900., perm=perm)
    ref = kref.heatmaps_to_keypoints(want, boxes, 2)
    mts, bt = [_t(m) for m in maps], _t(boxes)

    def check(outs):
        _assert_decode(outs[0], ref)
        rows_equal(_np(outs[1]), want, "combined maps")

    _both_fills(arena, monkeypatch,
                lambda: list(ops.heatmaps_to_keypoints_aug(mts, hf, ds, us, bt, 2, "HM_AVG", 900.,
                                                           flip_perm=perm, want_combined=True)),
                check)


def test_nms_oks_frames(arena, monkeypatch):
    """Frames with 0 rows and a failure code next to full ones (the d256 launch of
    tests/test_oks_nms_gpu.py on the executed reference's fixture): all six outputs are
    defined everywhere (-1 / zeros past the counts) and equal the restatement."""
    from tests import oks_ref
    from vosdetectron_amd import ops
    thresh, _, cases = oks_ref.fixture_cases()
    cases = {c["n"]: c for c in cases}
    frames, D = [0, 1, 17, 100, -1, 65, 2, 12, 16, 64], 256
    rng = np.random.default_rng(40)
    counts = np.asarray(frames, np.int32)
    dets = rng.uniform(0, 50, (len(frames), D, 5)).astype(np.float32)
    cls = rng.integers(1, 80, (len(frames), D)).astype(np.int32)
    kps = []
    for f, n in enumerate(frames):
        if n > 0:
            dets[f, :n, :4] = cases[n]["rois"]
            kps.append(cases[n]["kp"])
    kps = np.concatenate(kps + [rng.uniform(0, 100, (5, 4, 17)).astype(np.float32)])
    ref = oks_ref.nms_oks_frames(kps, dets, cls, counts, thresh)
    dev = [_t(a) for a in (kps, dets, cls, counts)]

    def check(outs):
        for key, o in zip(("keep", "counts", "dets", "classes", "keyps", "scores"), outs):
            rows_equal(_np(o), np.ascontiguousarray(ref[key]).astype(_np(o).dtype), key)
        assert _np(outs[1]).tolist()[:5] == [0, 1, len(cases[17]["keep"]), len(cases[100]["keep"]),
                                             -1]

    _both_fills(arena, monkeypatch, lambda: list(ops.nms_oks_frames(*dev, thresh=thresh)), check)


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_image_resize_to_blob_ragged(arena, nhwc):
    """Frames of four sizes into one 160 x 160 bound, as tests/test_ragged_gpu.py: each
    slice equals get_image_blob top-left and is +0.0 elsewhere (the whole carve is
    defined)."""
    from vosdetectron_amd import ops
    sizes = [(48, 80), (75, 53), (61, 97), (97, 161)]
    fr = [np.random.RandomState(700 + i).randint(0, 256, hw + (3,), np.uint8)
          for i, hw in enumerate(sizes)]
    refs = [orc.get_image_blob(f, 96, 160, 32)[0] for f in fr]
    geo = ops.frame_geometry([f.shape[:2] for f in fr], 96, 160, 32)
    Hb = max(h for h, _ in geo.padded)
    Wb = max(w for _, w in geo.padded)
    want = np.zeros((len(fr), 3, Hb, Wb), np.float32)
    for k, b in enumerate(refs):
        want[k, :, :b.shape[2], :b.shape[3]] = b[0]
    packed = _t(np.concatenate([f.reshape(-1) for f in fr]))
    lut = _t(ops.pixel_lut())
    for fill in G.FILLS:
        arena.reset()
        out = arena.carve((len(fr), Hb, Wb, 3) if nhwc else (len(fr), 3, Hb, Wb), torch.float32,
                          fill, "image_resize_to_blob_ragged out")
        ops.image_resize_to_blob_ragged(packed, geo, lut, Hb, Wb, nhwc=nhwc, out=out)
        arena.check("ragged blob")
        rows_equal(_np(out.permute(0, 3, 1, 2).contiguous() if nhwc else out), want, "blob")


def test_flow_to_levels(arena, monkeypatch):
    """The up_1.6 case of tests/test_flow_prep_gpu.py (45 x 80 raw flow, blob 128 x 128):
    the blob bit for bit, the five levels within their a-priori bound of the float64
    block sums, exactly zero in the padding."""
    from tests import flow_prep_ref as fref
    from vosdetectron_amd import ops
    (H, W), s, (Hp, Wp), F = (45, 80), 1.6, (128, 128), 3
    rng = np.random.default_rng(44)
    raw = rng.uniform(-6, 6, (F, H, W, 2)).astype(np.float32)
    raw[..., 1] = raw[..., 1] * 0.5 + 1.25
    blob_ref = fref.flow_blob(raw, s, Hp, Wp)
    rt = _t(raw)

    def run():
        levels, blob = ops.flow_to_levels(rt, s, Hp, Wp, want_blob=True)
        return list(levels) + [blob]

    def check(outs):
        rows_equal(_np(outs[-1]), blob_ref, "blob")
        for k, got in zip(fref.STRIDES, outs[:-1]):
            got = _np(got)
            err = np.abs(got.astype(np.float64) - fref.level(blob_ref, k))
            assert np.all(err <= fref.level_bound(blob_ref, k)), k
            assert not got[fref.block_sum(np.abs(blob_ref), k) == 0].any()

    _both_fills(arena, monkeypatch, run, check)


DELTA_TANH_T = 2 * 6.3e-8  # tests/test_delta_flow_gpu.py: twice the measured tanhf error


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
def test_delta_flow_features(arena, monkeypatch, nhwc):
    """The "valid" case of tests/test_delta_flow_gpu.py (B = 3, C = 64, blob 128 x 64, the
    middle row without a previous feature).  The state is updated in place, so the state
    tensors are carves too: new feature within its bound, delta = new - previous bit for
    bit where valid and zero where not."""
    from tests import delta_flow_ref as dref
    from vosdetectron_amd import ops
    B, C, (Hp, Wp), valid = 3, 64, (128, 64), (1, 0, 1)
    gen = torch.Generator().manual_seed(72)
    feats = [torch.randn((B, C, Hp // k, Wp // k), generator=gen) for k in dref.STRIDES]
    weights = [torch.randn((2, C, 3, 3), generator=gen) * 0.02 for _ in dref.STRIDES]
    prev = [torch.rand((B, 2, Hp // k, Wp // k), generator=gen) * 2 - 1 for k in dref.STRIDES]
    pa = [dref.pre(x, w) for x, w in zip(feats, weights)]
    ref = [torch.tanh(p) for p, _ in pa]
    bound = [dref.feature_bound(a, C, DELTA_TANH_T) for _, a in pa]
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = [f.to(DEV).contiguous(memory_format=fmt) for f in feats]
    w = [t.to(DEV) for t in weights]
    v = torch.tensor(valid, dtype=torch.int32, device=DEV)

    def run():
        state = []
        for i, p in enumerate(prev):
            st = arena.carve(tuple(p.shape), torch.float32, G.ZERO, "delta-flow state %d" % i)
            st.copy_(p)
            state.append(st)
        deltas = ops.delta_flow_features(x, w, state, v, layout=int(nhwc))
        return list(deltas) + state

    def check(outs):
        deltas, state = outs[:len(prev)], outs[len(prev):]
        for i, (s, d, p, r, b) in enumerate(zip(state, deltas, prev, ref, bound)):
            s, d = s.cpu(), d.cpu()
            assert bool(((s.double() - r).abs() <= b).all()), i
            want = s - p
            for row, ok in enumerate(valid):
                if ok:
                    assert torch.equal(d[row].view(torch.int32), want[row].view(torch.int32))
                else:
                    assert not d[row].any()

    seen = []
    for fill in G.FILLS:
        arena.reset()
        log = G.guarded_alloc(monkeypatch, arena, fill)
        outs = run()
        arena.check("delta_flow_features, outputs 0x%02X" % fill)
        assert len(log) >= len(prev)
        check(outs)
        seen.append([o.clone() for o in outs])
    for a, b in zip(*seen):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_delta_flow_to_levels(arena, monkeypatch):
    """The "border" case of tests/test_delta_flow_gpu.py (B = 2, blob 64 x 128: P6 is
    1 x 2): data_flow and the five levels within their bounds."""
    from tests import delta_flow_ref as dref
    from vosdetectron_amd import ops
    B, (Hp, Wp) = 2, (64, 128)
    gen = torch.Generator().manual_seed(90)
    deltas = [torch.rand((B, 2, Hp // k, Wp // k), generator=gen) * 4 - 2 for k in dref.STRIDES]
    dd = [d.to(DEV) for d in deltas]
    ref_blob = dref.upsample_sum(deltas)
    ref_levels = dref.levels(ref_blob)

    def run():
        levels, blob = ops.delta_flow_to_levels(dd, Hp, Wp, want_blob=True)
        return list(levels) + [blob]

    def check(outs):
        assert bool(((outs[-1].cpu().double() - ref_blob).abs() <= dref.pixel_bound(deltas)).all())
        for l, r, b in zip(outs[:-1], ref_levels, dref.level_bounds(deltas)):
            assert bool(((l.cpu().double() - r).abs() <= b).all())

    _both_fills(arena, monkeypatch, run, check)


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("mode", ["none", "same_bias", "up"])
def test_bias_act_odd_grid(arena, cl, mode):
    """vd_bias_act in place on a carve, an odd 13 x 7 grid (14 x 6 for the half-size
    residual): equal to the unfused torch sequence bit for bit, as
    tests/test_epilogue_gpu.py, and nothing outside x."""
    import torch.nn.functional as F
    from vosdetectron_amd import ops
    N, C, H, W = (3, 5, 14, 6) if mode == "up" else (3, 5, 13, 7)
    gen = torch.Generator().manual_seed(H + C)
    x0 = torch.randn((N, C, H, W), generator=gen).to(DEV)
    b = torch.randn(C, generator=gen).to(DEV)
    rb = torch.randn(C, generator=gen).to(DEV) if mode == "same_bias" else None
    res = None
    if mode != "none":
        res = torch.randn((N, C, H // 2, W // 2) if mode == "up" else (N, C, H, W),
                          generator=gen).to(DEV)
    y = x0 + b.view(1, -1, 1, 1)
    if res is not None:
        r = F.interpolate(res, scale_factor=2, mode="nearest") if mode == "up" else res
        y = y + (r + rb.view(1, -1, 1, 1) if rb is not None else r)
    want = F.relu(y)
    fmt = torch.channels_last if cl else torch.contiguous_format
    arena.reset()
    x = arena.carve((N, H, W, C) if cl else (N, C, H, W), torch.float32, G.ONES, "bias_act_ x")
    x = x.permute(0, 3, 1, 2) if cl else x
    x.copy_(x0)
    got = ops.bias_act_(x, b, None if res is None else res.contiguous(memory_format=fmt), rb,
                        relu=True, upsample_residual=mode == "up")
    arena.check("bias_act_ %s" % mode)
    assert got.data_ptr() == x.data_ptr()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("N,C,H,W", [(1, 64, 13, 7), (3, 8, 1, 2)])
def test_bias_relu_maxpool(arena, monkeypatch, N, C, H, W):
    """The two smallest (odd) shapes of tests/test_epilogue_gpu.py: equal to relu(x + b)
    followed by MaxPool2d(3, 2, 1) bit for bit."""
    import torch.nn.functional as F
    from vosdetectron_amd import ops
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(N, C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    b = torch.randn(C, generator=g).to(DEV)
    ref = F.max_pool2d(F.relu(x + b.view(1, -1, 1, 1)), kernel_size=3, stride=2, padding=1)

    def check(outs):
        assert outs[0].shape == ref.shape
        assert torch.equal(outs[0].contiguous().view(torch.int32),
                           ref.contiguous().view(torch.int32))

    _both_fills(arena, monkeypatch, lambda: [ops.bias_relu_maxpool(x, b)], check)
