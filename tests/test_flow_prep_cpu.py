"""Raw optical flow on the host: the .flo reader / writer, the known answers of
the numpy restatement of vd_flow_to_levels (tests/flow_prep_ref.py), and the
raw_flow argument checks that need no device."""
import numpy as np
import pytest
import torch

from tests import flow_prep_ref as fref


# ------------------------------------------------------------------ .flo files
@pytest.mark.parametrize("h,w", [(5, 5), (7, 12), (1, 3)])
def test_flo_round_trip(tmp_path, h, w):
    from vosdetectron_amd import flow_io
    flow = np.random.default_rng(h * 100 + w).uniform(-30, 30, (h, w, 2)).astype(np.float32)
    p = tmp_path / "a.flo"
    flow_io.write_flo(p, flow)
    raw = p.read_bytes()
    assert len(raw) == 12 + h * w * 8
    assert raw[:4] == b"PIEH"  # float32 202021.25, little-endian
    assert np.frombuffer(raw, "<i4", 2, 4).tolist() == [w, h]  # width first
    assert np.array_equal(np.frombuffer(raw, "<f4", 2, 12), flow[0, 0])  # u then v
    back = flow_io.read_flo(p)
    assert back.dtype == np.float32 and back.shape == (h, w, 2)
    assert np.array_equal(back, flow)
    assert back.flags.writeable


def test_flo_bad_tag_and_truncation_raise(tmp_path):
    from vosdetectron_amd import flow_io
    flow = np.arange(4 * 6 * 2, dtype=np.float32).reshape(4, 6, 2)
    good = tmp_path / "good.flo"
    flow_io.write_flo(good, flow)
    raw = good.read_bytes()
    bad = tmp_path / "bad.flo"
    bad.write_bytes(np.asarray([202021.0], "<f4").tobytes() + raw[4:])
    with pytest.raises(ValueError, match="tag"):
        flow_io.read_flo(bad)
    for n in (0, 7, 12, len(raw) - 1):
        cut = tmp_path / ("cut%d.flo" % n)
        cut.write_bytes(raw[:n])
        with pytest.raises(ValueError, match="truncated"):
            flow_io.read_flo(cut)
    with pytest.raises(ValueError):
        flow_io.write_flo(tmp_path / "x.flo", np.zeros((4, 6), np.float32))


# ---------------------------------------------------------------- restatement
def test_restatement_constant_field_known_answers():
    """A constant field (a, b) at scale 1: every block entirely inside the image
    gives exactly (a/k, b/k); a block straddling the image edge gives the
    covered fraction of that; a block in the padding gives 0."""
    a, b = 2.75, -1.5
    H, W, Hp, Wp = 96, 160, 128, 192
    raw = np.empty((2, H, W, 2), np.float32)
    raw[..., 0], raw[..., 1] = a, b
    blob = fref.flow_blob(raw, 1, Hp, Wp)
    assert np.array_equal(blob[:, :, :H, :W].transpose(0, 2, 3, 1), raw)
    assert not blob[:, :, H:].any() and not blob[:, :, :, W:].any()
    for k in fref.STRIDES:
        lv = fref.level(blob, k)
        assert lv.shape == (2, 2, Hp // k, Wp // k)
        ys = np.clip(H - np.arange(Hp // k) * k, 0, k) / k  # covered fraction per block row
        xs = np.clip(W - np.arange(Wp // k) * k, 0, k) / k
        cover = ys[:, None] * xs[None, :]
        assert np.array_equal(lv[:, 0], np.broadcast_to(cover * (a / k), lv[:, 0].shape))
        assert np.array_equal(lv[:, 1], np.broadcast_to(cover * (b / k), lv[:, 1].shape))
    lv64 = fref.level(blob, 64)
    assert lv64[0, 0, 0, 0] == a / 64 and lv64[0, 0, 1, 0] == 0.5 * a / 64  # 96 = 64 + 32
    assert lv64[0, 1, 1, 2] == 0.25 * b / 64  # 160 = 2 * 64 + 32


def test_restatement_scales_values_in_double_and_matches_conv():
    """The blob at a scale other than 1 is the resized flow times the scale (one
    float32 rounding of the float64 product), and the float64 level is what the
    modules' float32 conv computes, inside the a-priori float32 bound."""
    from oracle import oracle as orc
    rng = np.random.default_rng(5)
    raw = rng.uniform(-6, 6, (1, 45, 80, 2)).astype(np.float32)
    s = 1.6
    blob = fref.flow_blob(raw, s, 128, 128)
    r = orc.cv2_resize_fx(raw[0], s)
    assert r.shape == (72, 128, 2)
    want = (r.astype(np.float64) * s).astype(np.float32)
    assert np.array_equal(blob[0, :, :72, :128], want.transpose(2, 0, 1))
    assert not blob[0, :, 72:].any()
    for k in fref.STRIDES:
        conv = orc.flow_downsample(blob, 1.0 / k)
        err = np.abs(conv - fref.level(blob, k))
        assert np.all(err <= fref.level_bound(blob, k)), k


# ----------------------------------------------------------- argument checks
def test_flow_to_levels_argument_checks_without_device():
    from vosdetectron_amd import ops
    raw = torch.zeros((2, 70, 100, 2))
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.flow_to_levels(raw, 1.0, 96, 128)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.flow_to_levels(raw, 1.0, 128, 160)
    with pytest.raises(ValueError, match="F x H x W x 2"):
        ops.flow_to_levels(torch.zeros((2, 2, 70, 100)), 1.0, 128, 128)
    with pytest.raises(ValueError, match="strides"):
        ops.flow_to_levels(raw, 1.0, 128, 128, strides=(4, 2))
    with pytest.raises(ValueError, match="device"):  # no CPU path
        ops.flow_to_levels(raw, 1.0, 128, 128)
    with pytest.raises(TypeError):
        ops.flow_to_levels(raw.numpy(), 1.0, 128, 128)


def test_pipeline_raw_flow_argument_checks_without_device():
    from vosdetectron_amd.engine import check_flow_args
    dev = torch.device("cpu")
    raw = torch.zeros((2, 120, 200, 2))
    blob = torch.zeros((2, 2, 192, 256))
    check_flow_args(None, None, 2, (120, 200), (192, 256), dev)
    check_flow_args(blob, None, 2, (120, 200), (192, 256), dev)
    check_flow_args(None, raw, 2, (120, 200), (192, 256), dev)
    with pytest.raises(ValueError, match="not both"):
        check_flow_args(blob, raw, 2, (120, 200), (192, 256), dev)
    for bad in (raw[:1], raw[:, :100], raw.permute(0, 3, 1, 2), raw[..., :1]):
        with pytest.raises(ValueError, match="raw_flow"):
            check_flow_args(None, bad, 2, (120, 200), (192, 256), dev)
    with pytest.raises(ValueError, match="raw_flow"):
        check_flow_args(None, raw.double(), 2, (120, 200), (192, 256), dev)
    with pytest.raises(ValueError, match="raw_flow.*multiples of 64"):  # a stride-32 blob
        check_flow_args(None, raw, 2, (120, 200), (160, 224), dev)
    with pytest.raises(ValueError, match="raw_flow.*device"):
        check_flow_args(None, raw, 2, (120, 200), (192, 256), torch.device("cuda"))


def test_temporal_fusion_rejects_both_flows():
    from vosdetectron_amd.vos import Generalized_VOS_RCNN
    with pytest.raises(ValueError, match="not both"):
        Generalized_VOS_RCNN.temporal_fusion(None, [], data_flow=object(),
                                             level_flows=[None] * 5)
