"""The FPN top-down lateral step in one MFMA launch (csrc/gemm_lateral.hip,
vd_fpn_lateral_topdown) vs the reference's PyTorch sequence in fp32
(lib/modeling/FPN.py:292-300: conv_lateral(lateral) + F.upsample(top,
scale_factor=2, mode='nearest')): within 2e-5 of the output range (the GEMM's
summation order differs from the library conv's; the bias and the top-down term
are added in the reference's order).  Small shapes with ragged tiles (M not a
multiple of the 64-pixel tile), every K the kernel serves, the no-top form, the
benched P2-P4 shapes, and graph capture.  Every launch here takes the 64-pixel
(NB = 1) form; the 128-pixel form needs CUs x 1024 rows without a top-down map and
runs in tests/test_gemm_exact_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BATCH = __import__("bench").DEFAULT_FRAMES


def _case(N, K, H, W, seed, top=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(N, K, H, W, device=DEV, generator=g).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(256, K, 1, 1, device=DEV, generator=g) / K ** .5
    b = torch.randn(256, device=DEV, generator=g)
    t = torch.randn(N, 256, H // 2, W // 2, device=DEV, generator=g).contiguous(
        memory_format=torch.channels_last) if top else None
    # the torch reference in chunks of at most 16 maps x 200 x 336 (one MIOpen call over
    # a 64-frame P2 batch, > 4 GB, came out wrong on the box, round 6)
    step = max(1, (16 * 200 * 336) // (H * W))
    ref = torch.cat([F.conv2d(lat[i:i + step], w, b) for i in range(0, N, step)])
    if top:
        ref = ref + F.interpolate(t, scale_factor=2, mode="nearest")
    return lat, w, b, t, ref


def _check(got, ref):
    torch.cuda.synchronize()
    assert got.shape == ref.shape
    assert got.is_contiguous(memory_format=torch.channels_last)
    err = float((got - ref).abs().max())
    assert err <= 2e-5 * max(1., float(ref.abs().max())), err


@pytest.mark.parametrize("N,K,H,W", [(2, 256, 16, 20), (3, 512, 10, 14), (1, 1024, 6, 8),
                                     (1, 256, 2, 2), (5, 512, 38, 50), (2, 1024, 50, 84)])
@pytest.mark.parametrize("top", [True, False])
def test_fpn_lateral_vs_torch(N, K, H, W, top):
    from vosdetectron_amd import ops
    lat, w, b, t, ref = _case(N, K, H, W, N * 7 + K + H, top)
    got = ops.fpn_lateral_topdown(lat, ops.fpn_lateral_weight(w), b, t)
    _check(got, ref)


@pytest.mark.parametrize("K,H,W", [(256, 200, 336), (512, 100, 168), (1024, 50, 84)])
def test_fpn_lateral_benched_shapes(K, H, W):
    """P2 / P3 / P4 of the benched step (bench.DEFAULT_FRAMES frames)."""
    from vosdetectron_amd import ops
    lat, w, b, t, ref = _case(BATCH, K, H, W, K)
    got = ops.fpn_lateral_topdown(lat, ops.fpn_lateral_weight(w), b, t)
    _check(got, ref)
    del lat, t, ref, got


def test_fpn_lateral_rejects_bad_shapes():
    from vosdetectron_amd import ops
    w = torch.randn(256, 128, device=DEV)
    assert ops.fpn_lateral_weight(w) is None  # K = 128 is not served
    lat, w, b, t, _ = _case(1, 256, 8, 8, 1)
    wf = ops.fpn_lateral_weight(w)
    with pytest.raises(ValueError):
        ops.fpn_lateral_topdown(lat, wf, b, t[:, :, :3])


def test_fpn_lateral_graph_replay_bit_identical():
    """Captured and replayed (as bench.py's step is): bit-identical to eager."""
    from vosdetectron_amd import ops
    lat, w, b, t, ref = _case(4, 512, 40, 56, 3)
    wf = ops.fpn_lateral_weight(w)
    eager = ops.fpn_lateral_topdown(lat, wf, b, t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = ops.fpn_lateral_topdown(lat, wf, b, t)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    _check(eager, ref)


def test_fpn_lateral_module_follows_reloaded_weights():
    """weights loaded after prepare (load_state_dict) reach the fused
    path: the packed lateral weight is keyed by the live weight and repacked."""
    from vosdetectron_amd import modeling
    m = modeling.TopdownLateral(256, 256).to(DEV)
    modeling.prepare_topdown_lateral(m)
    assert m.fused_lateral  # K = 256: the default fused width
    lat, w, b, t, ref = _case(2, 256, 40, 56, 11)
    with torch.no_grad():
        m.conv_lateral.weight.copy_(torch.randn_like(w))
        m.load_state_dict({"conv_lateral.weight": w, "conv_lateral.bias": b})
        _check(m(t, lat), ref)
