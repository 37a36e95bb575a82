"""The two-piece fp16 split GEMM (csrc/gemm_split3.hip SCH = 1, vd_gemm_h2_bias_act): three
fp16 MFMA products per fp32 product in one accumulator.  Its accuracy claim is the
six-product kernel's: on every shape the error against an fp64 reference stays at torch's
own fp32 GEMM error (max <= 2e-5, max <= 3 x torch + 1e-7, mean <= 1.5 x torch + 1e-9 --
the rule of tests/test_gemm_split3_gpu.py::test_split3_fp32_accuracy), also at the ends
of its input contract.  Also: the weight image bit for bit, every tile configuration and
operand variant, overflow, determinism, graph replay, the weight cache and the switches.

VOSDET_H2_NUMERICS=path appends every error measured here, beside the six-product
kernel's on the same inputs, to that file as JSON lines."""
import functools
import json
import os

import pytest
import torch

from tests import test_gemm_h2_cpu as ref_h2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _case(M, N, K, res, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device=DEV, generator=g).relu_()
    w = torch.randn(N, K, device=DEV, generator=g) / K ** .5
    b = torch.randn(N, device=DEV, generator=g) * .1
    r = torch.randn(M, N, device=DEV, generator=g) if res else None
    return a, w, b, r


def _epi(y, b, r, relu):
    y = y + b.to(y.dtype)
    if r is not None:
        y = y + r.to(y.dtype)
    return y.relu() if relu else y


def _errs(got, ref):
    e = (got.double() - ref).abs()
    s = float(ref.abs().max())
    return float(e.max()) / s, float(e.mean()) / s


def _record(tag, **kw):
    path = os.environ.get("VOSDET_H2_NUMERICS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=tag, **kw)) + "\n")


def _check(tag, a, w, b, r, relu, cfg=0, ref=None, t32=None):
    """The accuracy rule on one input, the six-product kernel's figures recorded beside."""
    from vosdetectron_amd import ops
    if ref is None:
        ref = _epi(a.double() @ w.double().t(), b, r, relu)
    if t32 is None:
        t32 = _epi(a @ w.t(), b, r, relu)
    got = ops.gemm_h2_bias_act(a, ops.gemm_h2_weight(w), b, residual=r, relu=relu, cfg=cfg)
    six = ops.gemm_split3_bias_act(a, ops.gemm_split3_weight(w), b, residual=r, relu=relu,
                                   cfg=cfg)
    torch.cuda.synchronize()
    mx, mean = _errs(got, ref)
    smx, smean = _errs(six, ref)
    tmx, tmean = _errs(t32, ref)
    _record(tag, cfg=cfg, h2_max=mx, h2_mean=mean, six_max=smx, six_mean=smean, torch_max=tmx,
            torch_mean=tmean)
    print("%s cfg %d: h2 %.3g / %.3g  six %.3g / %.3g  torch %.3g / %.3g (max / mean)"
          % (tag, cfg, mx, mean, smx, smean, tmx, tmean))
    assert mx <= 2e-5, mx
    assert mx <= 3 * tmx + 1e-7 and mean <= 1.5 * tmean + 1e-9, (mx, mean, tmx, tmean)
    return got


SHAPES = [(1000, 64, 256, False, True), (777, 128, 512, True, True),
          (4099, 256, 1024, False, False), (513, 2048, 512, True, False),
          (333, 1024, 12544, False, True), (1, 256, 128, True, True),
          (257, 64, 128, False, True)]


@functools.lru_cache(maxsize=None)
def _shape_case(M, N, K, res, relu):
    """Inputs, the fp64 reference and torch's fp32 result of one shape, shared by its
    tile configurations."""
    a, w, b, r = _case(M, N, K, res, M + N + K)
    return a, w, b, r, _epi(a.double() @ w.double().t(), b, r, relu), _epi(a @ w.t(), b, r, relu)


def test_h2_weight_image_and_scale_are_the_rne_construction():
    """vd_gemm_h2_weight's three images and scale vector, bit for bit, against torch's
    round-to-nearest-even construction (tests/test_gemm_h2_cpu.py split_w), rows of very
    different magnitudes, a zero row, a power-of-two maximum and subnormal entries
    included; lane l = 32 h + r of (k-step s, tile t) holds W[32 t + r][16 s + 8 h .. + 7]."""
    from vosdetectron_amd import ops
    N, K = 128, 64
    g = torch.Generator().manual_seed(3)
    w = torch.randn(N, K, generator=g) * torch.exp2(
        torch.randint(-120, 120, (N, 1), generator=g).float())
    w[5] = 0
    w[6] = w[6].clamp(-.9, .9) * 2.0 ** -110
    w[6, 9] = 2.0 ** -110
    w[7, :8] = 2.0 ** -140
    img = ops.gemm_h2_weight(w.to(DEV))
    torch.cuda.synchronize()
    assert img.numel() == N * K * 6 + N * 4
    pieces = img[:N * K * 6].view(torch.int16).view(K // 16, N // 32, 3, 2, 32, 8).cpu()
    scale = img[N * K * 6:].view(torch.float32).cpu()
    wm, wr, w0, sc = ref_h2.split_w(w)
    assert torch.equal(scale.view(torch.int32), sc.view(torch.int32))
    for p, want in enumerate((wm, wr, w0)):
        # [N][K] -> [s][t][h][r][8]
        lay = want.view(torch.int16).view(N // 32, 32, K // 16, 2, 8).permute(2, 0, 3, 1, 4)
        assert torch.equal(pieces[:, :, p], lay), p


@pytest.mark.parametrize("M,N,K,res,relu", SHAPES)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_h2_fp32_accuracy(M, N, K, res, relu, cfg):
    if (cfg in (1, 5) and N % 256) or (cfg in (2, 4) and N % 128):
        pytest.skip("tile needs N %% %d" % (256 if cfg in (1, 5) else 128))
    a, w, b, r, ref, t32 = _shape_case(M, N, K, res, relu)
    _check("acc_%dx%dx%d" % (M, N, K), a, w, b, r, relu, cfg, ref, t32)


@pytest.mark.parametrize("what", ["a_2^-12", "a_2^9", "w_2^-15", "w_2^12", "zero_row",
                                  "pow2_row_max"])
def test_h2_range(what):
    """The ends of the input contract on the (1000, 64, 256) case.  The CPU emulation
    passes all of them, so a failure here is the device's handling of fp16 subnormal
    inputs or its rounding inside the MFMA's 16-term sum."""
    a, w, b, r = _case(1000, 64, 256, False, 1320)
    a, w = a.clone(), w.clone()
    if what.startswith("a_"):
        a *= 2.0 ** int(what[4:])
        b = b * 2.0 ** int(what[4:])
    elif what.startswith("w_"):
        w *= 2.0 ** int(what[4:])
        b = b * 2.0 ** int(what[4:])
    elif what == "zero_row":
        w[17] = 0
    else:
        w[17] = w[17].clamp(-2.0 ** -4 * .9, 2.0 ** -4 * .9)
        w[17, 100] = -2.0 ** -4
    _check("range_" + what, a, w, b, None, True)


def test_h2_overflow_is_not_finite():
    """An activation beyond fp16's range: its output row is non-finite (never a finite
    wrong value, ReLU included); the other rows are untouched."""
    from vosdetectron_amd import ops
    a, w, b, _ = _case(300, 128, 256, False, 77)
    wp = ops.gemm_h2_weight(w)
    good = ops.gemm_h2_bias_act(a, wp, b)
    a[41, 130] = 1e5
    for relu in (True, False):
        y = ops.gemm_h2_bias_act(a, wp, b, relu=relu)
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(y[41]).any())
        keep = torch.arange(300, device=DEV) != 41
        assert bool(torch.isfinite(y[keep]).all())
        if relu:
            assert torch.equal(y[keep], good[keep])


def test_h2_two_operands():
    from vosdetectron_amd import ops
    g = torch.Generator(device="cuda").manual_seed(64)
    h = torch.randn(5000, 64, device=DEV, generator=g).relu_()
    x = torch.randn(5000, 64, device=DEV, generator=g).relu_()
    w = torch.randn(256, 128, device=DEV, generator=g) / 128 ** .5
    b = torch.randn(256, device=DEV, generator=g)
    wp = ops.gemm_h2_weight(w)
    got = ops.gemm_h2_bias_act(h, wp, b, a2=x)
    want = _check("two_operands", torch.cat([h, x], 1), w, b, None, True)
    assert torch.equal(got, want)


def test_h2_stride2_rows_odd_map():
    from vosdetectron_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    n, C, H, W, N = 3, 256, 11, 17, 128
    x = torch.randn(n, C, H, W, device=DEV, generator=g).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(N, C, device=DEV, generator=g) / C ** .5
    b = torch.randn(N, device=DEV, generator=g)
    wp = ops.gemm_h2_weight(w)
    xs = x[:, :, ::2, ::2].contiguous(memory_format=torch.channels_last)
    rows = xs.permute(0, 2, 3, 1).reshape(-1, C)
    want = _check("stride2", rows, w, b, None, True)
    got = ops.gemm_h2_bias_act(x.permute(0, 2, 3, 1).reshape(-1, C), wp, b, sub_hw=(H, W))
    torch.cuda.synchronize()
    assert got.shape == (n * 6 * 9, N) and torch.equal(got, want)


def test_h2_a_bias_prologue():
    from vosdetectron_amd import ops
    g = torch.Generator(device="cuda").manual_seed(12)
    a = torch.randn(700, 256, device=DEV, generator=g)
    ab = torch.randn(256, device=DEV, generator=g) * .5
    w = torch.randn(128, 256, device=DEV, generator=g) / 16
    b = torch.randn(128, device=DEV, generator=g)
    res = torch.randn(700, 128, device=DEV, generator=g)
    wp = ops.gemm_h2_weight(w)
    pre = torch.relu(a + ab)
    for r in (None, res):
        want = _check("a_bias", pre, w, b, r, True)
        assert torch.equal(ops.gemm_h2_bias_act(a, wp, b, residual=r, a_bias=ab), want)


def test_h2_topdown_lateral_6x10():
    """RES 2: the top-down map of a 6 x 10 level added at the nearest-2x row."""
    import torch.nn.functional as F
    from vosdetectron_amd import ops
    g = torch.Generator(device="cuda").manual_seed(13)
    n, K, H, W = 2, 256, 6, 10
    lat = torch.randn(n * H * W, K, device=DEV, generator=g)
    w = torch.randn(256, K, device=DEV, generator=g) / K ** .5
    b = torch.randn(256, device=DEV, generator=g)
    top = torch.randn(n, H // 2, W // 2, 256, device=DEV, generator=g)
    up = F.interpolate(top.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(
        0, 2, 3, 1).reshape(-1, 256)
    want = _check("lateral_6x10", lat, w, b, up, False)
    got = ops.gemm_h2_bias_act(lat, ops.gemm_h2_weight(w), b, residual=top.reshape(-1, 256),
                               relu=False, up_hw=(H, W))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@torch.no_grad()
def test_h2_mask_tail_vs_unfused():
    """The mask head's upconv + class-selected logits + sigmoid on the fp16 scheme: 3 RoIs
    of 14 x 14, 5 classes, within 1e-5 of the unfused path and of fp64."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd import modeling, ops
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    g = torch.Generator(device="cuda").manual_seed(14)
    R, ncls, P = 3, 5, 14
    head = modeling.MaskHeadV1upXconvs(256, None, 1. / 16, cfg).to(DEV)
    outs = modeling.MaskRCNNOutputs(256, ncls).to(DEV)
    head.upconv.weight.copy_(torch.randn(256, 256, 2, 2, device=DEV, generator=g) / 16)
    head.upconv.bias.copy_(torch.randn(256, device=DEV, generator=g) * .1)
    outs.classify.weight.copy_(torch.randn(ncls, 256, 1, 1, device=DEV, generator=g) / 16)
    outs.classify.bias.copy_(torch.randn(ncls, device=DEV, generator=g))
    head.prepare()
    x = torch.randn(R * P * P, 256, device=DEV, generator=g).relu_()
    cls = torch.randint(0, ncls, (R,), device=DEV, generator=g, dtype=torch.int32)
    ch = outs._channel(cls).to(torch.int32)
    got = ops.mask_head_upconv_logits(x, ops.gemm_h2_weight(head.up_wt), head.up_b,
                                      outs.classify.weight.view(ncls, -1), outs.classify.bias,
                                      ch, P)
    unf = outs.selected_from_up(head._upconv_nhwc(x, R, P), cls)
    y = (x.double() @ head.up_wt.double().t() + head.up_b.double()).relu().view(R, P, P, 2, 2, 256)
    wc = outs.classify.weight.view(ncls, 256).double()[ch.long()]
    z = torch.einsum("rhwijc,rc->rhiwj", y, wc).reshape(R, 2 * P, 2 * P)
    ref = torch.sigmoid(z + outs.classify.bias.double()[ch.long()].view(-1, 1, 1))
    torch.cuda.synchronize()
    d64, dun = float((got.double() - ref).abs().max()), float((got - unf).abs().max())
    _record("mask_tail", h2_vs_fp64=d64, h2_vs_unfused=dun)
    assert got.shape == (R, 2 * P, 2 * P)
    assert d64 <= 1e-5 and dun <= 1e-5, (d64, dun)


def test_h2_deterministic_and_graph_replay():
    from vosdetectron_amd import ops
    a, w, b, r = _case(5000, 256, 512, True, 5)
    wp = ops.gemm_h2_weight(w)
    y0 = ops.gemm_h2_bias_act(a, wp, b, residual=r)
    y1 = ops.gemm_h2_bias_act(a, wp, b, residual=r)
    assert torch.equal(y0, y1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = ops.gemm_h2_bias_act(a, wp, b, residual=r)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y0)


def test_h2_route_and_cache(monkeypatch):
    """gemm_bias_act(h2=True) equals the direct h2 call bit for bit where h2_route serves
    the shape and keeps its default otherwise; the cached image follows an in-place update
    and load_state_dict; VOSDET_GEMM_H2=0 and VOSDET_GEMM_SPLIT3=0 switch it off."""
    from vosdetectron_amd import ops
    monkeypatch.delenv("VOSDET_GEMM_H2", raising=False)
    monkeypatch.delenv("VOSDET_GEMM_SPLIT3", raising=False)
    a, w, b, _ = _case(3000, 256, 512, False, 9)
    lin = torch.nn.Linear(512, 256).to(DEV).requires_grad_(False)
    with torch.no_grad():
        lin.weight.copy_(w)
    assert ops.h2_route(3000, 256, 512) and not ops.h2_route(3000, 256, 64)
    six = ops.gemm_bias_act(a, lin.weight, b)
    assert torch.equal(six, ops.gemm_split3_bias_act(a, ops.gemm_split3_weight(w), b))
    y = ops.gemm_bias_act(a, lin.weight, b, h2=True)
    assert torch.equal(y, ops.gemm_h2_bias_act(a, ops.gemm_h2_weight(w), b))
    assert not torch.equal(y, six)
    with torch.no_grad():
        lin.weight.mul_(0.5)
    y2 = ops.gemm_bias_act(a, lin.weight, b, h2=True)
    assert torch.equal(y2, ops.gemm_h2_bias_act(a, ops.gemm_h2_weight(w * 0.5), b))
    donor = torch.nn.Linear(512, 256).to(DEV)
    lin.load_state_dict(donor.state_dict())
    y3 = ops.gemm_bias_act(a, lin.weight, b, h2=True)
    assert torch.equal(y3, ops.gemm_h2_bias_act(a, ops.gemm_h2_weight(donor.weight.detach()), b))
    monkeypatch.setenv("VOSDET_GEMM_H2", "0")
    assert not ops.h2_route(3000, 256, 512)
    y4 = ops.gemm_bias_act(a, lin.weight, b, h2=True)
    assert torch.equal(y4, ops.gemm_bias_act(a, lin.weight, b))
    monkeypatch.delenv("VOSDET_GEMM_H2")
    monkeypatch.setenv("VOSDET_GEMM_SPLIT3", "0")
    assert not ops.h2_route(3000, 256, 512)
    torch.cuda.synchronize()


@torch.no_grad()
def test_h2_off_bottleneck_is_the_six_product_path(monkeypatch):
    """A Bottleneck at 2 x 256 x 20 x 24 launches no fp16-scheme GEMM (the body keeps the
    six-product kernel: it feeds the proposal ranking), with the switch at its default and
    with VOSDET_GEMM_H2=0: the output equals, bit for bit, the block composed from the
    six-product entries (conv1 and conv3 + residual through ops.gemm_split3_bias_act, conv2
    through the block's own 3x3 route)."""
    from vosdetectron_amd import modeling, ops
    monkeypatch.delenv("VOSDET_GEMM_SPLIT3", raising=False)
    torch.manual_seed(0)
    blk = modeling.Bottleneck(256, 256, 128, 1, 1).to(DEV).eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.normal_(m.weight, 0, (2. / m.weight[0].numel()) ** .5)
    modeling.prepare_bottlenecks([blk])
    x = torch.randn(2, 256, 20, 24, device=DEV).relu_().contiguous(
        memory_format=torch.channels_last)
    monkeypatch.delenv("VOSDET_GEMM_H2", raising=False)
    calls = []
    real = ops.gemm_h2_bias_act
    monkeypatch.setattr(ops, "gemm_h2_bias_act", lambda *a, **k: calls.append(1) or real(*a, **k))
    y_on = blk(x)
    monkeypatch.setenv("VOSDET_GEMM_H2", "0")
    y_off = blk(x)
    assert not calls
    x2d = x.permute(0, 2, 3, 1).reshape(-1, 256)
    h = ops.gemm_split3_bias_act(x2d, ops.gemm_split3_weight(blk.w1), blk.f1.bias)
    h = h.view(2, 20, 24, 128).permute(0, 3, 1, 2)
    h2 = modeling._conv3x3_mfma(blk.f2, h, relu=True)
    if h2 is None:
        h2 = modeling._conv_epi(blk.f2, h)
    want = ops.gemm_split3_bias_act(h2.permute(0, 2, 3, 1).reshape(-1, 128),
                                    ops.gemm_split3_weight(blk.w3), blk.f3.bias, residual=x2d)
    torch.cuda.synchronize()
    assert torch.equal(y_off.permute(0, 2, 3, 1).reshape(-1, 256), want)
    assert torch.equal(y_on, y_off)


@torch.no_grad()
def test_h2_switch_on_the_box_head(monkeypatch):
    """The heads ask for the fp16 scheme: FastRCNNOutputs' fused cls / bbox GEMM equals the
    direct fp16-scheme call bit for bit, and with VOSDET_GEMM_H2=0 the six-product one
    (today's output); the two agree at fp32's level."""
    from vosdetectron_amd import modeling, ops
    monkeypatch.delenv("VOSDET_GEMM_SPLIT3", raising=False)
    monkeypatch.delenv("VOSDET_GEMM_H2", raising=False)
    torch.manual_seed(1)
    head = modeling.FastRCNNOutputs(1024, 81).to(DEV).eval()
    x = torch.randn(777, 1024, device=DEV).relu_()
    w, b = head._cat_weights()
    _, box_on = head(x)
    monkeypatch.setenv("VOSDET_GEMM_H2", "0")
    _, box_off = head(x)
    nc, nb = 81, 324
    want_on = ops.gemm_h2_bias_act(x, ops.gemm_h2_weight(w), b, relu=False)[:, nc:nc + nb]
    want_off = ops.gemm_split3_bias_act(x, ops.gemm_split3_weight(w), b, relu=False)[:, nc:nc + nb]
    torch.cuda.synchronize()
    assert torch.equal(box_on, want_on) and torch.equal(box_off, want_off)
    assert not torch.equal(box_on, box_off)
    assert float((box_on - box_off).abs().max()) <= 2e-5 * float(box_off.abs().max())
