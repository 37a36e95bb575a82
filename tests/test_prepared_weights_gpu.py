"""The weights the 3x3 conv routes and the C4 upconv GEMM derive from a live module
weight (modeling._prepared): transformed once, and remade when the live weight changes
-- an in-place copy_ or a load_state_dict -- so that the module computes, bit for bit,
what a freshly built module holding the new weight computes.  One conv per route kind,
each at the smallest batch for which the route function gives that kind; the kind is
asserted through ROUTE_COUNTS, so a fallback to another kernel fails the test."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# id = the ROUTE_COUNTS name, Conv2d arguments, map size, the ops transform that makes
# the kernel's weight operand, the route function's answer that selects the kind
CASES = [
    ("wino4", dict(in_channels=8, out_channels=256, padding=1), (64, 64),
     "conv3x3_wino4_weight", ("wino4", None)),
    ("wino4_pair", dict(in_channels=8, out_channels=256, padding=1), (15, 15),
     "conv3x3_wino4_weight", ("wino4", "pair")),
    ("wino4_grid", dict(in_channels=8, out_channels=256, padding=1), (14, 14),
     "conv3x3_wino4_weight", ("wino4", "grid")),
    ("wino", dict(in_channels=8, out_channels=64, padding=1), (16, 16),
     "conv3x3_wino_weight", ("wino", False)),
    ("wino4_grouped", dict(in_channels=64, out_channels=64, padding=1, groups=16), (128, 128),
     "conv3x3_wino4_grouped_weight", False),
    # in place on the F(4x4) kernel: 4N sub-maps of 14 x 14
    ("dilated2", dict(in_channels=8, out_channels=128, padding=2, dilation=2), (28, 28),
     "conv3x3_wino4_weight", ("wino4", "grid")),
]


def _conv(kw, seed):
    torch.manual_seed(seed)
    return nn.Conv2d(kernel_size=3, stride=1, **kw).to(DEV).requires_grad_(False)


def _route(kw, n, H, W):
    from vosdetectron_amd import modeling
    ci, co = kw["in_channels"], kw["out_channels"]
    if kw.get("groups", 1) > 1:
        return modeling.conv3x3_grouped_route(n, ci, co, H, W, kw["groups"])
    if kw.get("dilation", 1) == 2:
        return modeling.conv3x3_route(4 * n, ci, co, H // 2, W // 2)
    return modeling.conv3x3_route(n, ci, co, H, W)


def _same(a, b):
    """== that tells False (a layout) from None and 0."""
    return a == b and repr(a) == repr(b)


def _counted(monkeypatch, name):
    """ops.<name> wrapped to count its calls."""
    from vosdetectron_amd import ops
    real, calls = getattr(ops, name), []

    def wrapper(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, name, wrapper)
    return calls


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv3x3_weight_transformed_once_and_follows_the_live_weight(case, monkeypatch):
    from vosdetectron_amd import modeling
    name, kw, (H, W), transform, want = case
    n = next(n for n in range(1, 4097) if _same(_route(kw, n, H, W), want))
    conv = _conv(kw, 1)
    g = torch.Generator(device="cuda").manual_seed(n + H)
    x = torch.randn(n, kw["in_channels"], H, W, device=DEV, generator=g).contiguous(
        memory_format=torch.channels_last)
    calls = _counted(monkeypatch, transform)
    run = lambda m: modeling._conv3x3_mfma(m, x, relu=True)  # noqa: E731
    monkeypatch.setattr(modeling, "ROUTE_COUNTS", {})
    # (a) two calls, one transform
    y1, y2 = run(conv), run(conv)
    assert y1 is not None and torch.equal(y1, y2)
    assert len(calls) == 1
    assert modeling.ROUTE_COUNTS == {name: 2}
    # (b) an in-place update of the weight
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, device=DEV, generator=g) * 0.1)
    fresh = _conv(kw, 2)
    fresh.load_state_dict(conv.state_dict())
    y3 = run(conv)
    assert len(calls) == 2 and not torch.equal(y3, y1)
    assert torch.equal(y3, run(fresh))
    # (c) load_state_dict
    donor = _conv(kw, 3)
    conv.load_state_dict(donor.state_dict())
    y4 = run(conv)
    assert not torch.equal(y4, y3)
    assert torch.equal(y4, run(donor))
    torch.cuda.synchronize()
    assert set(modeling.ROUTE_COUNTS) == {name}


def test_c4_upconv_gemm_weight_follows_weight_and_bias(monkeypatch):
    """MaskHeadV0upshare._upconv_gemm keeps the GEMM form of upconv5's weight and the
    bias repeated over the four taps: split once, and remade after a change of the
    weight, of the whole state, and of the bias alone."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.c4 import MaskHeadV0upshare
    monkeypatch.delenv("VOSDET_GEMM_SPLIT3", raising=False)
    cfg = vcfg.get("e2e_mask_rcnn_R-50-C4_1x")

    def head(seed):
        torch.manual_seed(seed)
        return MaskHeadV0upshare(1024, None, 1. / 16, cfg).to(DEV).requires_grad_(False)

    def twin(m):
        t = head(9)
        t.load_state_dict(m.state_dict())
        return t

    m = head(1)
    g = torch.Generator(device="cuda").manual_seed(5)
    h = torch.randn(3, 2048, 7, 7, device=DEV, generator=g).contiguous(
        memory_format=torch.channels_last)
    calls = _counted(monkeypatch, "gemm_split3_weight")
    y1, y2 = m._upconv_gemm(h), m._upconv_gemm(h)
    assert y1 is not None and tuple(y1.shape) == (3, cfg.MRCNN.DIM_REDUCED, 14, 14)
    assert torch.equal(y1, y2) and len(calls) == 1
    w = m.upconv5.weight
    with torch.no_grad():
        w.copy_(torch.randn(w.shape, device=DEV, generator=g) * 0.02)
    y3 = m._upconv_gemm(h)
    assert not torch.equal(y3, y1) and torch.equal(y3, twin(m)._upconv_gemm(h))
    m.load_state_dict(head(3).state_dict())
    y4 = m._upconv_gemm(h)
    assert not torch.equal(y4, y3) and torch.equal(y4, twin(m)._upconv_gemm(h))
    with torch.no_grad():  # the bias alone
        m.upconv5.bias.copy_(torch.randn(m.upconv5.bias.shape, device=DEV, generator=g))
    y5 = m._upconv_gemm(h)
    assert not torch.equal(y5, y4) and torch.equal(y5, twin(m)._upconv_gemm(h))
    torch.cuda.synchronize()
