"""The 1x1-conv GEMM kernels on integer-lattice inputs (tests/gemm_exact_ref.py): the output
must EQUAL the float64 product, bit for bit -- the split GEMM in both schemes
(csrc/gemm_split3.hip: six bf16 products, three fp16 products) in every tile configuration
and operand form, its fused mask tail, the fp32-MFMA kernels (gemm1x1.hip, the two-operand
GEMM, gemm_lateral.hip, rpn_head.hip) and the hipBLASLt route of vd_gemm_bias_act -- with
ReLU on and off.  A dropped piece product, a skipped K stage, a row taken from its
neighbour, a wrong row scale or a reduced-precision algorithm fails at any magnitude
(tests/test_gemm_exact_cpu.py shows each on the CPU); no tolerance is involved, but for
the one measured bound on the mask tail's sigmoid (SIGMOID_ERR).

Guard zones: a, a2, the residual or top-down map and `out` are each carved from the middle
of a larger allocation, GUARD floats on either side.  The input guards hold NaN, so a read
past either end that reaches a result poisons it; `out` and its guards hold a bit pattern
no lattice result can equal, so an unwritten output and a store past either end show.
Everything stays inside memory the test owns.  ops.rpn_head allocates its outputs: its
input is guarded and its outputs are checked by equality alone."""
import functools

import pytest
import torch

from tests import gemm_exact_ref as R
from tests.test_conv_exact_gpu import GUARD, SENTINEL

pytestmark = pytest.mark.gpu

# The mask tail writes 1 / (1 + __expf(-z)).  At an exact z its error is the intrinsic's and
# the division's alone.  Measured on the MI355X against the float64 sigmoid of the exact z,
# over every logit of R.MASK in both schemes, the planted sweep of z in [-16, 16] in steps
# of 2^-8 included (test_mask_tail_exact prints it; profiles/gemm_exact/README.md): the
# largest value, 8.81e-8 (the same in both schemes: their z is the same exact number).
# Asserted with a factor 2 for other logits than the sampled ones (the margin
# tests/test_gn_kernels_gpu.py gives its own measured sigmoid); held to a tenth of the 1e-5
# test_h2_mask_tail_vs_unfused allows.
SIGMOID_ERR = 8.81e-8
SIGMOID_CAP = 1e-6


# ------------------------------------------------------------------ guarded buffers
def _carve(shape, fill):
    """(flat buffer, its middle as a contiguous view of `shape`); channels_last for a
    4-d shape [N][C][H][W]."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(2 * GUARD + n, dtype=torch.float32, device="cuda")
    if fill is None:
        buf.view(torch.int32).fill_(SENTINEL)
    else:
        buf.fill_(fill)
    mid = buf[GUARD:GUARD + n]
    if len(shape) == 4:
        N, C, H, W = shape
        return buf, mid.view(N, H, W, C).permute(0, 3, 1, 2)
    return buf, mid.view(*shape)


def _guarded(t, shape=None):
    """t (CPU or device, rows as the kernel reads them) between NaN guards."""
    if t is None:
        return None
    _, v = _carve(tuple(t.shape) if shape is None else shape, float("nan"))
    rows = v if shape is None else v.permute(0, 2, 3, 1)   # NHWC: the rows in memory order
    rows.copy_(t.cuda().view(rows.shape))
    return v


def _guarded_out(shape):
    return _carve(shape, None)


def _verify(buf, out, ref, what):
    bits = buf.view(torch.int32)
    n = out.numel()
    assert bool((bits[:GUARD] == SENTINEL).all()), "%s: a store before out" % (what,)
    assert bool((bits[GUARD + n:] == SENTINEL).all()), "%s: a store past out" % (what,)
    assert not bool(torch.isnan(out).any()), "%s: NaN in out" % (what,)
    _equal(out, ref, what)


def _equal(out, ref, what):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if not torch.equal(out, ref):
        bad = (out != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outputs differ, first at %s: %r, float64 says %r" % (
            what, bad.shape[0], out.numel(), i, float(out[i]), float(ref[i])))


@functools.lru_cache(maxsize=None)
def _ref(c, res=True):
    """The float64 reference as the float32 it is, on the device (before the ReLU)."""
    y = R.reference(c, res)
    assert torch.equal(y.float().double(), y)
    return y.float().cuda()


def _act(y, relu):
    return torch.relu(y) if relu else y


# ------------------------------------------------------------------ the split GEMMs
def _cfgs(c):
    if c in R.SPLIT_WIDTH_DEEP:
        return (2, 4)
    return tuple(k for k in (0, 1, 2, 3, 4, 5)
                 if not ((k in (1, 5) and c.N % 256) or (k in (2, 4) and c.N % 128)))


SPLIT_RUNS = [(c, s) for c in R.SPLIT for s in R.schemes_of(c.cls)]


@pytest.mark.parametrize("c,scheme", SPLIT_RUNS,
                         ids=["%s-%s" % (R.case_id(c), s) for c, s in SPLIT_RUNS])
def test_split_gemm_exact(c, scheme):
    """ops.gemm_split3_bias_act / ops.gemm_h2_bias_act with out=, tile configurations 0 to 5
    (those whose tile width divides N; the sparse deeper-K cases 2 and 4), ReLU on and off
    (an a_bias form exists with ReLU alone)."""
    from vosdetectron_amd import ops
    i = R.inputs(c)
    weight, entry = ((ops.gemm_split3_weight, ops.gemm_split3_bias_act) if scheme == "bf16" else
                     (ops.gemm_h2_weight, ops.gemm_h2_bias_act))
    wp = weight(i.w.cuda())
    assert wp is not None
    a, a2, res = _guarded(i.a), _guarded(i.a2), _guarded(i.res)
    bias = i.bias.cuda()
    kw = {}
    if c.form == "up":
        kw["up_hw"] = c.arg[:2]
    if c.form in ("sub", "abias_sub"):
        kw["sub_hw"] = c.arg[:2]
    if i.a_bias is not None:
        kw["a_bias"] = i.a_bias.cuda()
    pre = _ref(c)
    for relu in ((True,) if i.a_bias is not None else (False, True)):
        want = _act(pre, relu)
        for cfg in _cfgs(c):
            buf, out = _guarded_out((c.M, c.N))
            y = entry(a, wp, bias, residual=res, relu=relu, out=out, cfg=cfg, a2=a2, **kw)
            torch.cuda.synchronize()
            assert y is out
            _verify(buf, out, want, "%s %s cfg %d relu=%s" % (R.case_id(c), scheme, cfg, relu))


def test_split_tile_order_cases_have_ragged_tile_counts():
    """What SPLIT_ORDER is for: under every tile shape its tile count is above 8 and no
    multiple of 8 (the XCD order's tail workgroups return early)."""
    c = R.SPLIT_ORDER[0]
    for bm, bn in ((256, 256), (256, 128), (256, 64), (128, 128)):
        tiles = -(-c.M // bm) * (c.N // bn)
        assert tiles > 8 and tiles % 8, (bm, bn, tiles)


# ------------------------------------------------------------------ the fused mask tail
MASK_RUNS = [(c, s) for c in R.MASK for s in ("bf16", "fp16")]


@pytest.mark.parametrize("c,scheme", MASK_RUNS,
                         ids=["%s-%s" % (R.mask_id(c), s) for c, s in MASK_RUNS])
def test_mask_tail_exact(c, scheme):
    """ops.mask_head_upconv_logits on both weight images: the logit z is exact on the
    lattice, so out > 0.5 exactly where z > 0, out < 0.5 where z < 0 and out == 0.5 where
    z == 0 (some are planted); the value within 2 SIGMOID_ERR of the float64 sigmoid."""
    from vosdetectron_amd import ops
    i = R.mask_inputs(c)
    z, _ = R.mask_logits(c)
    z = z.cuda()
    wp = (ops.gemm_split3_weight if scheme == "bf16" else ops.gemm_h2_weight)(i.w_up.cuda())
    x = _guarded(i.x)
    buf, out = _guarded_out((c.R, 2 * c.P, 2 * c.P))
    y = ops.mask_head_upconv_logits(x, wp, i.b_up.cuda(), i.w_cls.cuda(), i.b_cls.cuda(),
                                    i.ch.cuda(), c.P, out=out)
    torch.cuda.synchronize()
    assert y is out
    bits = buf.view(torch.int32)
    n = out.numel()
    what = "%s %s" % (R.mask_id(c), scheme)
    assert bool((bits[:GUARD] == SENTINEL).all()), what + ": a store before the masks"
    assert bool((bits[GUARD + n:] == SENTINEL).all()), what + ": a store past the masks"
    assert not bool((bits[GUARD:GUARD + n] == SENTINEL).any()), what + ": an unwritten mask pixel"
    assert not bool(torch.isnan(out).any()), what
    assert torch.equal(out > 0.5, z > 0), what
    assert torch.equal(out < 0.5, z < 0), what
    assert torch.equal(out == 0.5, z == 0), what
    dev = (out.double() - torch.sigmoid(z)).abs()
    err = float(dev.max())
    print("%s: sigmoid error %.4g over %d logits in [%.3f, %.3f]%s" % (
        what, err, n, float(z.min()), float(z.max()),
        "".join("; sweep RoI %d: %.4g" % (r, float(dev[r].max()))
                for r, ch in enumerate(c.ch) if ch == 0)))
    assert SIGMOID_ERR <= SIGMOID_CAP
    assert err <= 2 * SIGMOID_ERR, (what, err)


# ------------------------------------------------------------------ gemm1x1, hipBLASLt
def _gemm_bias_act_exact(c):
    """ops.gemm_bias_act(out=) with and without the residual, ReLU off and on; None when
    nothing serves the shape."""
    from vosdetectron_amd import ops
    i = R.inputs(c)
    a, res = _guarded(i.a), _guarded(i.res)
    w, bias = i.w.cuda(), i.bias.cuda()
    for r in (res, None):
        pre = _ref(c, r is not None)
        for relu in (False, True):
            buf, out = _guarded_out((c.M, c.N))
            y = ops.gemm_bias_act(a, w, bias, residual=r, relu=relu, out=out)
            torch.cuda.synchronize()
            if y is None:
                return None
            assert y is out
            _verify(buf, out, _act(pre, relu),
                    "%s res=%s relu=%s" % (R.case_id(c), r is not None, relu))
    return True


@pytest.mark.parametrize("c", R.G1X1, ids=R.case_id)
def test_gemm1x1_exact(monkeypatch, c):
    """csrc/gemm1x1.hip, forced with VOSDET_GEMM_MFMA=1 as test_gemm1x1_mfma_vs_torch does."""
    monkeypatch.setenv("VOSDET_GEMM_MFMA", "1")
    monkeypatch.setenv("VOSDET_GEMM_SPLIT3", "0")
    assert _gemm_bias_act_exact(c)


def test_gemm1x1_second_pass_exact(monkeypatch):
    """M = 65536 + 16 * 8 + 3: the persistent loop's 512 workgroups of 128 rows make a
    second pass, which ends ragged.  Inputs built on the device (dense narrow class; the
    condition is gemm_exact_ref.free_bound), the float64 reference too."""
    from vosdetectron_amd import ops
    monkeypatch.setenv("VOSDET_GEMM_MFMA", "1")
    monkeypatch.setenv("VOSDET_GEMM_SPLIT3", "0")
    M, K, N = R.G1X1_SECOND_PASS
    g = torch.Generator(device="cuda").manual_seed(M)
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()
    a = _guarded(ri((M, K), -3, 3) * R.Q_A)
    res = _guarded(ri((M, N), -R.B_MAX, R.B_MAX) * R.Q)
    w = ri((N, K), -3, 3) * R.Q_W
    bias = ri((N,), -R.B_MAX, R.B_MAX) * R.Q
    prod = a.double() @ w.double().t() + bias.double()
    for r in (res, None):
        pre = (prod + r.double() if r is not None else prod)
        assert float(pre.abs().max()) < R.LIMIT * R.Q
        pre = pre.float()
        for relu in (False, True):
            buf, out = _guarded_out((M, N))
            assert ops.gemm_bias_act(a, w, bias, residual=r, relu=relu, out=out) is out
            torch.cuda.synchronize()
            _verify(buf, out, _act(pre, relu), "second pass res=%s relu=%s" % (r is not None, relu))


@pytest.mark.parametrize("c", R.BLAS, ids=R.case_id)
def test_hipblaslt_route_exact(monkeypatch, c):
    """Shapes neither the split GEMMs nor gemm1x1 serve: vd_gemm_bias_act's hipBLASLt
    plan, whatever algorithm its search picks, must be exact (a reduced-precision
    algorithm fails the wide class)."""
    monkeypatch.delenv("VOSDET_GEMM_MFMA", raising=False)
    monkeypatch.setenv("VOSDET_GEMM_SPLIT3", "0")
    if _gemm_bias_act_exact(c) is None:
        pytest.skip("vd_gemm_bias_act serves no (M, K, N) = (%d, %d, %d)" % (c.M, c.K, c.N))


@pytest.mark.parametrize("c", R.DUAL, ids=R.case_id)
def test_gemm_dual_exact(c):
    from vosdetectron_amd import ops
    i = R.inputs(c)
    a1, a2 = _guarded(i.a), _guarded(i.a2)
    w, bias = i.w.cuda(), i.bias.cuda()
    pre = _ref(c)
    for relu in (False, True):
        buf, out = _guarded_out((c.M, c.N))
        assert ops.gemm_dual_bias_act(a1, a2, w, bias, relu=relu, out=out) is out
        torch.cuda.synchronize()
        _verify(buf, out, _act(pre, relu), "%s relu=%s" % (R.case_id(c), relu))


# ------------------------------------------------------------------ the FPN lateral kernel
@pytest.mark.parametrize("c", R.LATERAL, ids=R.case_id)
def test_fpn_lateral_exact(c):
    """ops.fpn_lateral_topdown(out=) with and without the top-down map, 3 images."""
    from vosdetectron_amd import ops
    i = R.inputs(c)
    h, w_, n = c.arg
    lat = _guarded(i.a, (n, c.K, h, w_))
    top = _guarded(i.res, (n, 256, h // 2, w_ // 2))
    wf = ops.fpn_lateral_weight(i.w.cuda())
    bias = i.bias.cuda()
    for t in (top, None):
        buf, out = _guarded_out((n, 256, h, w_))
        assert ops.fpn_lateral_topdown(lat, wf, bias, t, out=out) is out
        torch.cuda.synchronize()
        _verify(buf, out.permute(0, 2, 3, 1).reshape(c.M, 256), _ref(c, t is not None),
                "%s top=%s" % (R.case_id(c), t is not None))


@pytest.mark.parametrize("extra", [0, 64])
def test_fpn_lateral_128_pixel_form_exact(extra):
    """Without a top-down map and from M = CUs x 1024 rows the launcher selects the
    128-pixel (NB = 2) form: that M, the smallest, and M + 64 for its ragged end.  Built
    on the device (dense narrow class, gemm_exact_ref.free_bound), K = 256."""
    from vosdetectron_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, K = cus * 1024 + extra, R.LATERAL_BIG_K
    H, W = 64, M // 64
    g = torch.Generator(device="cuda").manual_seed(M)
    ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()
    lat = _guarded(ri((M, K), -3, 3) * R.Q_A, (1, K, H, W))
    w = ri((256, K), -3, 3) * R.Q_W
    bias = ri((256,), -R.B_MAX, R.B_MAX) * R.Q
    buf, out = _guarded_out((1, 256, H, W))
    assert ops.fpn_lateral_topdown(lat, ops.fpn_lateral_weight(w), bias, None, out=out) is out
    torch.cuda.synchronize()
    rows = lat.permute(0, 2, 3, 1).reshape(M, K)
    want = torch.empty((M, 256), dtype=torch.float32, device="cuda")
    step = 1 << 16   # the float64 reference in slices: no second copy of the whole input
    for m in range(0, M, step):
        want[m:m + step] = (rows[m:m + step].double() @ w.double().t() + bias.double()).float()
    _verify(buf, out.permute(0, 2, 3, 1).reshape(M, 256), want, "128-pixel form M=%d" % M)


# ------------------------------------------------------------------ the RPN head
@pytest.mark.parametrize("mfma", ["default", "0"])
@pytest.mark.parametrize("c", R.RPN, ids=R.case_id)
def test_rpn_head_exact(monkeypatch, c, mfma):
    """Both forms: the launcher reads VOSDET_RPN_HEAD_MFMA at every call; by default C = 256
    runs the MFMA form and every other C the LDS form, with 0 every C runs the LDS form.
    bbox_pred is exact (in-order FMA, or the MFMA's sums, on the lattice); cls_prob is on
    the right side of 0.5 (the old test keeps its value).  x is guarded."""
    from vosdetectron_amd import ops
    if mfma == "default":
        monkeypatch.delenv("VOSDET_RPN_HEAD_MFMA", raising=False)
    else:
        monkeypatch.setenv("VOSDET_RPN_HEAD_MFMA", mfma)
    i = R.inputs(c)
    n, h, w_, A = c.arg
    x = _guarded(i.a, (n, c.K, h, w_))
    cls, box = ops.rpn_head(x, i.a_bias.cuda(), i.w.cuda(), i.bias.cuda(), A)
    torch.cuda.synchronize()
    o = _ref(c).view(n, h, w_, 5 * A).permute(0, 3, 1, 2)
    what = "%s mfma=%s" % (R.case_id(c), mfma)
    assert not bool(torch.isnan(box).any()) and not bool(torch.isnan(cls).any()), what
    _equal(box, o[:, A:].contiguous(), what)
    z = o[:, :A]
    assert cls.shape == z.shape, what
    assert torch.equal(cls > 0.5, z > 0) and torch.equal(cls < 0.5, z < 0), what
    assert torch.equal(cls == 0.5, z == 0), what
