"""The lattice cases of tests/gemm_exact_ref.py on the CPU: every case meets its exactness
condition, its operands are on their lattice and inside their width class, the float64
reference is a float32, the inputs cover every output, K stage and piece -- and a float32
restatement of each scheme equals the float64 reference bit for bit in two K orders (so
the conditions admit a correct kernel), while each deliberate defect breaks the equality
on a case of the class that pins it (so the device tests can fail)."""
import pytest
import torch

from tests import gemm_exact_ref as R
from tests.test_gemm_h2_cpu import split_a, split_w
from tests.test_split3_cpu import split3

IDS = [R.case_id(c) for c in R.ALL_CASES]


def _schemes(c):
    return R.schemes_of(c.cls) if c.fam == "split" else ("fp32",)


def _find(fam, cls, form=None, **kw):
    for c in R.ALL_CASES:
        if c.fam == fam and c.cls == cls and (form is None or c.form == form) and \
                all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise LookupError((fam, cls, form, kw))


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_case_meets_its_exactness_condition(c):
    v = R.condition(c)
    assert 0 < v < 1, v


def test_device_built_cases_meet_the_data_free_bound():
    assert R.free_bound(R.G1X1_SECOND_PASS[1]) < 1 and R.free_bound(R.LATERAL_BIG_K) < 1
    M = R.G1X1_SECOND_PASS[0]
    assert M > 512 * 128 and (M - 512 * 128) % 16 != 0  # a second pass that ends ragged


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_operands_are_on_their_lattice_and_in_their_class(c):
    i = R.inputs(c)
    a, _ = R.gathered(c)
    ba, bw = R.CLASS_BITS[c.cls]
    for t, q in ((i.a, R.Q_A), (i.a2, R.Q_A), (i.a_bias, R.Q_A), (a, R.Q_A)):
        if t is not None:
            v = t.double() / q
            assert torch.equal(v, v.round())
    if not (c.fam == "rpn" and c.cls == "narrow"):   # there relu(a + a_bias) is 0..7
        assert R.significant_bits(a, R.Q_A) <= ba
    else:
        assert R.significant_bits(a, R.Q_A) <= 3
    if i.a_bias is not None:   # the prologue's ReLU acts: some relu(a + a_bias) are 0
        pre = i.a + i.a_bias
        assert bool((pre < 0).any()) and bool((pre > 0).any()) and bool((i.a_bias != 0).any())
    unit = i.col_unit
    v = i.w.double() / (unit / R.Q_A).view(-1, 1)
    assert torch.equal(v, v.round())
    assert R.significant_bits(v, 1.0) <= bw
    if c.cls != "narrow":   # the wide side does span its width
        assert max(R.significant_bits(a, R.Q_A), R.significant_bits(v, 1.0)) == max(ba, bw)
    for t in (i.bias, i.res):
        if t is not None:
            v = t.double() / unit
            assert torch.equal(v, v.round()) and float(v.abs().max()) <= R.B_MAX
    # inside float32's normal range, and the activations inside the fp16 scheme's contract
    lo = min(float(t[t != 0].abs().min()) for t in (a, i.w, i.bias) if bool((t != 0).any()))
    assert lo >= 2.0 ** -16
    assert 2.0 ** -10 <= float(a.abs().max()) <= 65504 or c.M == 1
    if c.fam == "split":
        assert int((i.w == 0).all(dim=1).sum()) == 1   # the all-zero row
        assert len(torch.unique(unit)) > 4             # row scales


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_reference_is_a_float32(c):
    for res in (True, False):
        y = R.reference(c, res)
        assert torch.equal(y.float().double(), y)
        assert float(y.abs().max()) < 2.0 ** 21


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_case_covers_outputs_stages_and_pieces(c):
    """Stated conditions, not measurements."""
    a, _ = R.gathered(c)
    w = R.inputs(c).w
    for res in (True, False):
        y = R.reference(c, res)
        assert float((y != 0).double().mean()) >= 0.9
        if y.numel() >= 64:   # ReLU hides nothing
            assert float((y > 0).double().mean()) >= 0.25
            assert float((y < 0).double().mean()) >= 0.25
        assert bool((y != 0).any(dim=1).all()) and bool((y != 0).any(dim=0).all())
    prod = a.double() @ w.double().t()
    if prod.numel() >= 64:
        assert float((prod != 0).double().mean()) >= 0.9
    for k in range(0, c.K, R.STAGE):
        s = slice(k, k + R.STAGE)
        assert bool((a[:, s].double() @ w[:, s].double().t() != 0).any()), k
    if c.fam != "split" or c.cls == "narrow":
        return
    # the wide operand's last piece: the third bf16 piece, or a1 / Wr of the fp16 scheme
    ka, kw = R.KINDS[c.cls]
    for t, kind, side in ((a, ka, "a"), (w, kw, "w")):
        nz = t != 0
        if kind == "b18":
            last = split3(t)[2]
        elif kind == "m10":
            last = split3(t)[1]
        elif kind == "h18":
            last = split_a(t)[1].float() if side == "a" else split_w(t)[1].float()
        else:
            continue
        assert float((last[nz] != 0).double().mean()) >= 0.5, side


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_restatement_equals_float64_exactly(c):
    ref = R.reference(c)
    for sch in _schemes(c):
        for order in ("asc", "desc"):
            y = R.restate(c, sch, order=order)
            assert torch.equal(y.double(), ref), (sch, order)
            y = R.restate(c, sch, order=order, relu=True)
            assert torch.equal(y.double(), torch.relu(ref)), (sch, order)


# ------------------------------------------------------------------ mutations
def _breaks(c, sch, **kw):
    ref = R.reference(c)
    assert torch.equal(R.restate(c, sch).double(), ref)
    return not torch.equal(R.restate(c, sch, **kw).double(), ref)


# the class of R.SPLIT_WIDTH (K = 16, M = 257) that has each bf16 product non-zero
BF16_PINS = {(0, 0): ("narrow", "w3", "a3", "mid"), (0, 1): ("w3", "mid"), (0, 2): ("w3",),
             (1, 0): ("a3", "mid"), (2, 0): ("a3",), (1, 1): ("mid",)}
FP16_PINS = {"a0Wm": ("narrow", "w2", "a2"), "a0Wr": ("w2",), "a1W0": ("a2",)}


def _width_case(cls):
    if cls == "narrow":
        return R.SPLIT_DEPTH[0]
    return _find("split", cls, "plain", K=16)


@pytest.mark.parametrize("drop", R.BF16_PRODUCTS, ids=lambda d: "a%dw%d" % d)
def test_each_bf16_product_is_necessary(drop):
    for cls in BF16_PINS[drop]:
        assert _breaks(_width_case(cls), "bf16", drop=drop), cls
    # and in the sparse deeper-K case of a pinning class
    cls = BF16_PINS[drop][-1]
    if cls != "narrow":
        assert _breaks(_find("split", cls, "plain", K=256), "bf16", drop=drop)


@pytest.mark.parametrize("drop", R.FP16_PRODUCTS)
def test_each_fp16_product_is_necessary(drop):
    for cls in FP16_PINS[drop]:
        assert _breaks(_width_case(cls), "fp16", drop=drop), cls
    cls = FP16_PINS[drop][-1]
    if cls != "narrow":
        assert _breaks(_find("split", cls, "plain", K=256), "fp16", drop=drop)


def test_w0_where_wm_plus_wr_belongs_breaks():
    assert _breaks(_width_case("w2"), "fp16", w0_for_wm=True)


@pytest.mark.parametrize("cls", R.FP16_CLASSES)
def test_row_scale_off_by_one_exponent_breaks(cls):
    assert _breaks(_width_case(cls), "fp16", scale_off=True)


@pytest.mark.parametrize("c", R.SPLIT_DEPTH + R.SPLIT_WIDTH_DEEP, ids=R.case_id)
def test_every_skipped_stage_breaks(c):
    """Every single K stage of the pipeline-depth cases and of the sparse deeper-K cases is
    needed (K = 1024: the first 8 and the last 2 by mutation; on the lattice a skipped stage
    changes the result exactly when its own contribution is non-zero somewhere, which
    test_case_covers_outputs_stages_and_pieces holds for all 64)."""
    n = c.K // R.STAGE
    stages = range(n) if n <= 16 else list(range(8)) + [n - 2, n - 1]
    for sch in R.schemes_of(c.cls):
        for s in stages:
            assert _breaks(c, sch, skip=s), (sch, s)


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.M > 1 and c.fam != "rpn"], ids=R.case_id)
def test_row_reading_its_neighbour_breaks(c):
    for sch in _schemes(c):
        assert _breaks(c, sch, mutate="row_next")


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.form == "up"], ids=R.case_id)
def test_topdown_row_at_the_next_x_breaks(c):
    if c.arg[1] == 2:   # a 2-wide map has one top-down column: x / 2 + 1 does not exist
        return
    for sch in _schemes(c):
        assert _breaks(c, sch, mutate="up_x")


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.form in ("sub", "abias_sub")],
                         ids=R.case_id)
def test_stride2_row_without_the_image_offset_breaks(c):
    for sch in _schemes(c):
        assert _breaks(c, sch, mutate="sub_image")


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.form == "a2" and 2 * c.arg == c.K],
                         ids=R.case_id)
def test_second_operands_columns_on_the_first_breaks(c):
    for sch in _schemes(c):
        assert _breaks(c, sch, mutate="a2_cols")


@pytest.mark.parametrize("c", [c for c in R.FP32 if c.cls == "wide" and c.M > 1], ids=R.case_id)
def test_reduced_precision_route_breaks_the_wide_class(c):
    """Operands of 9 bits instead of 10 (any reduced-precision algorithm keeps fewer)."""
    assert _breaks(c, "fp32", bits=9)


def test_index_tables():
    """sub_rows / up_rows against the definition (a stride-2 slice, nearest-2x)."""
    for (h, w, n) in ((11, 17, 3), (1, 1, 3), (2, 3, 3)):
        m = torch.arange(n * h * w).view(n, h, w)
        assert torch.equal(R.sub_rows(h, w, n), m[:, ::2, ::2].reshape(-1))
    for (h, w, n) in ((2, 2, 3), (6, 10, 3), (4, 34, 3)):
        t = torch.arange(n * (h // 2) * (w // 2)).view(n, 1, h // 2, w // 2).double()
        up = torch.nn.functional.interpolate(t, scale_factor=2, mode="nearest").long()
        assert torch.equal(R.up_rows(h, w, n), up.reshape(-1))


# ------------------------------------------------------------------ the mask tail
@pytest.mark.parametrize("c", R.MASK, ids=R.mask_id)
def test_mask_logits_are_exact_and_cover_the_signs(c):
    z, cond = R.mask_logits(c)
    assert 0 < cond < 1
    assert torch.equal(z.float().double(), z)
    v = z / R.Q_Z
    assert torch.equal(v, v.round())
    if 0 in c.ch:
        assert bool((z == 0).any())          # the planted zero logit
        r = c.ch.index(0)
        assert float(z[r].min()) >= -16 and float(z[r].max()) <= 16
    if c.P > 1:
        assert bool((z > 0).any()) and bool((z < 0).any())
        assert float((z[z != 0].abs()).min()) >= R.Q_Z
    assert R.MASK_CLASSES - 1 in c.ch                       # the last class channel
    assert c is R.MASK[0] or 0 in c.ch                       # the first, and the sweep


def test_mask_restatement_is_exact():
    """z through both schemes' float32 restatement of the upconv, the class dot product in
    float32 in two orders."""
    c = R.MASK[1]
    i = R.mask_inputs(c)
    z, _ = R.mask_logits(c)
    wc = i.w_cls[i.ch.long()]
    for f in (R.restate_bf16, R.restate_fp16):
        y = f(i.x, i.w_up, i.b_up, relu=True).view(c.R, c.P, c.P, 2, 2, 256)
        for flip in (False, True):
            yy, ww = (y.flip(-1), wc.flip(-1)) if flip else (y, wc)
            zz = torch.einsum("rhwijc,rc->rhiwj", yy, ww).reshape(z.shape) + \
                i.b_cls[i.ch.long()].view(-1, 1, 1)
            assert torch.equal(zz.double(), z)
