"""The lattice cases of tests/conv_exact_ref.py on the CPU: every case meets its
exactness condition, a float32 restatement of the Winograd arithmetic then equals the
float64 convolution bit for bit (so the condition admits a correct kernel), U is exactly
representable, the inputs cover every tap, channel and pixel -- and each of five
deliberate defects breaks the equality.  The per-tile-position precision criterion that
was measured and not adopted: the figures that decided it."""
import pytest
import torch

from tests import conv_exact_ref as R

IDS = [R.case_id(c) for c in R.ALL_CASES]
WINO_IDS = [R.case_id(c) for c in R.WINO_CASES]
DIL = {c for c, _ in R.W4_DILATED}


def _dilation(c):
    return 2 if c in DIL else 1


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_case_meets_its_exactness_condition(c):
    v = R.condition(c, _dilation(c))
    assert 0 < v < 1, v
    if c.kind == "stem":
        x, w, _ = R.inputs(c)
        ok, bits = R.stem_bits_ok(x, w)
        assert ok, bits
        assert max(bits) > 8  # one side does span two bf16 pieces


@pytest.mark.parametrize("c", R.ALL_CASES, ids=IDS)
def test_case_covers_taps_pixels_outputs(c):
    """Caps, not measurements: every (tap, input channel) has a nonzero weight for some
    output channel, every input pixel is nonzero in some channel, at least 90 % of the
    outputs are nonzero (the stem: of its conv's outputs, and of the pooled ones past one
    pixel, where the pool sees a positive value)."""
    x, w, _ = R.inputs(c)
    assert bool((w != 0).any(dim=0).all())
    assert bool((x != 0).any(dim=1).all())
    for bias in (False, True):
        y = R.reference(c, bias, _dilation(c))
        if c.kind == "stem" and bias and c.H * c.W == 1:
            continue
        assert float((y != 0).double().mean()) >= 0.9, bias


@pytest.mark.parametrize("c", R.WINO_CASES, ids=WINO_IDS)
def test_restatement_equals_float64_exactly(c):
    """F(4x4) / F(2x2) in float32 == the float64 direct conv, bit for bit, in every
    accumulation order; U = G g G^T is exactly representable.  (A dilated case: the
    restatement runs on its four polyphase sub-maps, each a pad-1 conv.)"""
    x, w, b = R.inputs(c)
    m = 4 if c.kind == "w4" else 2
    U = R.u64(R.dense_weight(w, c.groups), m)
    assert torch.equal(U.float().double(), U)
    # the weight kernels' own route to it (G's 1 / 6 as a double, one rounding) lands there,
    # but for residues where the exact U is 0 (conv_exact_ref.u_as_kernel)
    Uk = R.u_as_kernel(R.dense_weight(w, c.groups), m)
    assert torch.equal(Uk.double()[U != 0], U[U != 0])
    assert float((Uk.double() * (U == 0)).abs().max()) <= 2.0 ** -50 * float(w.abs().max())
    for bias in (True, False):
        ref = R.reference(c, bias, _dilation(c))
        for order in R.ORDERS:
            if c in DIL:
                y = torch.empty(ref.shape, dtype=torch.float32)
                for a in (0, 1):
                    for bb in (0, 1):
                        y[:, :, a::2, bb::2] = R.wino_restate(
                            x[:, :, a::2, bb::2], w, b if bias else None, m=m, order=order)
            else:
                y = R.wino_restate(x, w, b if bias else None, m=m, order=order, groups=c.groups)
            assert torch.equal(y.double(), ref), (bias, order)
            assert torch.equal(torch.relu(y).double(), torch.relu(ref))
        if c not in DIL:
            y = R.wino_restate(x, w, b if bias else None, m=m, groups=c.groups, U=Uk)
            assert torch.equal(y.double(), ref), bias


@pytest.mark.parametrize("c", [R.W4_PLAIN[0], R.W4_PLAIN[1]], ids=R.case_id)
@pytest.mark.parametrize("mutate", ["bt", "tap", "shift", "chunk", "pad"])
def test_mutations_break_exact_equality(c, mutate):
    """The test form has teeth: one coefficient of B^T off by one, one tap dropped, the
    patch shifted by one pixel, the last 8-channel chunk skipped, a padding tap read as
    the neighbouring pixel -- each breaks the equality on the table's smallest F(4x4)
    case (one pixel) and on the smallest with neighbours (5 x 3)."""
    x, w, b = R.inputs(c)
    ref = R.reference(c, True)
    assert torch.equal(R.wino_restate(x, w, b).double(), ref)
    y = R.wino_restate(x, w, b, mutate=mutate)
    assert not torch.equal(y.double(), ref)


def test_generator_is_on_the_lattice():
    for c in (R.W4_PLAIN[0], R.W2_PLAIN[1], R.GEMM[0], R.STEM[1]):
        x, w, b = R.inputs(c)
        qd, qw, unit = R.UNITS[c.kind]
        for t, q in ((x, qd), (w, unit * qw), (b, qd * qw)):
            v = t.double() / q
            assert torch.equal(v, v.round())
        assert float(x.abs().max()) <= c.d_max * qd
        assert float(w.abs().max()) <= c.w_max * unit * qw
        lo = min(float(t[t != 0].abs().min()) for t in (x, w, b))
        assert lo >= 2.0 ** -12 and R.LIMIT * qd * qw <= 2.0 ** 17


# ------------------------------------------------------------------ precision criterion
def test_precision_criterion_is_not_shippable():
    """The per-position criterion's factor, measured on the restatement alone: the
    accumulation order of the channel sum moves the per-class RMS by R.ORDER_RATIO at
    C = 256, so K = 1.25 x that is above 2 -- and the 20-bit-operand restatement it was
    to reject sits inside K, while the existing 5e-5 max|y| criterion accepts it too.
    (One seed and the deepest form here; conv_exact_ref records all of them.)"""
    form, data = ("w4", 256, 1), "randn"
    # the two elementwise orders: the same on every host (a batched matmul's is not)
    rms = {o: R.precision_restated(form, data, 0, o)[0] for o in ("asc", "mfma4")}
    ratio = float((rms["asc"] / rms["mfma4"]).max())
    assert ratio == pytest.approx(R.ORDER_RATIO, rel=0.03), ratio
    assert R.K_PRECISION == pytest.approx(1.25 * R.ORDER_RATIO) and R.K_PRECISION > 2
    r20, ref, m = R.precision_restated(form, data, 0, "asc", bits=20)
    worse = r20 / rms["asc"]
    assert 1.5 < float(worse.min()) and float(worse.max()) < R.K_PRECISION, worse
    x, w = R.precision_inputs(form, data, 0)
    err = float((R.wino_restate(x, w, order="asc", bits=20).double() - ref).abs().max())
    assert err <= 5e-5 * max(1., float(ref.abs().max()))  # the present criterion accepts it


def test_restatement_error_is_uneven_over_the_tile():
    """What a single global tolerance hides: the F(4x4) restatement's RMS error differs
    by more than 8x between the tile's output positions."""
    rms = R.precision_restated(("w4", 64, 1), "randn", 0, "asc")[0]
    assert float(rms.max() / rms.min()) > 8
    assert float(rms[1, 1]) == float(rms.min())
