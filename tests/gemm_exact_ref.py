"""Integer-lattice inputs on which the 1x1-conv GEMM kernels (csrc/gemm_split3.hip in both
schemes and its fused mask tail, gemm1x1.hip, gemm_lateral.hip, rpn_head.hip) and the
hipBLASLt route of vd_gemm_bias_act must equal the float64 product bit for bit; the
float64 references, the conditions under which that holds, float32 restatements of the two
split schemes (the proof that the conditions admit a correct kernel, and the place where
deliberate defects are shown to break the equality) and the case table both test files
run.  CPU only; nothing is imported from the package.

The lattice argument.  Activations are integers times q_a, weights integers times q_w,
bias, residual and top-down values integers in [-64, 64] times q = q_a q_w, all powers of
two.  Every product, every partial sum in any order, the bias and the residual added are
integers times q.  While their magnitudes stay below 2^24 q every float32 operation on
them is exact whatever the rounding mode, the FMA contraction or the summation order: the
kernel's output is the float64 result rounded to float32 without error.  The direct
condition, per output:

    sum_k |a| |w| + |bias| + |res| < 2^24 q.

With an a_bias, a is taken after relu(a + a_bias), which is exact (both on q_a's
lattice).  A weight row multiplied by a power of two 2^s keeps the argument with that
column's unit q 2^s, when the column's bias and residual are on that unit too (the
reference uses the scaled weight): `col_unit`.

The units.  q_a = 2^-4, q_w = 2^-6 (q = 2^-10), row scales 2^-6 .. 2^6: the largest
activation is 2^18 q_a = 2^14 < 65504 and the smallest 2^-4 >= 2^-10 (the fp16 scheme's
input contract, include/vosdet.h: largest magnitude in [2^-10, 65504]); 2^11 (a - fp16(a))
is at least 2^11 q_a = 2^7 and at most 2^17, a normal fp16; weights lie in
[2^-12, 2^18], biases from 2^-16 and outputs below 2^24 q 2^6 = 2^20: all inside float32's
normal range.

The pieces then limit the operand widths ("bits": the span from the highest to the lowest
set bit of the integer, `significant_bits`).  A split keeps every bit of an operand whose
span fits the pieces, and the kernel keeps only some piece products, so a class names
which are non-zero:

six-product bf16 scheme (8-bit pieces; a_i w_j kept for i + j <= 2)
  narrow  a, w <= 2 bits (+-1..3), dense: only a0 w0.  Shapes, pipeline, indexing, any K.
  w3      a <= 3 bits, w 18 bits built as t 2^10 +- u (t of 8 bits, u odd of 9 bits: the
          second piece rounds u to 8 bits and leaves +-1): a0 w0, a0 w1, a0 w2.
  a3      the mirror: a0 w0, a1 w0, a2 w0.
  mid     a, w 10 bits built as 4 t +- 1: a0 w0, a0 w1, a1 w0, a1 w1.
three-product fp16 scheme (11-bit pieces; S r (a . w) ~= a0 Wr + a1 W0 + a0 Wm)
  narrow  as above: only a0 Wm.
  w2      a <= 3 bits, w 18 bits built as t 2^7 +- u (t of 11 bits, u odd below 2^6):
          a1 = 0, a0 Wm + a0 Wr exact (W0 is rounded, and multiplies nothing).
  a2      a 18 bits (the same construction), w <= 3 bits: Wr = 0, a0 Wm + a1 W0 exact.
fp32-MFMA kernels and hipBLASLt (no pieces)
  narrow, and wide: a, w 10 bits (4 t +- 1), sparse: a route that quietly computes in
  reduced precision (operands of fewer than 10 bits, an accumulator of fewer than 24)
  fails there.

The wide classes leave 3 to 4 bits below 2^24 q (an 18 x 3 or a 10 x 10 bit product is
21 or 20 bits), so they run dense at K = 16 and with both operands non-zero with
probability sqrt(6 / K) at deeper K (six products an output on average).  Besides the
direct condition a piece condition is held: sum_k (sum_i |a_i|) (sum_j |w_j|) + |bias| +
|res| < 2^24 q, the bound on every partial sum of piece products (a piece can exceed its
operand in magnitude by one rounding)."""
import functools
import math
from collections import namedtuple

import torch

from tests.conv_exact_ref import LIMIT, significant_bits  # noqa: F401  (re-exported)
from tests.test_gemm_h2_cpu import split_a, split_w
from tests.test_split3_cpu import split3

Q_A, Q_W = 2.0 ** -4, 2.0 ** -6
Q = Q_A * Q_W
B_MAX = 64          # bias, residual, top-down: integers in [-64, 64] times the column unit
STAGE = 16          # fp32 K per pipeline stage of the split kernels
S = 2048.0          # the fp16 scheme's common scale

# class -> (bits of a, bits of w) its operands may span
CLASS_BITS = {"narrow": (2, 2), "w3": (3, 18), "a3": (18, 3), "mid": (10, 10),
              "w2": (3, 18), "a2": (18, 3), "wide": (10, 10)}
BF16_CLASSES = ("narrow", "w3", "a3", "mid")
FP16_CLASSES = ("narrow", "w2", "a2")


def schemes_of(cls):
    return tuple(s for s, cs in (("bf16", BF16_CLASSES), ("fp16", FP16_CLASSES)) if cls in cs)


# ------------------------------------------------------------------ generators
def _sign(g, shape):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


def _keep(g, shape, p):
    return (torch.rand(shape, generator=g, dtype=torch.float64) < p).double()


def _small(g, shape, p, vmax):
    """Integers +-1..vmax, non-zero with probability p."""
    mag = torch.randint(1, vmax + 1, shape, generator=g).double()
    return mag * _sign(g, shape) * _keep(g, shape, p)


def _built(g, shape, p, t_lo, t_hi, shift, u_lo, u_hi):
    """+-(t 2^shift +- u), t in [t_lo, t_hi), u odd in [u_lo, u_hi]: the leading piece is
    t 2^shift exactly (u < 2^(shift - 1)) and the rest is never zero."""
    t = torch.randint(t_lo, t_hi, shape, generator=g).double()
    u = torch.randint(u_lo // 2, u_hi // 2 + 1, shape, generator=g).double() * 2 + 1
    return (t * 2.0 ** shift + u * _sign(g, shape)) * _sign(g, shape) * _keep(g, shape, p)


def operand(g, shape, kind, p):
    """Integers (float64) of one width kind: 's2' +-1..3, 's3' +-1..7, 'b18' 18 bits in
    three bf16 pieces, 'h18' 18 bits in two fp16 pieces, 'm10' 10 bits in two bf16 pieces.
    The 18-bit kinds keep t in the lower quarter of its range: 16 dense products of 18 x 3
    bits then stay below 2^24."""
    if kind == "s2":
        return _small(g, shape, p, 3)
    if kind == "s3":
        return _small(g, shape, p, 7)
    if kind == "b18":
        return _built(g, shape, p, 128, 160, 10, 257, 511)
    if kind == "h18":
        return _built(g, shape, p, 1024, 1280, 7, 1, 63)
    if kind == "m10":
        return _built(g, shape, p, 128, 256, 2, 1, 1)
    raise ValueError(kind)


# class -> (kind of a, kind of w)
KINDS = {"narrow": ("s2", "s2"), "w3": ("s3", "b18"), "a3": ("b18", "s3"), "mid": ("m10", "m10"),
         "w2": ("s3", "h18"), "a2": ("h18", "s3"), "wide": ("m10", "m10")}


def density(fam, cls, K):
    """Both operands' non-zero probability: dense, but sqrt(6 / K) in a wide class past
    K = 16 (sqrt(16 / K) for the RPN head, whose a_bias and ReLU leave 3 / 8 of them)."""
    if cls == "narrow" or K <= STAGE:
        return 1.0
    return math.sqrt((16.0 if fam == "rpn" else 6.0) / K)


# ------------------------------------------------------------------ the cases
# fam: "split" (gemm_split3_bias_act / gemm_h2_bias_act), "g1x1", "dual", "lateral", "rpn",
# "blas".  form / arg: "plain"; "res"; "up" (H, W, images); "sub" (H, W, images); "a2" K2;
# "abias"; "abias_res"; "abias_sub" (H, W, images).  M: output rows.
Case = namedtuple("Case", "fam cls M K N form arg seed")


# seeds moved on where the first one left an output column of a one-row case at exactly 0
# (tests/test_gemm_exact_cpu.py holds every case to its coverage conditions)
SEED_BUMP = {("split", "narrow", 1, 32, 256, "plain"): 11,
             ("g1x1", "narrow", 1, 64, 256, "res"): 27, ("g1x1", "narrow", 1, 128, 512, "res"): 3,
             ("dual", "narrow", 1, 128, 256, "a2"): 5, ("rpn", "wide", 1, 128, 15, "abias"): 2}


def case(fam, cls, M, K, N, form="plain", arg=None):
    seed = (((M * 131 + K) * 131 + N) * 131 + sum(map(ord, fam + cls + form))) % (2 ** 31)
    seed += SEED_BUMP.get((fam, cls, M, K, N, form), 0)
    return Case(fam, cls, M, K, N, form, arg, seed)


def _maps(form, H, W, n=3):
    if form == "up":
        return n * H * W
    return n * ((H + 1) // 2) * ((W + 1) // 2)


SPLIT_WIDE = ("w3", "a3", "mid", "w2", "a2")
SPLIT_DEPTH = [case("split", "narrow", 257, K, 256) for K in (16, 32, 48, 64, 1024)]
SPLIT_TILES = [case("split", "narrow", M, 32, N) for N in (64, 128, 256)
               for M in (1, 127, 128, 129, 255, 256, 257)]
# 3 x 3 tiles of 256 x 256, 3 x 6 of 256 x 128, 3 x 12 of 256 x 64, 6 x 6 of 128 x 128: none
# a multiple of 8 (the single-tile counts are in SPLIT_TILES)
SPLIT_ORDER = [case("split", "narrow", 3 * 256 - 5, 32, 768)]
SPLIT_WIDTH = [case("split", c, 257, 16, 256) for c in SPLIT_WIDE]
SPLIT_WIDTH_DEEP = [case("split", c, 257, 256, 256) for c in SPLIT_WIDE]   # cfg 2 and 4


def _forms(cls):
    K = 64 if cls == "narrow" else 16
    out = [case("split", cls, 257, K, 128, "res")]
    out += [case("split", cls, _maps("up", h, w), K, 128, "up", (h, w, 3))
            for h, w in ((2, 2), (6, 10), (4, 34))]
    out += [case("split", cls, _maps("sub", h, w), K, 128, "sub", (h, w, 3))
            for h, w in ((11, 17), (1, 1), (2, 3))]
    out += [case("split", cls, 257, 128, 128, "a2", 64), case("split", cls, 257, 64, 128, "a2", 16)]
    out += [case("split", cls, 257, K, 128, "abias"), case("split", cls, 257, K, 128, "abias_res"),
            case("split", cls, _maps("sub", 11, 17), K, 128, "abias_sub", (11, 17, 3))]
    return out


SPLIT_FORMS = _forms("narrow") + _forms("w3") + _forms("w2")
SPLIT = SPLIT_DEPTH + SPLIT_TILES + SPLIT_ORDER + SPLIT_WIDTH + SPLIT_WIDTH_DEEP + SPLIT_FORMS

G1X1_SHAPES = ((64, 256), (64, 64), (256, 64), (128, 512))
G1X1 = [case("g1x1", c, M, K, N, "res") for (K, N) in G1X1_SHAPES for M in (1, 15, 16, 17, 1003)
        for c in ("narrow", "wide")]
DUAL = [case("dual", c, M, 128, 256, "a2", 64) for M in (1, 17, 1003) for c in ("narrow", "wide")]
LATERAL = [case("lateral", c, _maps("up", h, w), K, 256, "up", (h, w, 3))
           for K in (256, 512, 1024) for h, w in ((2, 2), (6, 10), (38, 50))
           for c in ("narrow", "wide")]
# (N, C, H, W, A) -> M = N H W pixels, K = C, N = 5 A outputs; arg = (N, H, W, A)
RPN = [case("rpn", c, n * h * w, C, 5 * A, "abias", (n, h, w, A))
       for (n, C, h, w, A) in ((3, 64, 7, 11, 1), (1, 128, 1, 1, 3), (2, 256, 5, 13, 3))
       for c in ("narrow", "wide")]
BLAS = [case("blas", c, M, K, N, "res")
        for (M, K, N) in ((777, 64, 128), (100, 32, 96), (1, 128, 32)) for c in ("narrow", "wide")]
FP32 = G1X1 + DUAL + LATERAL + RPN + BLAS
ALL_CASES = SPLIT + FP32

# the cases built on the device (dense narrow class, integers +-1..3): their condition is
# the data-free bound 9 K + 2 B_MAX < 2^24
G1X1_SECOND_PASS = (65536 + 16 * 8 + 3, 64, 64)   # M, K, N: 512 workgroups x 128 rows, + ragged
LATERAL_BIG_K = 256


def free_bound(K):
    return (9.0 * K + 2 * B_MAX) / LIMIT


def case_id(c):
    a = "" if c.arg is None else "-" + ("x".join(map(str, c.arg)) if isinstance(c.arg, tuple)
                                        else str(c.arg))
    return "%s-%s-%dx%dx%d-%s%s" % (c.fam, c.cls, c.M, c.K, c.N, c.form, a)


Inputs = namedtuple("Inputs", "a a2 a_bias w bias res col_unit")


def _in_rows(c):
    """Rows of the `a` the kernel is given (a stride-2 form reads a larger map)."""
    if c.form in ("sub", "abias_sub"):
        h, w, n = c.arg
        return n * h * w
    return c.M


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The case's operands as float32 CPU tensors (shared, never modified): a [rows, K1],
    a2 [M, K2] or None, a_bias [K1] or None, w [N, K], bias [N], res (the residual [M, N],
    or the top-down map [M / 4, N]) or None, col_unit [N] float64 (q times the row scale).
    The split cases' weight rows carry scales 2^-6 .. 2^6 and one all-zero row; the fp32
    families always have a residual (the tests run them with and without it)."""
    g = torch.Generator(device="cpu").manual_seed(c.seed)
    ka, kw = KINDS[c.cls]
    p = density(c.fam, c.cls, c.K)
    K2 = c.arg if c.form == "a2" else 0
    K1 = c.K - K2
    a = operand(g, (_in_rows(c), K1), ka, p)
    a2 = operand(g, (c.M, K2), ka, p) if K2 else None
    ab = None
    if c.form.startswith("abias"):
        if c.fam == "rpn" and c.cls == "wide":
            # relu(a + a_bias) stays 0 or a 10-bit value: a_bias 0, or past every a
            ab = -4096.0 * (torch.rand(K1, generator=g) < 0.25).double()
        elif c.fam == "rpn":
            ab = torch.randint(-4, 5, (K1,), generator=g).double()
        else:  # narrow: relu(a + a_bias) in 0..3; w3 / w2 (a <= 3 bits): in 0..7
            ab = torch.randint(-2, 1 if c.cls == "narrow" else 5, (K1,), generator=g).double()
            if c.cls != "narrow":
                a = _small(g, a.shape, p, 3)
    w = operand(g, (c.N, c.K), kw, p)
    scale = torch.ones(c.N, dtype=torch.float64)
    if c.fam == "split":
        scale = torch.exp2(torch.randint(-6, 7, (c.N,), generator=g).double())
        w[(c.seed % c.N)] = 0
    unit = Q * scale
    bias = torch.randint(-B_MAX, B_MAX + 1, (c.N,), generator=g).double()
    bias[bias == 0] = 1   # a column whose weight row is zero still has an output
    res = None
    if c.form in ("res", "abias_res", "up"):
        rows = c.M // 4 if c.form == "up" else c.M
        res = torch.randint(-B_MAX, B_MAX + 1, (rows, c.N), generator=g).double() * unit
    out = Inputs(a * Q_A, None if a2 is None else a2 * Q_A, None if ab is None else ab * Q_A,
                 w * Q_W * scale.view(-1, 1), bias * unit, res, unit)
    for t in out[:6]:
        assert t is None or torch.equal(t.float().double(), t)
    return Inputs(*[None if t is None else t.float() for t in out[:6]], unit)


# ------------------------------------------------------------------ index arithmetic
def sub_rows(H, W, n, image_offset=True):
    """Input row of every output row of a stride-2 read of n maps of H x W.
    image_offset False: (mutation) every image reads the first one's rows."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    m = torch.arange(n * Ho * Wo)
    img, rem = m // (Ho * Wo), m % (Ho * Wo)
    y, x = rem // Wo, rem % Wo
    return ((img if image_offset else 0) * H + 2 * y) * W + 2 * x


def up_rows(H, W, n, dx=0):
    """Top-down row (of n maps of H/2 x W/2) of every pixel of n maps of H x W.
    dx 1: (mutation) the row taken at x / 2 + 1 (held inside the map)."""
    m = torch.arange(n * H * W)
    img, rem = m // (H * W), m % (H * W)
    y, x = rem // W, rem % W
    xs = torch.clamp(x // 2 + dx, max=W // 2 - 1) if dx else x // 2
    return (img * (H // 2) + y // 2) * (W // 2) + xs


def gathered(c, mutate=None):
    """(A [M, K] float32 as the GEMM sees it -- relu(a + a_bias), the stride-2 rows, a2's
    columns appended --, the residual rows [M, N] or None)."""
    i = inputs(c)
    a = i.a
    if i.a_bias is not None:
        a = torch.relu(a + i.a_bias)
    if c.form in ("sub", "abias_sub"):
        h, w, n = c.arg
        a = a[sub_rows(h, w, n, image_offset=mutate != "sub_image")]
    if i.a2 is not None:
        a = torch.cat([a, i.a2], 1)
    if mutate == "row_next":
        a = a[torch.clamp(torch.arange(c.M) + 1, max=c.M - 1)]
    res = i.res
    if c.form == "up":
        h, w, n = c.arg
        res = res[up_rows(h, w, n, dx=1 if mutate == "up_x" else 0)]
    return a, res


@functools.lru_cache(maxsize=None)
def reference(c, res=True):
    """a @ w.T + bias (+ residual) in float64, before the activation."""
    a, r = gathered(c)
    i = inputs(c)
    y = a.double() @ i.w.double().t() + i.bias.double()
    if res and r is not None:
        y = y + r.double()
    return y


# ------------------------------------------------------------------ conditions
def pieces(c):
    """(sum_i |a_i| [M, K], sum_j |w_j| [N, K]) float64: the magnitudes the kept piece
    products are bounded by, per scheme; the operands themselves for the fp32 families."""
    a, _ = gathered(c)
    w = inputs(c).w
    if c.fam != "split":
        return {"fp32": (a.double().abs(), w.double().abs())}
    out = {}
    for sch in schemes_of(c.cls):
        if sch == "bf16":
            pa = sum(p.double().abs() for p in split3(a))
            pw = sum(p.double().abs() for p in split3(w))
        else:
            a0, a1 = split_a(a)
            wm, wr, w0, sc = split_w(w)
            pa = a0.double().abs() + a1.double().abs() / S
            # a1 multiplies W0 = fp16(r w), a0 multiplies Wm + Wr: the larger of the two
            pw = torch.maximum(wm.double().abs() + wr.double().abs(), w0.double().abs() * S) \
                * sc.double().view(-1, 1)
        out[sch] = (pa, pw)
    return out


def condition(c):
    """The largest of the direct and the piece conditions over 2^24 times the column's
    unit: below 1 the arithmetic is exact."""
    a, r = gathered(c)
    i = inputs(c)
    extra = i.bias.double().abs()
    if r is not None:
        extra = extra + r.double().abs()
    lim = LIMIT * i.col_unit
    v = float(((a.double().abs() @ i.w.double().abs().t() + extra) / lim).max())
    for pa, pw in pieces(c).values():
        v = max(v, float(((pa @ pw.t() + extra) / lim).max()))
    return v


# ------------------------------------------------------------------ float32 restatements
BF16_PRODUCTS = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))   # (a piece, w piece), as issued
FP16_PRODUCTS = ("a0Wr", "a1W0", "a0Wm")


def _stages(K, order, skip):
    ks = [k for n, k in enumerate(range(0, K, STAGE)) if n != skip]
    return ks[::-1] if order == "desc" else ks


def restate_bf16(a, w, bias, res=None, relu=False, order="asc", drop=None, skip=None):
    """The six-product scheme in float32: three bf16 pieces per operand (split3), per
    16-deep stage the six kept products into one float32 accumulator, then (acc + bias) +
    res.  order: the stages ascending or descending.  drop: one (i, j) product left out;
    skip: one stage left out."""
    A, W = split3(a), split3(w)
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in _stages(a.shape[1], order, skip):
        s = slice(k, k + STAGE)
        for (i, j) in BF16_PRODUCTS:
            if (i, j) != drop:
                acc = acc + A[i][:, s] @ W[j][:, s].t()
    y = acc + bias
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def restate_fp16(a, w, bias, res=None, relu=False, order="asc", drop=None, skip=None,
                 w0_for_wm=False, scale_off=False):
    """The three-product scheme in float32 (split_a / split_w): per 16-deep stage
    acc += a0 Wr; acc += a1 W0; acc += a0 Wm, then acc / (S r_n), + bias, + res.
    w0_for_wm: S W0 where Wm + Wr belongs; scale_off: the row scale one exponent off."""
    a0, a1 = (t.float() for t in split_a(a))
    wm, wr, w0, sc = split_w(w)
    wm, wr, w0 = wm.float(), wr.float(), w0.float()
    if w0_for_wm:
        wm, wr = w0 * S, torch.zeros_like(wr)
    if scale_off:
        sc = sc * 2
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in _stages(a.shape[1], order, skip):
        s = slice(k, k + STAGE)
        if drop != "a0Wr":
            acc = acc + a0[:, s] @ wr[:, s].t()
        if drop != "a1W0":
            acc = acc + a1[:, s] @ w0[:, s].t()
        if drop != "a0Wm":
            acc = acc + a0[:, s] @ wm[:, s].t()
    y = acc * sc + bias
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def restate_fp32(a, w, bias, res=None, relu=False, order="asc", skip=None, bits=None):
    """A float32 GEMM in 16-deep stages.  bits: both operands rounded to that many
    significant bits (a reduced-precision route)."""
    if bits is not None:
        from tests.conv_exact_ref import round_bits
        a, w = round_bits(a, bits), round_bits(w, bits)
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in _stages(a.shape[1], order, skip):
        acc = acc + a[:, k:k + STAGE] @ w[:, k:k + STAGE].t()
    y = acc + bias
    if res is not None:
        y = y + res
    return torch.relu(y) if relu else y


def restate(c, scheme, mutate=None, **kw):
    """The case through its scheme's restatement.  mutate: an index defect of `gathered`
    ("row_next", "up_x", "sub_image") or "a2_cols" (the second operand's weight columns
    applied to the first: K1 = K2 only)."""
    a, r = gathered(c, mutate)
    i = inputs(c)
    w = i.w
    if mutate == "a2_cols":
        K1 = c.K - c.arg
        w = torch.cat([w[:, K1:], w[:, :K1]], 1)
    f = {"bf16": restate_bf16, "fp16": restate_fp16, "fp32": restate_fp32}[scheme]
    return f(a, w, i.bias, r, **kw)


# ------------------------------------------------------------------ the fused mask tail
# x [R P P, 256] -> y = relu(x @ w_up.T + b_up) [.., (i, j, co)] -> z = sum_co w_cls[ch][co]
# y[i, j, co] + b_cls[ch] -> sigmoid.  Units: x on q_a, w_up on q_w, b_up on q, w_cls on
# Q_C, b_cls and z on Q_Z = q Q_C = 2^-8 (the smallest non-zero |z|: exp(-z) is well away
# from 1).  The condition extends by the second sum: sum |w_cls| y + |b_cls| < 2^24 Q_Z.
# Class channel 0 is a planted sweep: its classify row is Q_C at channel 0 alone, the
# upconv rows of channel 0 read x[:, 0] alone with bias (i, j) index times q, and b_cls is
# -16: in a RoI of class 0, z = (x0 / q_a + 2 i + j) Q_Z - 16 with x0 = 42 pixel q_a up to
# 8189 q_a (13 bits: two pieces of either scheme, times a one-piece weight) -- exact z over
# [-16, 16] --, but 4096 q_a at the RoI's middle pixel: z = 0 at tap (0, 0).
Q_C = 4.0
Q_Z = Q * Q_C
MASK_CLASSES = 5
MaskCase = namedtuple("MaskCase", "R P ch seed")
MASK = [MaskCase(1, 14, (4,), 11), MaskCase(3, 14, (0, 4, 2), 12),
        MaskCase(5, 7, (4, 0, 1, 3, 0), 13), MaskCase(2, 1, (0, 4), 14)]
MaskInputs = namedtuple("MaskInputs", "x w_up b_up w_cls b_cls ch")


def mask_id(c):
    return "mask-%dx%d" % (c.R, c.P)


@functools.lru_cache(maxsize=None)
def mask_inputs(c):
    g = torch.Generator(device="cpu").manual_seed(c.seed)
    PP = c.P * c.P
    x = _small(g, (c.R * PP, 256), 1.0, 3)
    w_up = _small(g, (1024, 256), 1.0, 3)
    b_up = torch.randint(-B_MAX, B_MAX + 1, (1024,), generator=g).double()
    w_cls = _small(g, (MASK_CLASSES, 256), 1.0, 3)
    b_cls = torch.randint(-B_MAX, B_MAX + 1, (MASK_CLASSES,), generator=g).double()
    w_cls[0] = 0
    w_cls[0, 0] = 1
    b_cls[0] = -16 / Q_Z
    for ij in range(4):
        w_up[256 * ij] = 0
        w_up[256 * ij, 0] = 1
        b_up[256 * ij] = ij
    for r, ch in enumerate(c.ch):
        if ch == 0:
            sweep = 42.0 * torch.arange(PP, dtype=torch.float64)
            x[r * PP:(r + 1) * PP, 0] = torch.clamp(sweep, max=8189)
            x[r * PP + PP // 2, 0] = 4096
    out = (x * Q_A, w_up * Q_W, b_up * Q, w_cls * Q_C, b_cls * Q_Z)
    for t in out:
        assert torch.equal(t.float().double(), t)
    return MaskInputs(*[t.float() for t in out], torch.tensor(c.ch, dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def mask_logits(c):
    """(z [R, 2P, 2P] float64 exact, the mask condition's largest value over 2^24)."""
    i = mask_inputs(c)
    R, P = c.R, c.P
    x, w, b = i.x.double(), i.w_up.double(), i.b_up.double()
    y = torch.relu(x @ w.t() + b).view(R, P, P, 2, 2, 256)
    wc = i.w_cls.double()[i.ch.long()]
    bc = i.b_cls.double()[i.ch.long()]
    z = torch.einsum("rhwijc,rc->rhiwj", y, wc).reshape(R, 2 * P, 2 * P) + bc.view(-1, 1, 1)
    c1 = float((x.abs() @ w.abs().t() + b.abs()).max()) / (LIMIT * Q)
    c2 = float((torch.einsum("rhwijc,rc->rhiwj", y, wc.abs()) + bc.abs().view(-1, 1, 1, 1, 1)).max()
               ) / (LIMIT * Q_Z)
    return z, max(c1, c2)
