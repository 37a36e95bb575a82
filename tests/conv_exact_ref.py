"""Integer-lattice inputs on which the 3x3 conv kernels (csrc/conv3x3.hip,
conv3x3_wino.hip, conv3x3_wino4.hip) and the stem (csrc/stem.hip) must equal the
float64 convolution bit for bit, the float64 references, the conditions under which
that holds, a float32 restatement of the Winograd arithmetic (the proof that the
conditions admit a correct kernel), the per-tile-position precision criterion, and the
case table both test files run.  CPU only.

The lattice argument.  The Winograd data transforms use only the constants 4, 5, 2, 8
and +-1 (B^T, A^T below); the weight transform uses 1/4, 1/6, 1/12, 1/24 and 1 (F(4x4))
or 1/2 and 1 (F(2x2)).  With the weights multiples of 576 q_w (F(4x4); 4 q_w for
F(2x2), q_w for the direct kernels) and the data multiples of q_d, q_w and q_d powers of
two, U = G g G^T is an integer times q_w, V = B^T d B an integer times q_d, and every
product, every partial sum in any order and the output transform are integers times
q = q_w q_d.  While their magnitudes stay below 2^24 q, every float32 operation on them
is exact whatever the rounding mode, the FMA contraction or the accumulation order, and
so is a split of an operand into bf16 pieces that keeps all its bits.  The kernel's
output is then the float64 convolution, rounded to float32 without error.

Two conditions bound those magnitudes (each must stay below 2^24 q):
  data-dependent  S = |A^T| [ sum_ci |U| (.) (|B^T| |d| |B|) ] |A| + |bias|, the maps
                  tiled from their own origin: the plain launch, pairs, octets, the
                  tile-aligned stacks (every tile sits in one map at that offset);
  data-free       d_max |A^T| [ (sum_ci |U|) (.) (r r^T) ] |A| + |bias|, r the row sums
                  of |B^T| (F(4x4): 10, 10, 10, 6, 6, 10): any tile alignment and any
                  neighbour, for the grid (tiles straddle maps) and the dilated sub-maps.
For the direct kernels the condition is sum |w| |x| + |bias|.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

LIMIT = 2.0 ** 24

# ------------------------------------------------------------------ transform matrices
# restated from the kernels' comments (conv3x3_wino4.hip: w4_bt6, w4_at6,
# wino4_weight_kernel; conv3x3_wino.hip: transform, the output transform,
# wino_weight_kernel), not imported from the package
BT4 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0],
       [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
G4 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6],
      [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G2 = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]


def mats(m):
    """(B^T, G, A^T) of F(m x m, 3x3) as float64 tensors, m = 4 or 2."""
    bt, g, at = (BT4, G4, AT4) if m == 4 else (BT2, G2, AT2)
    return (torch.tensor(bt, dtype=torch.float64), torch.tensor(g, dtype=torch.float64),
            torch.tensor(at, dtype=torch.float64))


# ------------------------------------------------------------------ lattices
# kind -> (q_d, q_w, weight unit in q_w).  All values then lie between about 2^-8 (the
# smallest U, q_w) and 2^16 (2^24 q), far from float32's subnormals.
UNITS = {"w4": (2.0 ** -2, 2.0 ** -6, 576),   # w = +-9, U from 2^-6, y < 2^16
         "w2": (2.0 ** -2, 2.0 ** -6, 4),     # G holds 1/2: w = +-1/16
         "gemm": (2.0 ** -2, 2.0 ** -6, 1),
         "stem": (1.0, 2.0 ** -12, 1)}
B_MAX = 64  # bias: integers in [-64, 64] times q


def q_of(kind):
    qd, qw, _ = UNITS[kind]
    return qd * qw


def _ints(g, shape, p, vmax):
    """Integers in [-vmax, vmax], nonzero with probability p, as float64."""
    mag = torch.randint(1, vmax + 1, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    keep = (torch.rand(shape, generator=g, dtype=torch.float64) < p).double()
    return mag * sign * keep


def lattice(kind, N, C, H, W, Co, seed, p_d, p_w, d_max, groups=1, w_max=1):
    """(x [N, C, H, W], w [Co, C / groups, k, k], bias [Co]) float32 on the lattice of
    `kind`: x integers in [-d_max, d_max] times q_d (nonzero with probability p_d), w
    integers in [-w_max, w_max] times unit q_w (nonzero with probability p_w), bias
    integers times q.  k = 7 for the stem, else 3."""
    qd, qw, unit = UNITS[kind]
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 7 if kind == "stem" else 3
    x = _ints(g, (N, C, H, W), p_d, d_max) * qd
    w = _ints(g, (Co, C // groups, k, k), p_w, w_max) * (unit * qw)
    b = torch.randint(-B_MAX, B_MAX + 1, (Co,), generator=g).double() * (qd * qw)
    for t in (x, w, b):
        assert torch.equal(t.float().double(), t)
    return x.float(), w.float(), b.float()


# ------------------------------------------------------------------ float64 references
def conv64(x, w, b=None, relu=False, groups=1, dilation=1):
    """act(conv3x3(x, pad = dilation) + bias) in float64."""
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=dilation,
                 dilation=dilation, groups=groups)
    return F.relu(y) if relu else y


def stem64(x, w, b):
    """MaxPool 3x3 / 2 pad 1 (relu(conv 7x7 / 2 pad 3 (x) + bias)) in float64."""
    y = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3)
    return F.max_pool2d(F.relu(y), 3, 2, 1)


def dense_weight(w, groups):
    """A grouped conv's weight [C][C / groups][3][3] as the dense [C][C][3][3] one."""
    if groups == 1:
        return w
    Co, cpg = w.shape[:2]
    opg = Co // groups
    wd = torch.zeros((Co, cpg * groups, 3, 3), dtype=w.dtype)
    for co in range(Co):
        gi = co // opg
        wd[co, gi * cpg:(gi + 1) * cpg] = w[co]
    return wd


# ------------------------------------------------------------------ exactness conditions
def u64(w, m, G=None):
    """U = G g G^T in float64, [Co][Ci][m + 2][m + 2], through the integer matrix 24 G
    (2 G for F(2x2)): on a lattice weight every step is an exact integer operation, where
    1/6 as a double is not."""
    s = 24.0 if m == 4 else 2.0
    Gi = ((mats(m)[1] if G is None else G) * s).round()
    return torch.einsum("ak,oikl,bl->oiab", Gi, w.double(), Gi) / (s * s)


def u_as_kernel(w, m):
    """U as the weight kernels compute it: G's entries as doubles (1 / 6 rounded), the
    products in double, one rounding to float32.  Every nonzero lattice U comes out
    exact.  Where the exact U is 0 through cancellation (g0 + g1 + g2 = 0 under a row of
    sixths) the rounded 1 / 6 can leave a residue of some 1e-17 |w| instead, F(4x4) only;
    which, depends on the FMA contraction of the build.  Its products (below 1e-14) are
    absorbed by the first nonzero lattice value they are added to (at least q = 2^-8,
    ulp 2^-32), so they reach an output only if every other term of that output is zero
    at every stage; the restatement fed with this U stays exact on every table case."""
    G = mats(m)[1]
    t = torch.einsum("ak,oikl->oial", G, w.double())
    return torch.einsum("oial,bl->oiab", t, G).float()


def _tiles(x, m, pad_mode="zeros", shift=0):
    """The (m + 2)^2 patches of x's pad-1 image, tiled from the map's origin:
    [N][C][th][tw][m + 2][m + 2]."""
    H, W = x.shape[2:]
    eh, ew = -H % m, -W % m
    if pad_mode == "replicate":  # (mutation) a padding tap read as the neighbouring pixel
        xp = F.pad(F.pad(x, (1, 1, 1, 1), mode="replicate"), (0, ew, 0, eh))
    else:
        xp = F.pad(x, (1 + shift, 1 + ew - shift, 1, 1 + eh))
    return xp.unfold(2, m + 2, m).unfold(3, m + 2, m)


def cond_data(x, w, b, m, groups=1):
    """The data-dependent condition's largest value, in units of q's float (compare
    with LIMIT * q): S = |A^T| [sum_ci |U| (.) (|B^T| |d| |B|)] |A| + |bias|."""
    bt, _, at = mats(m)
    U = u64(dense_weight(w, groups), m).abs()
    V = torch.einsum("ak,nihwkl,bl->nihwab", bt.abs(), _tiles(x.double().abs(), m), bt.abs())
    M = torch.einsum("oiab,nihwab->nohwab", U, V)
    S = torch.einsum("ak,nohwkl,bl->nohwab", at.abs(), M, at.abs())
    if b is not None:
        S = S + b.double().abs().view(1, -1, 1, 1, 1, 1)
    return float(S.max())


def cond_free(w, b, x_max, m, groups=1):
    """The data-free condition: x_max |A^T| [(sum_ci |U|) (.) (r r^T)] |A| + |bias|, r the
    row sums of |B^T|; x_max the largest |x| (d_max q_d)."""
    bt, _, at = mats(m)
    r = bt.abs().sum(dim=1)
    U = u64(dense_weight(w, groups), m).abs().sum(dim=1) * torch.outer(r, r)
    S = x_max * torch.einsum("ak,okl,bl->oab", at.abs(), U, at.abs())
    if b is not None:
        S = S + b.double().abs().view(-1, 1, 1)
    return float(S.max())


def cond_direct(x, w, b, stride=1, pad=1):
    """The direct kernels' condition: sum |w| |x| + |bias|."""
    S = F.conv2d(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(),
                 stride=stride, padding=pad)
    return float(S.max())


def significant_bits(t, q):
    """The most significant bits any element of t (integers times q) needs."""
    v = (t.double().abs() / q).round().long().view(-1)
    v = v[v > 0]
    bits = 0
    for e in v.unique().tolist():
        while e % 2 == 0:
            e //= 2
        bits = max(bits, e.bit_length())
    return bits


# The split-bf16 stem keeps six of the nine piece products of a three-way bf16 split,
# x_i w_j with i + j <= 2 (gemm_split3.hip's scheme); the dropped ones all hold a second
# or third piece of both operands or a third piece of one.  An operand of at most 8
# significant bits is one bf16 piece (pieces 2 and 3 are zero), one of at most 16 is two
# (piece 3 is zero): with 8 bits on one side and 16 on the other every nonzero piece
# product is x_0 w_0, x_0 w_1 (or x_1 w_0) -- all kept -- and a product of two 8-bit
# pieces is exact in the MFMA's float32 accumulator.
STEM_BITS = ((8, 16), (16, 8))


def stem_bits_ok(x, w):
    bx, bw = significant_bits(x, UNITS["stem"][0]), significant_bits(w, UNITS["stem"][1])
    return any(bx <= a and bw <= b for a, b in STEM_BITS), (bx, bw)


# ------------------------------------------------------------------ float32 restatement
def round_bits(t, bits):
    """float32 t rounded (to nearest, ties away) to `bits` mantissa bits, the implicit
    one included."""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e).float()


def wino_restate(x, w, b=None, relu=False, m=4, order="torch", groups=1, bits=None,
                 mutate=None, U=None):
    """act(conv3x3(x, pad 1) + bias) by Winograd F(m x m, 3x3) in float32, as the kernels
    compute it: U = G g G^T in float64 rounded once, V = B^T d B, M = sum_ci U (.) V per
    transform position, Y = A^T M A, + bias.  order: the channel sum "torch" (one batched
    matmul), "asc" (ascending, one channel at a time) or "mfma4" (in groups of four, as
    a 16x16x4 MFMA takes them).  bits: both MFMA operands rounded to that many mantissa
    bits.  mutate: one deliberate defect ("bt", "tap", "shift", "chunk", "pad")."""
    bt, G, at = mats(m)
    wd = dense_weight(w, groups)
    if mutate == "bt":
        bt = bt.clone()
        bt[1, 1] += 1
    if mutate == "tap":
        wd = wd.clone()
        wd[:, :, 1, 1] = 0
    U = u64(wd, m, G).float() if U is None else U
    btf, atf = bt.float(), at.float()
    d = _tiles(x, m, "replicate" if mutate == "pad" else "zeros", 1 if mutate == "shift" else 0)
    V = torch.einsum("ak,nihwkl->nihwal", btf, d)
    V = torch.einsum("nihwal,bl->nihwab", V, btf)
    if bits is not None:
        U, V = round_bits(U, bits), round_bits(V, bits)
    C = U.shape[1] - (8 if mutate == "chunk" else 0)
    N, _, th, tw = V.shape[:4]
    if order == "torch":
        M = torch.einsum("oiab,nihwab->nohwab", U[:, :C], V[:, :C])
    else:
        M = torch.zeros((N, U.shape[0], th, tw, m + 2, m + 2), dtype=torch.float32)
        prod = lambda c: U[None, :, c, None, None] * V[:, None, c]
        if order == "asc":
            for c in range(C):
                M = M + prod(c)
        elif order == "mfma4":
            for c in range(0, C, 4):
                M = M + (((prod(c) + prod(c + 1)) + prod(c + 2)) + prod(c + 3))
        else:
            raise ValueError(order)
    Y = torch.einsum("ak,nohwkl->nohwal", atf, M)
    Y = torch.einsum("nohwal,bl->nohwab", Y, atf)
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(N, U.shape[0], th * m, tw * m)
    Y = Y[:, :, :x.shape[2], :x.shape[3]]
    if b is not None:
        Y = Y + b.view(1, -1, 1, 1)
    return F.relu(Y) if relu else Y.contiguous()


# ------------------------------------------------------------------ the case table
Case = namedtuple("Case", "kind N C H W Co groups cond p_d p_w d_max w_max seed")


def _params(kind, ceff, cond):
    """(p_d, p_w, d_max) by the channels one output sums over: dense small integers
    where few channels leave room below 2^24 q, thinner +-1 lattices for many."""
    if kind in ("gemm", "w2"):
        return (1.0, 1.0, 3)
    if cond == "free":
        return {8: (1.0, 1.0, 2), 16: (1.0, 0.5, 2)}[ceff]
    if ceff <= 8:
        return (1.0, 1.0, 3)
    if ceff <= 16:
        return (1.0, 0.5, 3)
    if ceff <= 24:
        return (1.0, 1.0, 1)
    if ceff <= 32:
        return (1.0, 0.5, 1)
    if ceff <= 128:
        return (0.5, 0.5, 1)
    if ceff <= 256:  # at 0.25 / 0.25 the condition comes to 1.03 .. 1.11 over twelve seeds
        return (0.25, 0.2, 1)
    return (0.125, 0.125, 1)


def case(kind, N, C, H, W, Co, groups=1, cond="data", d_max=None):
    p_d, p_w, dm = _params(kind, C // groups, cond)
    d_max = d_max or dm
    seed = ((N * 131 + C) * 131 + H) * 131 + W + Co + groups
    return Case(kind, N, C, H, W, Co, groups, cond, p_d, p_w, d_max, 1, seed)


# F(4x4) plain: (case, plans or None)
W4_PLAIN = [case("w4", 2, 8, 1, 1, 64, d_max=15),   # one chunk, one pixel (one tap: a wider
            # range keeps the 8-term sums off zero)
            case("w4", 1, 16, 5, 3, 64),      # two-chunk pipeline depth
            case("w4", 1, 24, 5, 3, 64),      # three
            case("w4", 1, 32, 5, 3, 64),      # four
            case("w4", 1, 16, 17, 33, 128),   # one past a wide block, two channel blocks
            case("w4", 1, 8, 33, 17, 64),     # one past the tall block (both plans)
            case("w4", 2, 64, 19, 35, 192),   # three channel blocks: the non-cbx mapping
            case("w4", 1, 8, 6, 6, 1024),     # sixteen channel blocks
            case("w4", 1, 256, 9, 13, 64)]    # 32 chunks
W4_PLANS = {(1, 8, 33, 17, 64): ("tall,1", "wide,1")}
W4_PAIR = [case("w4", 3, 8, 15, 15, 64), case("w4", 2, 8, 8, 9, 64)]
W4_OCTET = [case("w4", 9, 8, 7, 7, 64), case("w4", 5, 16, 1, 7, 64)]
W4_ROWS = [(case("w4", 3, 16, 25, 42, 64), ("tall,1", "wide,2", "wide,3")),
           (case("w4", 4, 16, 15, 15, 64), ("wide,4", "tall,3")),
           (case("w4", 4, 16, 16, 16, 64), ("wide,4", "tall,3")),
           (case("w4", 7, 8, 4, 4, 64), ("wide,7", "tall,2"))]
W4_GRID = [case("w4", 33, 8, 14, 14, 64, cond="free"), case("w4", 5, 8, 7, 7, 64, cond="free"),
           case("w4", 50, 8, 1, 1, 64, cond="free"), case("w4", 70, 16, 3, 40, 64, cond="free")]
W4_GROUPED = [case("w4", 2, 64, 9, 11, 64, groups=8), case("w4", 1, 128, 17, 33, 128, groups=32),
              case("w4", 1, 64, 5, 5, 64, groups=2)]
# dilation 2: (case, layouts the entry serves).  As launch_conv3x3_wino4 reads (N' = 4 N
# sub-maps of h x w = H / 2 x W / 2): one per block and the grid serve every shape here;
# pairs / octets need h, w <= 15, which 20 x 36 (w = 18) is not.
W4_DILATED = [(case("w4", 2, 8, 2, 4, 64, cond="free"), (False, "pair", "grid")),
              (case("w4", 3, 16, 14, 14, 64, cond="free"), (False, "pair", "grid")),
              (case("w4", 1, 8, 28, 30, 64, cond="free"), (False, "pair", "grid")),
              (case("w4", 2, 8, 20, 36, 128, cond="free"), (False, "grid"))]
DILATED_LAYOUTS = (False, "pair", "grid")
W2_PLAIN = [case("w2", 1, 24, 1, 1, 64), case("w2", 1, 8, 5, 3, 64),
            case("w2", 2, 16, 9, 17, 128),    # both block shapes (W <= 16 and above)
            case("w2", 1, 64, 17, 70, 192)]
W2_SEG = [case("w2", 3, 8, 2, 9, 64), case("w2", 5, 8, 6, 20, 64)]
W2_2D = [case("w2", 9, 8, 7, 7, 64), case("w2", 5, 8, 13, 21, 128)]
# implicit GEMM: Cin 64 is the smallest the entry serves (conv3x3_mfma_supported: C % 64
# == 0); Cout 64 (the narrow 256 x 64 tile), 128, 384; (2, 64, 9, 13): a ragged pixel tail
GEMM = [case("gemm", n, 64, h, w, co) for (n, h, w) in ((1, 1, 1), (1, 5, 3), (2, 9, 13))
        for co in (64, 128, 384)]
GEMM_VARIANTS = ({"VOSDET_CONV3X3_VARIANT": "1"}, {"VOSDET_CONV3X3_VARIANT": "2"},
                 {"VOSDET_CONV3X3_VARIANT": "6"}, {"VOSDET_CONV3X3_MID": "1"})


def _stem(N, H, W, wide_x):
    """wide_x: x of 12 significant bits and w of 4; else x of 4 bits and w of 12 -- each
    two bf16 pieces on one side and one on the other, 147 products below 2^24 q."""
    return Case("stem", N, 3, H, W, 64, 1, "direct", 1.0, 1.0, 4095 if wide_x else 15,
                15 if wide_x else 4095, H * 1000 + W + int(wide_x))


# (1, 29, 33): 15 x 17 conv pixels = one past the 13 x 15 under a pooled 7 x 8 tile's
# own rows / columns, so an 8th pooled row and a 9th pooled column exist
STEM = [_stem(N, H, W, wx) for (N, H, W) in ((1, 1, 1), (1, 7, 9), (2, 37, 45), (1, 29, 33))
        for wx in (False, True)]

WINO_CASES = (W4_PLAIN + W4_PAIR + W4_OCTET + [c for c, _ in W4_ROWS] + W4_GRID + W4_GROUPED
              + [c for c, _ in W4_DILATED] + W2_PLAIN + W2_SEG + W2_2D)
ALL_CASES = WINO_CASES + GEMM + STEM


def case_id(c):
    return "%s-%dx%dx%dx%d-%d%s" % (c.kind, c.N, c.C, c.H, c.W, c.Co,
                                    ("-g%d" % c.groups if c.groups > 1 else "")
                                    + ("-x" if c.kind == "stem" and c.d_max > 15 else ""))


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The case's (x, w, bias), float32, CPU; shared, never modified."""
    return lattice(c.kind, c.N, c.C, c.H, c.W, c.Co, c.seed, c.p_d, c.p_w, c.d_max,
                   groups=c.groups, w_max=c.w_max)


@functools.lru_cache(maxsize=None)
def reference(c, bias, dilation=1):
    """The float64 reference before the activation (the stem: the whole stem; its
    conv alone, for the coverage check, with bias False)."""
    x, w, b = inputs(c)
    if c.kind == "stem":
        return stem64(x, w, b) if bias else F.conv2d(x.double(), w.double(), None, 2, 3)
    return conv64(x, w, b if bias else None, groups=c.groups, dilation=dilation)


def condition(c, dilation=1):
    """The case's exactness condition over LIMIT * q: below 1 the arithmetic is exact."""
    x, w, b = inputs(c)
    q = q_of(c.kind)
    if c.kind == "stem":
        return cond_direct(x, w, b, stride=2, pad=3) / (LIMIT * q)
    if c.kind == "gemm":
        return cond_direct(x, w, b) / (LIMIT * q)
    m = 4 if c.kind == "w4" else 2
    if c.cond == "free":
        return cond_free(w, b, c.d_max * UNITS[c.kind][0], m, c.groups) / (LIMIT * q)
    return cond_data(x, w, b, m, c.groups) / (LIMIT * q)


# ------------------------------------------------------------------ precision by position
# A criterion that was measured and NOT shipped.  The plan: on real-valued data hold the
# kernels' RMS error against the float64 conv, per output position class (y mod m, x mod
# m; 16384 samples a class at PRECISION_SHAPE), to K times the RMS of wino_restate on the
# same inputs, K = 1.25 (the statistical error of such an RMS) times the largest ratio of
# that RMS between any two accumulation orders of the channel sum -- "asc" (one channel
# at a time), "mfma4" (groups of four, as a 16x16x4 MFMA takes them) and "torch" (one
# batched matmul) -- in any class, over four seeds and both data kinds (randn, and the
# post-ReLU-like relu(randn + 0.5)).  Measured largest ratios (always asc / mfma4; torch's
# order depends on the host, and sat within 3 % of asc where this was measured; the
# classes of one form agree to 1 %):
#   F(4x4) C = 64: 1.52   F(4x4) C = 256: 1.83   F(2x2) C = 64: 1.50   F(2x2) C = 256: 1.80
#   F(4x4) grouped, 8 of 64 channels a group: 1.08
# so K = 1.25 x 1.83 = 2.29, above the 2 at which the criterion stops doing its job:
# with both MFMA operands rounded to 20 mantissa bits the restatement's RMS is 2.1-2.2
# x its own full-precision RMS in the same order at C = 256 (3.7-3.9 x at C = 64), inside
# K.  (The 5e-5 max|y| criterion of the existing tests accepts those 20-bit operands in
# every form: largest error 1e-4 against a tolerance of 2.4e-4.)  The order of the sum
# alone moves the RMS by more than the defect the criterion was to catch, so no
# per-position tolerance is asserted on the device; the exact lattice tests carry the
# weight.  tests/test_conv_exact_cpu.py recomputes the figures behind this decision.
PRECISION_SHAPE = (2, 32, 64, 64)  # N, H, W, Cout
PRECISION_FORMS = (("w4", 64, 1), ("w4", 256, 1), ("w2", 64, 1), ("w2", 256, 1), ("w4g", 64, 8))
PRECISION_DATA = ("randn", "relu")
PRECISION_SEEDS = (0, 1, 2, 3)
ORDERS = ("asc", "mfma4", "torch")
ORDER_RATIO = 1.83
K_PRECISION = 1.25 * ORDER_RATIO  # 2.29 > 2: not shipped


def precision_inputs(form, data, seed):
    kind, C, groups = form
    N, H, W, Co = PRECISION_SHAPE
    g = torch.Generator(device="cpu").manual_seed(1000 * seed + C + groups)
    x = torch.randn((N, C, H, W), generator=g)
    if data == "relu":
        x = F.relu(x + 0.5)
    cpg = C // groups
    w = torch.randn((Co, cpg, 3, 3), generator=g) / (9 * C) ** .5
    return x, w


def class_rms(y, ref, m):
    """RMS of y - ref per output position class: [m][m] float64."""
    e = (y.double() - ref) ** 2
    return torch.stack([torch.stack([e[:, :, a::m, b::m].mean().sqrt() for b in range(m)])
                        for a in range(m)])


def precision_restated(form, data, seed, order="torch", bits=None):
    """(per-class RMS of the restatement, float64 reference, m)."""
    kind, C, groups = form
    m = 2 if kind == "w2" else 4
    x, w = precision_inputs(form, data, seed)
    ref = conv64(x, w, groups=groups)
    y = wino_restate(x, w, m=m, order=order, groups=groups, bits=bits)
    return class_rms(y, ref, m), ref, m
