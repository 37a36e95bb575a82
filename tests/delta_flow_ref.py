"""Float64 restatement of the delta-flow head (MODEL.USE_DELTA_FLOW) and the
a-priori float32 error bounds the tests hold the kernels to.

  feat_i    = tanh(conv3x3(P_i, w_i))                     i = 0..4 on [P6..P2]
  d_i       = feat_i - previous feat_i
  data_flow = sum_i interpolate(d_i, 1/s_i, bilinear, align_corners=False) / s_i
  level_j   = s_j^3 * (k_j x k_j block sums of data_flow)  (a strided block conv)

All in torch float64 on the CPU; inputs are float32 tensors (exactly representable).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24                      # float32 unit roundoff
STRIDES = (64, 32, 16, 8, 4)        # [P6 .. P2]
SCALES = tuple(1.0 / k for k in STRIDES)
# block-sum tree depth of vd_delta_flow_to_levels: 4 additions inside a thread's
# 4 x 4 block (pairwise), two more per 2 x 2 step to the next coarser level
TREE_DEPTH = {4: 4, 8: 6, 16: 8, 32: 10, 64: 12}
PIXEL_OPS = 8                       # see pixel_bound


def gamma(n):
    return n * U / (1.0 - n * U)


def pre(x, w):
    """The conv before tanh, and sum |w * x| per output element."""
    x, w = x.double(), w.double()
    return F.conv2d(x, w, padding=1), F.conv2d(x.abs(), w.abs(), padding=1)


def feature_bound(abs_sum, C, t):
    """|float32 feature - tanh64(pre64)| <= gamma_n * sum|w x| + t, n = 9C: the
    bound of an n-term float32 dot product in any summation order (with or without
    fused multiply-adds), tanh' <= 1, and t the device tanhf's own error."""
    return gamma(9 * C) * abs_sum + t


def upsample_sum(deltas):
    """data_flow from the five deltas [P6 .. P2] (float64)."""
    out = None
    for d, s in zip(deltas, SCALES):
        up = F.interpolate(d.double(), scale_factor=1.0 / s, mode="bilinear",
                           align_corners=False) / s
        out = up if out is None else out + up
    return out


def block_sum(blob, k):
    """k x k block sums as the strided block conv with unit diagonal weight."""
    w = torch.zeros((2, 2, k, k), dtype=blob.dtype)
    w[0, 0] = 1
    w[1, 1] = 1
    return F.conv2d(blob, w, stride=k)


def levels(blob):
    """[level flows of strides 64 .. 4] of a float64 data_flow."""
    return [block_sum(blob, k) * (1.0 / k) ** 3 for k in STRIDES]


def pixel_bound(deltas):
    """|float32 data_flow - float64| per blob pixel for vd_delta_flow_to_levels.

    A = sum_i (1/s_i) * bilerp_i(|d_i|).  The kernel evaluates, per level,
    hy0 * (hx0 * a + hx1 * b) + hy1 * (hx0 * c + hx1 * d) with exact weights: a
    source value passes through one product, one sum, one product and one sum = 4
    roundings; the product with 1/s is exact (a power of two); the five terms are
    then added coarsest first into an accumulator that starts at zero (the first
    addition is exact), so a term sees at most 4 further roundings.  (1+u)^8 - 1
    <= gamma_8: c = PIXEL_OPS = 8."""
    return gamma(PIXEL_OPS) * upsample_sum([d.abs() for d in deltas])


def level_bounds(deltas):
    """Per element of each level flow: the pixel bound carried through the block
    sum tree, gamma_(8 + depth_k) * s^3 * blocksum(A) (|data_flow| <= A)."""
    A = upsample_sum([d.abs() for d in deltas])
    return [gamma(PIXEL_OPS + TREE_DEPTH[k]) * block_sum(A, k) * (1.0 / k) ** 3 for k in STRIDES]


def propagate(errs):
    """Per-element error bounds e_i of the five deltas -> the bounds they induce on
    the five level flows (everything downstream is linear with non-negative
    weights)."""
    return levels(upsample_sum(errs))
