"""Float64 restatement of GroupNorm with the epilogues of vd_group_norm_act, of
the ConvGRU stages (vd_convgru_gates, vd_convgru_update), the a-priori float32
error bounds the tests hold the kernels to, a numpy float32 restatement of the
kernels' own arithmetic (the proof that the bounds admit a correct kernel), and
the cases both test files run.  CPU only; inputs are float32 tensors (exactly
representable in double).

Reference, per (n, g) over the group's C/G x H x W values of V:
  mu = mean(V), var = mean((V - mu)^2), rho = 1 / sqrt(var + float32(eps))
  Y  = (V - mu) * rho * gamma + beta
V is x, or the *float32* sum x + x2 cast to double: that rounded sum is what both
torch and the kernel normalise.

Bound of the normalisation, u = 2^-24, per element:
  b_gn = u * (|mu| rho |gamma| + 8 |V - mu| rho |gamma| + 2 |Y|)
Count: the kernel keeps the statistics in double and rounds them once.
  |mu| rho |gamma|       float(mu) is off by at most u |mu|; that shift reaches
                         the output through rho * gamma.
  8 |V - mu| rho |gamma| relative roundings on the path of (V - mu) * rho * gamma:
                         the subtraction (1), rho = 1 / sqrt(float(var) + eps) with
                         float(var) (<= 1/2: it sits under the square root), the
                         eps add (<= 1/2), sqrt (1) and the divide (1), the two
                         products (2) = 6; the remaining 2 cover the double
                         statistics' own cancellation (ss / n - mean^2) and the
                         second-order terms.
  2 |Y|                  the final add of beta and the store (none if contracted
                         into an FMA).
Epilogues carry the bound forward: relu and tanh are 1-Lipschitz, sigmoid is
1/4-Lipschitz, every float add or product adds u times its result; S and T are
the device's sigmoid and tanhf errors (measured on the device, passed in).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-5
EPILOGUES = ("none", "relu", "sigmoid", "tanh", "res", "res_up", "res_gn")
ACT_RANGE = 8.0  # S and T are measured over [-8, 8]


# --------------------------------------------------------------------------- float64
def _eps64(eps):
    return float(np.float32(eps))


def _v(x, x2):
    """The value the kernels normalise: x, or the float32 sum x + x2, as double."""
    return (x if x2 is None else x + x2).double()


def gn64(x, G, gamma, beta, eps=EPS, x2=None):
    """(Y, b_gn): float64 GroupNorm of V = x (+ x2) and its per-element bound."""
    V = _v(x, x2)
    B, C = V.shape[:2]
    grp = V.reshape(B, G, -1)
    mu = grp.mean(dim=2, keepdim=True)
    var = ((grp - mu) ** 2).mean(dim=2, keepdim=True)
    rho = 1.0 / torch.sqrt(var + _eps64(eps))
    ga = gamma.double().view(1, C, 1, 1)
    cen = ((grp - mu) * rho).reshape(V.shape)          # (V - mu) * rho
    Y = cen * ga + beta.double().view(1, C, 1, 1)
    shift = (mu.abs() * rho).expand_as(grp).reshape(V.shape)  # |mu| rho
    bound = U * ((shift + 8.0 * cen.abs()) * ga.abs() + 2.0 * Y.abs())
    return Y, bound


def up2(r):
    return F.interpolate(r, scale_factor=2, mode="nearest")


def epilogue64(kind, d, G, S, T, eps=EPS):
    """(reference, bound, pre-activation or None) of one vd_group_norm_act epilogue
    on the inputs d (see gn_inputs).  The sigmoid and tanh epilogues normalise
    x + x2, the rest x alone."""
    if kind in ("sigmoid", "tanh"):
        Y, b = gn64(d["x"], G, d["gamma"], d["beta"], eps, d["x2"])
        if kind == "sigmoid":
            return torch.sigmoid(Y), b / 4.0 + S, Y
        return torch.tanh(Y), b + T, Y
    Y, b = gn64(d["x"], G, d["gamma"], d["beta"], eps)
    if kind == "none":
        return Y, b, None
    if kind == "relu":
        return torch.relu(Y), b, None
    if kind == "res":            # relu(GN(x) + r)
        s = Y + d["res"].double()
        return torch.relu(s), b + U * s.abs(), None
    if kind == "res_up":         # GN(x) + nearest-2x(r)
        s = Y + up2(d["res_up"].double())
        return s, b + U * s.abs(), None
    if kind == "res_gn":         # relu(GN(x) + GN_r(r))
        Yr, br = gn64(d["res_g"], G, d["gamma_r"], d["beta_r"], eps)
        s = Y + Yr
        return torch.relu(s), b + br + U * s.abs(), None
    raise ValueError(kind)


def gates64(d, G, S, eps=EPS, state=True):
    """z = sigmoid(GN_z(zx + zh)), hr = h * sigmoid(GN_r(rx + rh)) with their bounds
    |z - Z| <= b/4 + S, |hr - HR| <= |h| (b/4 + S) + u |HR|.  Zero state: z from zx
    alone, no hr."""
    Pz, bz = gn64(d["zx"], G, d["gamma_z"], d["beta_z"], eps, d["zh"] if state else None)
    out = {"z": (torch.sigmoid(Pz), bz / 4.0 + S), "pre": [Pz]}
    if state:
        Pr, br = gn64(d["rx"], G, d["gamma_r"], d["beta_r"], eps, d["rh"])
        h = d["h"].double()
        HR = h * torch.sigmoid(Pr)
        out["hr"] = (HR, h.abs() * (br / 4.0 + S) + U * HR.abs())
        out["pre"].append(Pr)
    return out


def mean2x2(f):
    f = f.double()
    return (f[..., 0::2, 0::2] + f[..., 0::2, 1::2] + f[..., 1::2, 0::2] + f[..., 1::2, 1::2]) / 4.0


def update64(d, G, T, eps=EPS, state=True, finer=True):
    """hn = (1 - z) h + z tanh(GN_h(hx + hh)) on an arbitrary z in (0, 1) (zero
    state: z tanh(GN_h(hx))); out = hn / 2 + mean2x2(finer) / 2 when finer.
      e_hn = z (b + T) + 3u (|(1 - z) h| + |z tanh P|)
      |out - OUT| <= e_hn / 2 + 3u (|a| + |b| + |c| + |d|) / 8 + u |OUT|
    (the halvings are exact; the 2x2 mean is three float additions deep)."""
    P, b = gn64(d["hx"], G, d["gamma_h"], d["beta_h"], eps, d["hh"] if state else None)
    z = d["z"].double()
    h = d["h"].double() if state else torch.zeros_like(z)
    t = torch.tanh(P)
    HN = (1.0 - z) * h + z * t
    e = z * (b + T) + 3.0 * U * (((1.0 - z) * h).abs() + (z * t).abs())
    if not finer:
        return HN, e, P
    OUT = HN / 2.0 + mean2x2(d["finer"]) / 2.0
    taps = mean2x2(d["finer"].abs()) * 4.0
    return OUT, e / 2.0 + 3.0 * U * taps / 8.0 + U * OUT.abs(), P


# --------------------------------------------------------------------------- float32 restatement
f32 = np.float32


def stats_double(v, G):
    """The kernels' statistics: double sum and sum of squares, var = ss/n - mean^2
    clamped at 0, rounded to float once."""
    B = v.shape[0]
    g = v.reshape(B, G, -1).astype(np.float64)
    n = g.shape[2]
    mean = g.sum(axis=2) / n
    var = np.maximum((g * g).sum(axis=2) / n - mean * mean, 0.0)
    return mean.astype(f32), var.astype(f32)


def stats_float32(v, G):
    """Deliberately wrong: the sums and the variance kept in float32."""
    B = v.shape[0]
    g = v.reshape(B, G, -1)
    n = f32(g.shape[2])
    mean = g.sum(axis=2, dtype=f32) / n
    var = np.maximum((g * g).sum(axis=2, dtype=f32) / n - mean * mean, f32(0))
    return mean, var


def stats_count_hw(v, G):
    """Deliberately wrong: count taken as H*W instead of (C/G)*H*W."""
    B = v.shape[0]
    g = v.reshape(B, G, -1).astype(np.float64)
    n = v.shape[2] * v.shape[3]
    mean = g.sum(axis=2) / n
    var = np.maximum((g * g).sum(axis=2) / n - mean * mean, 0.0)
    return mean.astype(f32), var.astype(f32)


def _np(t):
    return None if t is None else t.numpy()


def gn32(x, G, gamma, beta, eps=EPS, x2=None, stats=stats_double):
    """float32 restatement of gn_consts + gn_norm: ((v - m) * r) * gamma + beta."""
    v = _np(x) if x2 is None else _np(x) + _np(x2)
    B, C = v.shape[:2]
    mean, var = stats(v, G)
    rstd = f32(1) / np.sqrt(var + f32(eps))
    cg = C // G
    m = np.repeat(mean, cg, axis=1).reshape(B, C, 1, 1)
    r = np.repeat(rstd, cg, axis=1).reshape(B, C, 1, 1)
    y = ((v - m) * r) * _np(gamma).reshape(1, C, 1, 1) + _np(beta).reshape(1, C, 1, 1)
    assert y.dtype == f32
    return y


def sigmoid32(v):
    """1 / (1 + exp(-v)) in float32 with a correctly rounded exp."""
    e = np.exp(-v.astype(np.float64)).astype(f32)
    return f32(1) / (f32(1) + e)


def tanh32(v):
    return np.tanh(v.astype(np.float64)).astype(f32)


def epilogue32(kind, d, G, eps=EPS, stats=stats_double):
    if kind in ("sigmoid", "tanh"):
        y = gn32(d["x"], G, d["gamma"], d["beta"], eps, d["x2"], stats)
        return sigmoid32(y) if kind == "sigmoid" else tanh32(y)
    y = gn32(d["x"], G, d["gamma"], d["beta"], eps, None, stats)
    if kind == "none":
        return y
    if kind == "relu":
        return np.maximum(y, f32(0))
    if kind == "res":
        return np.maximum(y + _np(d["res"]), f32(0))
    if kind == "res_up":
        return y + _np(up2(d["res_up"]))
    if kind == "res_gn":
        return np.maximum(y + gn32(d["res_g"], G, d["gamma_r"], d["beta_r"], eps, None, stats),
                          f32(0))
    raise ValueError(kind)


def gates32(d, G, eps=EPS, state=True):
    z = sigmoid32(gn32(d["zx"], G, d["gamma_z"], d["beta_z"], eps, d["zh"] if state else None))
    if not state:
        return z, None
    r = sigmoid32(gn32(d["rx"], G, d["gamma_r"], d["beta_r"], eps, d["rh"]))
    return z, _np(d["h"]) * r


def update32(d, G, eps=EPS, state=True, finer=True):
    t = tanh32(gn32(d["hx"], G, d["gamma_h"], d["beta_h"], eps, d["hh"] if state else None))
    z = _np(d["z"])
    hn = (f32(1) - z) * _np(d["h"]) + z * t if state else z * t
    if not finer:
        return hn
    f = _np(d["finer"])
    h_ = f32(0.5)
    down = h_ * (h_ * f[..., 0::2, 0::2] + h_ * f[..., 0::2, 1::2]) + \
        h_ * (h_ * f[..., 1::2, 0::2] + h_ * f[..., 1::2, 1::2])
    out = hn / f32(2) + down / f32(2)
    assert out.dtype == f32
    return out


# --------------------------------------------------------------------------- cases
# name: (B, C, H, W, G, scale, shift, layouts, epilogues) -- data = scale * randn + shift.
# What each is the smallest instance of:
_ALL, _BOTH, _NHWC, _NCHW = EPILOGUES, ("nchw", "nhwc"), ("nhwc",), ("nchw",)
GN_CASES = {
    # RoI head: 8 channels per group (the cg % 4 == 0 fold), H*W = 49 below one block's
    # pixel share, odd map (no nearest-2x residual: the C layer refuses it)
    "roi7": (2, 256, 7, 7, 32, 1.0, 0.0, _BOTH, tuple(e for e in _ALL if e != "res_up")),
    # mask-head geometry, several images on grid.y
    "mask14": (5, 256, 14, 14, 32, 1.0, 0.0, _BOTH, _ALL),
    # res5: C/4 = 512, two passes of the q0 loop, 32 KiB LDS table, 8 pixels per apply block
    "res5": (2, 2048, 4, 6, 32, 1.0, 0.5, _NHWC, _ALL),
    # C/4 = 256 exactly, the boundary of that loop
    "c1024": (1, 1024, 6, 6, 32, 1.0, 0.0, _NHWC, _ALL),
    # exactly one quad per group (cg = 4)
    "quad": (2, 128, 12, 20, 32, 1.0, 0.0, _BOTH, _ALL),
    # stem: quads straddle groups (cg = 2); 1564 pixels, no multiple of the 512-pixel
    # statistics share nor of the apply share
    "stem": (1, 64, 34, 46, 32, 3.0, 1.0, _BOTH, _ALL),
    # cg = 3, C/4 = 24 does not divide 256 (idle threads); not a model shape
    "cg3": (1, 96, 10, 12, 32, 1.0, 0.0, _BOTH, _ALL),
    # P6 of a 512 x 896 blob; nearest-2x residual from 4 x 7
    "p6": (3, 256, 8, 14, 32, 1.0, 0.0, _BOTH, _ALL),
    # mean = 4000 sigma: fails if the statistics lose double precision
    "highmean": (2, 128, 12, 20, 32, 0.05, 200.0, _BOTH, _ALL),
    # var << eps: the rstd path; the mean's rounding reaches 0.99 of the bound
    "lowvar": (2, 128, 12, 20, 32, 1e-3, 1.0, _BOTH, _ALL),
    # the ends of the C layer's range of G; red[2][64] full
    "g64": (2, 64, 6, 8, 64, 1.0, 0.0, _BOTH, _ALL),
    "g1": (2, 64, 6, 8, 1, 1.0, 0.0, _BOTH, _ALL),
    # 17.3 M elements > 65536 x 256: the grid-stride loop of the NCHW apply kernel,
    # 67 chunks per group in the NCHW statistics
    "big": (1, 64, 520, 520, 32, 1.0, 0.0, _NCHW, ("none", "relu")),
}
# The input of test_vos_gpu.py::test_group_norm_act_vs_torch restated with a CPU
# generator (same shape and distributions: x = 3 randn + 1, gamma, beta ~ randn);
# only the CPU file runs it, for the never-weaker-than-2e-5 check.
LEGACY_GN = (3, 64, 10, 14, 32, 3.0, 1.0, _BOTH, _ALL)
LEGACY_GN_TOL, LEGACY_GRU_TOL = 2e-5, 1e-5

# (B, C, H, W), G = 32; finer is 2H x 2W
GRU_CASES = {
    "cell": (2, 256, 8, 14),     # the model's cell at the coarsest level
    "odd": (1, 256, 3, 5),       # odd, smaller than any block share
    "c64": (2, 64, 12, 18),      # 2 channels per group; the existing test's shape
}
GRU_G = 32


def _seed(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name))


def _affine(gen, C, legacy=False):
    """gamma, beta.  Uniform in [-1.25, 1.25] and [-1, 1]: with |normalised| < 5.5
    the pre-activations stay inside [-8, 8], the range S and T are measured on."""
    if legacy:
        return torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    return (torch.rand(C, generator=gen) * 2.5 - 1.25, torch.rand(C, generator=gen) * 2 - 1)


def gn_inputs(name):
    """Seeded CPU inputs of a GroupNorm case: x, x2 (the same sigma as x, so that a
    high-mean case stays one), a plain residual, a half-size one where both sides
    are even, and a residual with statistics like x's for the GroupNorm'd one."""
    legacy = name == "legacy"
    B, C, H, W, G, scale, shift, _, epis = LEGACY_GN if legacy else GN_CASES[name]
    gen = torch.Generator().manual_seed(11 if legacy else _seed(name))
    d = {"x": torch.randn((B, C, H, W), generator=gen) * scale + shift}
    d["gamma"], d["beta"] = _affine(gen, C, legacy)
    if "sigmoid" in epis or "tanh" in epis:
        d["x2"] = torch.randn((B, C, H, W), generator=gen) * scale
    if "res" in epis:
        d["res"] = torch.randn((B, C, H, W), generator=gen)
    if "res_up" in epis:
        d["res_up"] = torch.randn((B, C, H // 2, W // 2), generator=gen)
    if "res_gn" in epis:
        d["res_g"] = torch.randn((B, C, H, W), generator=gen) * (2 * scale) + shift
        d["gamma_r"], d["beta_r"] = _affine(gen, C, legacy)
    return d


def gru_inputs(name):
    """Seeded CPU inputs of a ConvGRU case: the six convolution outputs, the state,
    an arbitrary z in (0, 1) for the update stage, and the finer level."""
    B, C, H, W = GRU_CASES[name]
    gen = torch.Generator().manual_seed(_seed("gru_" + name))
    d = {k: torch.randn((B, C, H, W), generator=gen) for k in
         ("zx", "zh", "rx", "rh", "hx", "hh", "h")}
    d["z"] = torch.rand((B, C, H, W), generator=gen) * 0.998 + 0.001
    d["finer"] = torch.randn((B, C, 2 * H, 2 * W), generator=gen)
    for k in "zrh":
        d["gamma_" + k], d["beta_" + k] = _affine(gen, C)
    return d
