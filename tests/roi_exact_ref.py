"""RoIAlign on dyadic RoI lattices: a float64 reference and the inputs on which every float32
evaluation order of RoIAlign -- the reference's per-sample order, the product kernel's
separable order, atomics in any order -- must EQUAL it bit for bit (DESIGN.md section 2,
item 9).  No device is needed here; tests/test_roi_exact_cpu.py checks the inputs and
tests/test_roi_exact_gpu.py runs the kernels on them.

The lattice, per level and in level pixels: a RoI starts on the 1/4 grid and is P m / 8 wide
and high with an integer m >= 2 (at least one pixel, so the reference's max(w, 1) stays out
of it).  Level scales are powers of two, so the image-space RoI (the level-space one divided
by the scale) and roi * scale are exact.  The bin is m / 8 wide, every sample of a grid of
1, 2 or 4 sits on a dyadic grid, every bilinear weight is dyadic, and with integer features
every term, every partial sum in any order and the result are integers times one unit q --
as long as no sum reaches 2^24 q, which `condition` evaluates in float64."""
import collections
import functools
import math

import numpy as np

SIZES = ((50, 84), (25, 42), (13, 21), (7, 11))   # a 200 x 336 blob at strides 4 .. 32
SCALES = (1. / 4, 1. / 8, 1. / 16, 1. / 32)
B = 2
LIMIT = float(1 << 24)

Case = collections.namedtuple("Case", "name C P sr levels fmax n_random seed reaches")
# levels: indices into SIZES / SCALES of the case's pyramid (one entry: a single-level case)
CASES = (
    Case("p7-c256-simple-launch", 256, 7, 2, (0, 1, 2, 3), 128, 40, 1,
         "the SIMPLE launch of the product kernel (C <= 256, one chunk, every lane active)"),
    Case("p14-c256-mask-head", 256, 14, 2, (0, 1, 2, 3), 128, 56, 2,
         "the mask head's launch: 14 rows on 8 waves, a second pass of the wave loop"),
    Case("p7-c64-lanes-past-c", 64, 7, 2, (0, 1, 2, 3), 128, 40, 3,
         "lanes 16 .. 63 past C inactive"),
    Case("p14-c520-three-chunks", 520, 14, 2, (0, 1, 2, 3), 128, 56, 4,
         "three 256-channel chunks, the last 8 channels wide: the general form"),
    Case("p7-c4-minimum", 4, 7, 2, (0, 1, 2, 3), 128, 40, 5,
         "the smallest channel count: one active lane"),
    Case("p5-c64-other-size", 64, 5, 2, (0, 1, 2, 3), 128, 20, 6,
         "a pooled size other than 7 and 14"),
    Case("p7-c64-sr0-pyramid", 64, 7, 0, (0, 1, 2, 3), 8, 40, 7,
         "the adaptive grid (1, 2 or 4 samples a side) over the pyramid: the row kernel"),
    Case("p7-c24-one-level", 24, 7, 2, (1,), 128, 40, 8,
         "one level: layout='nchw' and the NCHW drop-in"),
    Case("p7-c24-sr0-one-level", 24, 7, 0, (1,), 8, 40, 9,
         "one level, adaptive grid: the NCHW drop-in at sr = 0"),
    Case("p5-c24-sr0-generic", 24, 5, 0, (2,), 8, 40, 10,
         "PH == PW not in {7, 14} and sr != 2: the generic kernel"),
    Case("p6-c24-sr4-generic", 24, 6, 4, (2,), 8, 40, 11,
         "the generic kernel with a fixed grid of 4"),
)
BY_NAME = {c.name: c for c in CASES}
PYRAMID = tuple(c for c in CASES if len(c.levels) == 4)
SEPARABLE = tuple(c for c in PYRAMID if c.sr == 2)
ONE_LEVEL = tuple(c for c in CASES if len(c.levels) == 1)

# backward: many RoIs on the same pixels of one small map
BwdCase = collections.namedtuple("BwdCase", "name C P sr level gmax n_random seed")
BWD_CASES = (
    BwdCase("bwd-p7-sr2", 8, 7, 2, 2, 8, 60, 21),
    BwdCase("bwd-p5-sr0", 8, 5, 0, 3, 4, 60, 22),
)
BWD_BY_NAME = {c.name: c for c in BWD_CASES}


# ------------------------------------------------------------------ the lattice
def grid_of(m, sr):
    """Samples a side of a bin m / 8 wide."""
    return sr if sr > 0 else int(math.ceil(m / 8.))


def _roi(b, x0, y0, mx, my, P):
    """Level-space RoI [b, x1, y1, x2, y2]: start on the 1/4 grid, P m / 8 wide and high."""
    assert (4 * x0) == int(4 * x0) and (4 * y0) == int(4 * y0) and mx >= 2 and my >= 2
    assert P * mx >= 8 and P * my >= 8
    return [b, x0, y0, x0 + P * mx / 8., y0 + P * my / 8.]


def _edge_m(sr, k):
    """The k-th bin width m whose first sample lies a multiple of 1/4 after the start
    (m / (16 grid) in 1/4 Z), so that a start on the 1/4 grid puts a sample on an integer."""
    ms = (8, 16, 24) if sr == 2 else (16, 32, 48) if sr == 4 else (4, 8, 16, 32)
    return ms[k % len(ms)]


def _planted(H, W, P, sr, k):
    """The planted RoIs of one level, variant k (level pixels).  `first` is the distance
    from the start to the first sample, `last` to the last one."""
    b = k % B
    m = _edge_m(sr, k)
    g = grid_of(m, sr)
    first = m / (16. * g)
    last = P * m / 8. - first
    step = m / (8. * g)            # between two samples
    wide = 40 if sr == 2 else 32   # bins of 5 and 4 pixels: no column is used twice
    whole = lambda n: max(2, int(math.ceil(8. * n / P)))
    if sr == 0:                    # a grid of 1, 2 or 4 only: at most 4 P pixels of the map
        whole = lambda n: min(v for v in list(range(2, 17)) + list(range(25, 33))
                              if v >= min(8. * n / P, 32))
    r = [
        _roi(b, -1 - first, -1 - first, m, m, P),            # first sample at -1, x and y
        _roi(1 - b, W - last, H - last, m, m, P),            # last sample at W and at H
        _roi(b, -first, -first, m, m, P),                    # first sample at 0
        _roi(1 - b, -first - step, -first - step, m, m, P),  # second sample at 0
        _roi(b, W - 1 - last, H - 1 - last, m, m, P),        # last sample at W - 1 / H - 1
        _roi(1 - b, W - 1 - first - step, H - 1 - first - step, m, m, P),  # second at W-1/H-1
        _roi(b, 2 - first, 1 - first, m, m, P),              # samples on interior integers
        _roi(1 - b, 1.25, 0.5, 3, 2, P),     # y samples of a bin share a pixel row; narrow bins
        _roi(b, W - 3.5, H - 2.25, 2, 3, P),                 # the same at the far corner
        _roi(1 - b, -3.25, -2.5, wide, wide, P),             # bins wider than two pixels
        _roi(b, W + 2, H + 1.5, m, 5, P),                    # wholly off the map (past it)
        _roi(1 - b, -40.25, 3, 7, 9, P),                     # wholly off the map (before it)
        _roi(b, 0, 0, whole(W), whole(H), P),                # the whole map
        _roi(1 - b, -2.75, 3.25, 11, 5, P),                  # crossing the left border
        _roi(b, W - 3.25, 1.5, 12, 4, P),                    # the right border
        _roi(1 - b, 4.5, -1.75, 6, 10, P),                   # the top border
        _roi(b, 2.25, H - 2.5, 5, 13, P),                    # the bottom border
    ]
    if sr == 0:  # a grid of 3 would make count no power of two
        r = [q for q in r if all(grid_of(round((q[3 + a] - q[1 + a]) * 8 / P), 0) in (1, 2, 4)
                                 for a in (0, 1))]
    return r


def _tiles(H, W, P, sr):
    """RoIs with bins of 4 pixels and a sample every 2 pixels (sr = 2) or every pixel, off the
    integers, that tile the map: between them every pixel carries a non-zero weight."""
    # a map smaller than such a tile takes one tile of its own size (denser samples)
    mx, my = (min(32, int(math.ceil(8 * (n + .25) / P))) for n in (W, H))
    if sr == 0:
        mx, my = (m if grid_of(m, 0) in (1, 2, 4) else 25 for m in (mx, my))
    out = []
    for b in range(B):
        for ty in range(int(math.ceil((H + .25) / (P * my / 8.)))):
            for tx in range(int(math.ceil((W + .25) / (P * mx / 8.)))):
                out.append(_roi(b, -.25 + tx * P * mx / 8., -.25 + ty * P * my / 8., mx, my, P))
    return out


def _random(rng, H, W, P, sr, n):
    # up to 5-pixel bins, and no wider than the map: most bins then lie on it
    msx, msy = (np.array([v for v in range(2, max(4, min(41, int(8 * N / P))))
                          if sr != 0 or grid_of(v, 0) in (1, 2, 4)]) for N in (W, H))
    out = []
    for _ in range(n):
        mx, my = rng.choice(msx), rng.choice(msy)
        w, h = P * mx / 8., P * my / 8.
        x0 = rng.integers(-8, max(4 * (W - 2), -7)) / 4. - (w / 2 if rng.random() < .3 else 0)
        y0 = rng.integers(-8, max(4 * (H - 2), -7)) / 4. - (h / 2 if rng.random() < .3 else 0)
        out.append(_roi(int(rng.integers(0, B)), math.floor(4 * x0) / 4., math.floor(4 * y0) / 4.,
                        int(mx), int(my), P))
    return out


def _lattice_rois(rng, levels, P, sr, n_random, variants, tiles=True):
    """(rois in image pixels float32 [R, 5], level index per RoI int32), shuffled."""
    rows, lv = [], []
    for i, l in enumerate(levels):
        H, W = SIZES[l]
        r = []
        for k in variants:
            r += _planted(H, W, P, sr, k + l)
        if tiles:
            r += _tiles(H, W, P, sr)
        r += _random(rng, H, W, P, sr, n_random // len(levels))
        r = np.array(r, np.float64)
        r[:, 1:] /= SCALES[l]                      # exact: the scale is a power of two
        rows.append(r)
        lv += [i] * len(r)
    rois = np.concatenate(rows)
    assert np.array_equal(rois.astype(np.float32).astype(np.float64), rois)
    perm = rng.permutation(len(rois))
    return rois[perm].astype(np.float32), np.array(lv, np.int32)[perm]


Inputs = collections.namedtuple("Inputs", "feats rois levels scales sizes P sr C")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's (features per level [B, C, H, W] float32 integers, rois, levels, ...).
    Cached: treat as read-only."""
    c = BY_NAME[name]
    rng = np.random.default_rng(900 + c.seed)
    feats = [rng.integers(-c.fmax, c.fmax + 1, (B, c.C) + SIZES[l]).astype(np.float32)
             for l in c.levels]
    variants = (0,) if len(c.levels) > 1 else (0, 1, 2, 3)
    rois, lv = _lattice_rois(rng, c.levels, c.P, c.sr, c.n_random, variants)
    for f in feats:
        f.setflags(write=False)
    rois.setflags(write=False)
    lv.setflags(write=False)
    return Inputs(tuple(feats), rois, lv, tuple(SCALES[l] for l in c.levels),
                  tuple(SIZES[l] for l in c.levels), c.P, c.sr, c.C)


def cases():
    """name -> (features per level, rois, levels, P, sr) of every forward case."""
    out = collections.OrderedDict()
    for c in CASES:
        i = inputs(c.name)
        out[c.name] = (i.feats, i.rois, i.levels, i.P, i.sr)
    return out


BwdInputs = collections.namedtuple("BwdInputs", "top rois scale shape P sr")


@functools.lru_cache(maxsize=None)
def bwd_inputs(name):
    """Integer top_grad [R, C, P, P] and lattice RoIs piled on one small map."""
    c = BWD_BY_NAME[name]
    rng = np.random.default_rng(900 + c.seed)
    rois, _ = _lattice_rois(rng, (c.level,), c.P, c.sr, c.n_random, (0, 1, 2, 3))
    top = rng.integers(-c.gmax, c.gmax + 1, (len(rois), c.C, c.P, c.P)).astype(np.float32)
    top.setflags(write=False)
    return BwdInputs(top, rois, SCALES[c.level], (B, c.C) + SIZES[c.level], c.P, c.sr)


# ------------------------------------------------------------------ float64 reference
Axis = collections.namedtuple("Axis", "pos valid lo hi l h grid")


def axis(start, end, P, sr, N):
    """One axis of a RoI's sample grid, reference semantics (roi_align_kernel.cu:16-63,
    :85-116) in float64: raw positions, in-range flags (inclusive at -1 and N), the two
    taps and their weights after the <= 0 and >= N - 1 clamps."""
    size = max(end - start, 1.0)
    bin_ = size / P
    g = sr if sr > 0 else int(math.ceil(size / P))
    p = np.repeat(np.arange(P), g)
    i = np.tile(np.arange(g), P)
    pos = start + p * bin_ + (i + .5) * bin_ / g
    valid = ~((pos < -1.0) | (pos > N))
    x = np.where(pos <= 0, 0.0, pos)
    lo = np.floor(x).astype(np.int64)
    clamp = lo >= N - 1
    lo = np.where(clamp, N - 1, lo)
    hi = np.where(clamp, N - 1, lo + 1)
    x = np.where(clamp, lo.astype(np.float64), x)
    lo = np.where(valid, lo, 0)         # a dropped sample reads nothing; keep the index legal
    hi = np.where(valid, hi, 0)
    l = x - lo
    l = np.where(valid, l, 0.0)
    return Axis(pos, valid, lo, hi, l, np.where(valid, 1.0 - l, 0.0), g)


def roi_axes(roi, scale, P, sr, H, W):
    r = np.asarray(roi, np.float64)
    ax = axis(r[1] * scale, r[3] * scale, P, sr, W)
    ay = axis(r[2] * scale, r[4] * scale, P, sr, H)
    return ay, ax


def roi_align(feats, rois, levels, scales, P, sr, absolute=False):
    """Float64 RoIAlign forward over a pyramid -> [R, C, P, P].  feats[l]: [B, C, H, W];
    levels[r] indexes feats.  absolute=True pools |F| without the division by count (the
    left side of the exactness condition)."""
    f64 = [np.abs(f.astype(np.float64)) if absolute else f.astype(np.float64) for f in feats]
    R, C = len(rois), feats[0].shape[1]
    out = np.zeros((R, C, P, P))
    for n in range(R):
        l = int(levels[n])
        Bn, _, H, W = f64[l].shape
        ay, ax = roi_axes(rois[n], scales[l], P, sr, H, W)
        F = f64[l][int(rois[n][0])]
        yl, yh, xl, xh = ay.lo[:, None], ay.hi[:, None], ax.lo[None, :], ax.hi[None, :]
        hy, ly, hx, lx = ay.h[:, None], ay.l[:, None], ax.h[None, :], ax.l[None, :]
        s = (hy * hx) * F[:, yl, xl] + (hy * lx) * F[:, yl, xh] \
            + (ly * hx) * F[:, yh, xl] + (ly * lx) * F[:, yh, xh]
        s = s.reshape(C, P, ay.grid, P, ax.grid).sum(axis=(2, 4))
        out[n] = s if absolute else s / (ay.grid * ax.grid)
    return out


def roi_align_backward(top, rois, scale, shape, sr, absolute=False):
    """Float64 RoIAlign backward (roi_align_kernel.cu:195-270) -> bottom_diff [B, C, H, W]."""
    Bn, C, H, W = shape
    R, _, P, _ = top.shape
    out = np.zeros((Bn, H, W, C))
    g64 = np.abs(top.astype(np.float64)) if absolute else top.astype(np.float64)
    for n in range(R):
        ay, ax = roi_axes(rois[n], scale, P, sr, H, W)
        g = np.repeat(np.repeat(g64[n], ay.grid, axis=1), ax.grid, axis=2) / (ay.grid * ax.grid)
        g = g.transpose(1, 2, 0)                       # [ny, nx, C]
        plane = out[int(rois[n][0])]
        yl, yh, xl, xh = ay.lo[:, None], ay.hi[:, None], ax.lo[None, :], ax.hi[None, :]
        hy, ly, hx, lx = ay.h[:, None, None], ay.l[:, None, None], ax.h[None, :, None], \
            ax.l[None, :, None]
        np.add.at(plane, (yl, xl), g * (hy * hx))
        np.add.at(plane, (yl, xh), g * (hy * lx))
        np.add.at(plane, (yh, xl), g * (ly * hx))
        np.add.at(plane, (yh, xh), g * (ly * lx))
    return out.transpose(0, 3, 1, 2).copy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's float64 forward [R, C, P, P].  Cached: treat as read-only."""
    i = inputs(name)
    y = roi_align(i.feats, i.rois, i.levels, i.scales, i.P, i.sr)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def bwd_reference(name):
    i = bwd_inputs(name)
    y = roi_align_backward(i.top, i.rois, i.scale, i.shape, i.sr)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------ the exactness condition
def dyadic_unit(values):
    """The largest power of two of which every value is an integer multiple."""
    v = np.asarray(values, np.float64).ravel()
    v = v[v != 0]
    u = 1.0
    while v.size and not np.array_equal(np.floor(v / u), v / u):
        u /= 2
        assert u > 2.0 ** -40, "not dyadic"
    return u


def lattice_unit(rois, levels, scales, sizes, P, sr, value_unit=1.0):
    """q of a case: over its RoIs the smallest (x weight unit) (y weight unit) (value unit)
    / count, each unit read off the RoI's own weights."""
    q = None
    for n in range(len(rois)):
        l = int(levels[n])
        ay, ax = roi_axes(rois[n], scales[l], P, sr, *sizes[l])
        u = dyadic_unit(np.concatenate([ax.l, ax.h])) * dyadic_unit(np.concatenate([ay.l, ay.h])) \
            * value_unit / (ay.grid * ax.grid)
        q = u if q is None else min(q, u)
    return q


def condition(name):
    """(largest sum of |term| over an output, 2^24 q, q) of a forward case."""
    i = inputs(name)
    q = lattice_unit(i.rois, i.levels, i.scales, i.sizes, i.P, i.sr,
                     dyadic_unit(np.concatenate([f.ravel() for f in i.feats])))
    return float(roi_align(i.feats, i.rois, i.levels, i.scales, i.P, i.sr, True).max()), LIMIT * q, q


def bwd_condition(name):
    """(largest sum over a pixel of w |g| / count, 2^24 q, q) of a backward case."""
    i = bwd_inputs(name)
    R = len(i.rois)
    q = lattice_unit(i.rois, np.zeros(R, np.int32), (i.scale,), (i.shape[2:],), i.P, i.sr,
                     dyadic_unit(i.top))
    return float(roi_align_backward(i.top, i.rois, i.scale, i.shape, i.sr, True).max()), \
        LIMIT * q, q


# ------------------------------------------------------------------ what the inputs reach
def reach(rois, levels, scales, sizes, P, sr):
    """Counts over a case's samples, from the reference's rules alone: samples exactly on
    -1, 0, N - 1 and N per axis, bin rows whose y taps merge (a pixel row named twice among
    the 2 grid taps), x samples that reuse the previous sample's column pair, that slide
    (xl == the previous xh), that load two new columns, and right-edge samples (xl == xh)."""
    c = collections.Counter()
    for n in range(len(rois)):
        l = int(levels[n])
        H, W = sizes[l]
        ay, ax = roi_axes(rois[n], scales[l], P, sr, H, W)
        for tag, a, N in (("x", ax, W), ("y", ay, H)):
            for what, v in (("-1", -1), ("0", 0), ("last", N - 1), ("N", N)):
                c["%s==%s" % (tag, what)] += int((a.pos == v).sum())
            c[tag + " lattice zero weight"] += int(((a.l == 0) & a.valid & (a.pos > 0)
                                                    & (a.pos < N - 1)).sum())
            c[tag + " dropped"] += int((~a.valid).sum())
        for ph in range(P):
            s = slice(ph * ay.grid, (ph + 1) * ay.grid)
            rows = np.concatenate([ay.lo[s][ay.valid[s]], ay.hi[s][ay.valid[s]]])
            if rows.size and len(set(rows.tolist())) < rows.size:
                c["merged tap rows"] += 1
        cl = ch = -1
        for j in range(len(ax.pos)):
            if not ax.valid[j]:
                continue
            xl, xh = int(ax.lo[j]), int(ax.hi[j])
            if xl == cl and xh == ch:
                c["column pair reused"] += 1
            elif xl == ch:
                c["column slid"] += 1
            elif cl >= 0:
                c["columns both new"] += 1
            if xl == xh:
                c["right edge (xl == xh)"] += 1
            cl, ch = xl, xh
    return c


def coverage(rois, levels, scales, sizes, P, sr):
    """Per level a [B, H, W] mask of the pixels some sample reads with a non-zero weight."""
    cov = [np.zeros((B,) + s, bool) for s in sizes]
    for n in range(len(rois)):
        l = int(levels[n])
        ay, ax = roi_axes(rois[n], scales[l], P, sr, *sizes[l])
        ry = np.zeros(sizes[l][0], bool)
        rx = np.zeros(sizes[l][1], bool)
        ry[ay.lo[ay.h != 0]] = True
        ry[ay.hi[ay.l != 0]] = True
        rx[ax.lo[ax.h != 0]] = True
        rx[ax.hi[ax.l != 0]] = True
        cov[l][int(rois[n][0])] |= ry[:, None] & rx[None, :]
    return cov


def fpn_blobs(rois, levels, n_levels=4):
    """The oracle's roi_feature_transform inputs for a given level per RoI (level 0 is the
    finest, fpn2): per-level RoI lists and the restore index."""
    d = {"rois": rois}
    order = np.empty((0,))
    for k in range(n_levels):
        idx = np.where(levels == k)[0]
        d["rois_fpn%d" % (k + 2)] = rois[idx]
        order = np.concatenate([order, idx])
    d["rois_idx_restore_int32"] = np.argsort(order, kind="stable").astype(np.int32)
    return d
