"""The inputs of tests/test_roi_exact_gpu.py, checked without a device (tests/roi_exact_ref.py):
every case meets its exactness condition and reaches the branches it is there for; the
oracle's C restatement and a float32 restatement of the product kernel's separable order
both EQUAL the float64 reference on them; and each of a list of planted defects, applied
to a float32 restatement, breaks that equality on a named case.  On real-valued data the two
float32 orders differ, which is why the lattice is needed."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import roi_exact_ref as R

f32 = np.float32
NAMES = [c.name for c in R.CASES]
BWD_NAMES = [c.name for c in R.BWD_CASES]


# ------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("name", NAMES)
def test_forward_condition(name):
    """max over outputs of sum_samples sum_taps w |F| < 2^24 q, q read off the lattice."""
    worst, limit, q = R.condition(name)
    print("%s: q = 2^%d, largest sum %.6g, limit %.6g" % (name, np.log2(q), worst, limit))
    assert worst < limit
    ref = R.reference(name)
    assert np.array_equal(np.round(ref / q), ref / q), "an output off the lattice"
    assert np.array_equal(ref.astype(f32).astype(np.float64), ref)


@pytest.mark.parametrize("name", BWD_NAMES)
def test_backward_condition(name):
    """max over pixels of the sum over all RoIs, bins and samples of w |g| / count < 2^24 q."""
    worst, limit, q = R.bwd_condition(name)
    print("%s: q = 2^%d, largest sum %.6g, limit %.6g" % (name, np.log2(q), worst, limit))
    assert worst < limit
    ref = R.bwd_reference(name)
    assert np.array_equal(np.round(ref / q), ref / q)
    i = R.bwd_inputs(name)
    # many RoIs on the same pixels: the busiest pixel collects from dozens of them
    hits = np.zeros(i.shape[2:])
    for r in i.rois:
        ay, ax = R.roi_axes(r, i.scale, i.P, i.sr, *i.shape[2:])
        m = np.zeros(i.shape[2:], bool)
        m[np.ix_(np.unique(ay.lo[ay.valid]), np.unique(ax.lo[ax.valid]))] = True
        hits += m
    assert hits.max() >= 24, hits.max()


def test_lattice_keeps_every_roi_at_least_one_pixel():
    """Below one level pixel the reference's max(w, 1) makes the bin 1 / P: not dyadic."""
    for name in NAMES:
        i = R.inputs(name)
        sc = np.array([i.scales[l] for l in i.levels])
        assert ((i.rois[:, 3] - i.rois[:, 1]) * sc >= 1).all(), name
        assert ((i.rois[:, 4] - i.rois[:, 2]) * sc >= 1).all(), name
        assert set(i.rois[:, 0].astype(int).tolist()) == {0, 1}, name
        if len(i.sizes) == 4:
            assert 100 <= len(i.rois) <= 150, (name, len(i.rois))
            assert set(i.levels.tolist()) == {0, 1, 2, 3}


MIN_BOUNDARY = 4   # samples exactly on each of -1, 0, N - 1 and N, per axis and case
MIN_BRANCH = 4     # merged tap rows / reused column pairs / slides / fresh pairs / edge samples


@pytest.mark.parametrize("name", NAMES + BWD_NAMES)
def test_boundary_counts(name):
    if name in R.BY_NAME:
        i = R.inputs(name)
        c = R.reach(i.rois, i.levels, i.scales, i.sizes, i.P, i.sr)
        sr = i.sr
    else:
        i = R.bwd_inputs(name)
        c = R.reach(i.rois, np.zeros(len(i.rois), np.int32), (i.scale,), (i.shape[2:],), i.P, i.sr)
        sr = i.sr
    print(name, dict(c))
    for tag in "xy":
        for what in ("-1", "0", "last", "N"):
            assert c["%s==%s" % (tag, what)] >= MIN_BOUNDARY, (name, tag, what, c)
        assert c[tag + " lattice zero weight"] >= MIN_BOUNDARY, (name, tag)   # lx = 0 inside
        assert c[tag + " dropped"] >= MIN_BOUNDARY, (name, tag)
    if sr == 2:   # what row_taps merges and what the sweep's column registers do
        for what in ("merged tap rows", "column pair reused", "column slid", "columns both new",
                     "right edge (xl == xh)"):
            assert c[what] >= MIN_BRANCH, (name, what, c)


@pytest.mark.parametrize("name", NAMES)
def test_most_outputs_are_non_zero(name):
    assert np.count_nonzero(R.reference(name)) > 0.6 * R.reference(name).size


@pytest.mark.parametrize("name", [c.name for c in R.PYRAMID])
def test_coverage(name):
    """Every pixel of every level map, in both images, carries a non-zero weight."""
    i = R.inputs(name)
    for l, cov in enumerate(R.coverage(i.rois, i.levels, i.scales, i.sizes, i.P, i.sr)):
        assert cov.all(), (name, l, np.argwhere(~cov)[:4])


def test_coverage_of_single_level_cases():
    for c in R.ONE_LEVEL:
        i = R.inputs(c.name)
        cov = R.coverage(i.rois, i.levels, i.scales, i.sizes, i.P, i.sr)[0]
        assert cov.all(), c.name


# ------------------------------------------------------------------ the oracle's C restatement
@pytest.mark.parametrize("name", NAMES)
def test_oracle_forward_equals_float64(name):
    """oracle.roi_align level by level, and oracle.roi_feature_transform over the pyramid
    (the per-level loop and the restore index), bit for bit."""
    i = R.inputs(name)
    ref = R.reference(name)
    for l in range(len(i.feats)):
        sel = i.levels == l
        got = orc.roi_align(i.feats[l], i.rois[sel], i.P, i.P, i.scales[l], i.sr)
        assert np.array_equal(got.astype(np.float64), ref[sel]), (name, l)
    if len(i.feats) == 4:
        got = orc.roi_feature_transform(list(i.feats[::-1]), R.fpn_blobs(i.rois, i.levels), "rois",
                                        i.P, list(i.scales[::-1]), i.sr)
        assert np.array_equal(got.astype(np.float64), ref), name


@pytest.mark.parametrize("name", BWD_NAMES)
def test_oracle_backward_equals_float64(name):
    i = R.bwd_inputs(name)
    got = orc.roi_align_backward(i.top, i.rois, i.shape, i.scale, i.sr)
    assert np.array_equal(got.astype(np.float64), R.bwd_reference(name))


# ------------------------------------------------------------------ the separable order, float32
def _row_taps(sh, bh, ph, H, SR, defect):
    """row_taps of csrc/roi_geom.hpp: the 2 SR y taps of output row ph, a pixel row named
    twice merged into its first tap (weights added)."""
    row, w, alive = [], [], []
    for iy in range(SR):
        y = sh + f32(ph) * bh + f32(iy + .5) * bh / f32(SR)
        ok = not (y <= -1 or y > H) if defect == "y <= -1" else not (y < -1 or y > H)
        if y <= 0:
            y = f32(0)
        yl = int(y)
        if yl >= H - 1:
            yh = yl = H - 1
            y = f32(yl)
        else:
            yh = yl + 1
        ly = y - f32(yl)
        row += [yl, yh]
        w += [f32(1) - ly, ly]
        alive += [ok, ok]
    for k in range(1, 2 * SR):
        for k2 in range(k):
            if alive[k] and alive[k2] and row[k2] == row[k]:
                if defect != "merged weight dropped":
                    w[k2] = w[k2] + w[k]
                alive[k] = False
    return row, w, alive


def separable_f32(feats, rois, levels, scales, P, segs=1, defect=None):
    """The product kernel's order (sep_row_sweep / combine_column of csrc/roi_align.hip) in
    float32 numpy, a vector over the channels: V(x) = sum over the merged y taps, once per
    distinct column; per bin sum_ix hx V(xl) + lx V(xh), times 1 / count.  Each row in
    `segs` runs of bins, every run starting with no column held.  feats[l]: [B, C, H, W].
    -> [R, C, P, P]."""
    SR = 2
    nhwc = [np.ascontiguousarray(f.transpose(0, 2, 3, 1)) for f in feats]
    C = nhwc[0].shape[3]
    out = np.zeros((len(rois), P, P, C), f32)
    for n, roi in enumerate(rois):
        l = int(levels[n])
        Bn, H, W, _ = nhwc[l].shape
        b = int(roi[0])
        if defect == "next image's base for b = 1" and b == 1:
            b = (b + 1) % Bn
        flat = nhwc[l][b].reshape(H * W, C)   # the RoI's image as the buffer resource sees it
        scale = f32(scales[min(l + 1, len(scales) - 1)] if defect == "next level's scale"
                    else scales[l])
        sw, sh, ew, eh = (f32(v) * scale for v in roi[1:5])
        rw, rh = max(ew - sw, f32(1)), max(eh - sh, f32(1))
        bh, bw = rh / f32(P), rw / f32(P)
        inv = f32(1) / f32(SR if defect == "count of SR" else SR * SR)
        for ph in range(P):
            row, tw, alive = _row_taps(sh, bh, ph, H, SR, defect)

            def column(x):
                v = np.zeros(C, f32)
                for k in range(2 * SR):
                    if alive[k]:
                        at = row[k] * W + x
                        v = v + tw[k] * (flat[at] if at < H * W else np.zeros(C, f32))
                return v
            for sg in range(segs):
                cl = ch = -1
                va = vb = np.zeros(C, f32)
                for pw in range(sg * P // segs, (sg + 1) * P // segs):
                    acc = np.zeros(C, f32)
                    for ix in range(SR):
                        x = sw + f32(pw) * bw + f32(ix + .5) * bw / f32(SR)
                        if x < -1 or (x >= W if defect == "x >= W" else x > W):
                            continue
                        if x <= 0:
                            x = f32(0)
                        xl = int(x)
                        if xl >= W - 1:
                            xh = W - 1
                            if defect != "xl left unclamped":
                                xl = W - 1
                            if defect != "clamp without x = xl":
                                x = f32(W - 1)
                        else:
                            xh = xl + 1
                        lx = x - f32(min(xl, W - 1))
                        hx = f32(1) - lx
                        if defect == "hx / lx swapped":
                            hx, lx = lx, hx
                        if xl != cl or xh != ch:
                            if xl == ch or (defect == "stale column reuse" and ch >= 0):
                                va = vb
                            else:
                                va = column(xl)
                            vb = va if xh == xl else column(xh)
                            cl, ch = xl, xh
                        acc = acc + (hx * va + lx * vb)
                    out[n, ph, pw] = acc * inv
    return out.transpose(0, 3, 1, 2)


def _sep(name, **kw):
    i = R.inputs(name)
    return separable_f32(i.feats, i.rois, i.levels, i.scales, i.P, **kw).astype(np.float64)


@pytest.mark.parametrize("name", [c.name for c in R.SEPARABLE])
def test_separable_order_equals_float64(name):
    assert np.array_equal(_sep(name), R.reference(name))


@pytest.mark.parametrize("segs", [2, 4, 7])
def test_separable_order_in_segments_equals_float64(segs):
    name = "p7-c4-minimum"
    assert np.array_equal(_sep(name, segs=segs), R.reference(name))


def test_single_level_separable_order_equals_float64():
    name = "p7-c24-one-level"
    assert np.array_equal(_sep(name), R.reference(name))


# ------------------------------------------------------------------ planted defects
SEP_DEFECTS = [
    ("x >= W", "p7-c4-minimum"),
    ("y <= -1", "p7-c4-minimum"),
    ("xl left unclamped", "p7-c4-minimum"),
    ("hx / lx swapped", "p7-c4-minimum"),
    ("merged weight dropped", "p7-c4-minimum"),
    ("stale column reuse", "p7-c4-minimum"),
    ("next image's base for b = 1", "p7-c4-minimum"),
    ("next level's scale", "p7-c4-minimum"),
    ("count of SR", "p7-c4-minimum"),
]


@pytest.mark.parametrize("defect,name", SEP_DEFECTS, ids=[d for d, _ in SEP_DEFECTS])
def test_planted_defect_breaks_equality(defect, name):
    got, ref = _sep(name, defect=defect), R.reference(name)
    bad = np.argwhere((got != ref).any(axis=(1, 2, 3))).ravel()
    print("%s on %s: %d of %d RoIs differ" % (defect, name, len(bad), len(ref)))
    assert len(bad) > 0


@pytest.mark.parametrize("defect,want", [("x >= W", "x==N"), ("y <= -1", "y==-1")])
def test_boundary_defects_show_only_on_the_boundary_samples(defect, want):
    """The two inclusive-bound defects change exactly the RoIs that have a sample on that
    bound: nothing else in the suite's inputs can see them."""
    name = "p7-c4-minimum"
    i = R.inputs(name)
    got, ref = _sep(name, defect=defect), R.reference(name)
    bad = set(np.argwhere((got != ref).any(axis=(1, 2, 3))).ravel().tolist())
    on = set(n for n in range(len(i.rois))
             if R.reach(i.rois[n:n + 1], i.levels[n:n + 1], i.scales, i.sizes, i.P, i.sr)[want])
    assert bad and bad <= on, (bad, on)


def test_right_edge_clamp_without_x_is_not_observable():
    """'The right-edge clamp without x = xl' cannot break equality, here or in any kernel:
    once xl = xh = W - 1 both taps read the same pixel, and the weights hx = 1 - lx and lx
    still add up to one for any lx in [0, 1] (x <= W is all that is in range), so
    hx v + lx v = v on the lattice.  The observable neighbour of that mistake -- xh clamped
    and xl left at (int)x = W for a sample exactly on W, a read of the next row's first
    pixel or past the image -- is the planted defect 'xl left unclamped' above."""
    for name in ("p7-c4-minimum", "p7-c24-one-level"):
        assert np.array_equal(_sep(name, defect="clamp without x = xl"), R.reference(name))
        i = R.inputs(name)
        assert R.reach(i.rois, i.levels, i.scales, i.sizes, i.P, i.sr)["x==N"] >= MIN_BOUNDARY


def backward_f32(top, rois, scale, shape, sr, defect=None):
    """The reference's backward in float32, sample by sample, a vector over the channels."""
    Bn, C, H, W = shape
    R_, _, P, _ = top.shape
    out = np.zeros((Bn, H, W, C), f32)
    scale = f32(scale)
    for n, roi in enumerate(rois):
        sw, sh, ew, eh = (f32(v) * scale for v in roi[1:5])
        rw, rh = max(ew - sw, f32(1)), max(eh - sh, f32(1))
        bh, bw = rh / f32(P), rw / f32(P)
        gh = sr if sr > 0 else int(np.ceil(rh / f32(P)))
        gw = sr if sr > 0 else int(np.ceil(rw / f32(P)))
        count = f32(gh * gw)
        plane = out[int(roi[0])]
        for ph in range(P):
            for iy in range(gh):
                y = sh + f32(ph) * bh + f32(iy + .5) * bh / f32(gh)
                if y < -1 or y > H:
                    continue
                if y <= 0:
                    y = f32(0)
                yl = int(y)
                if yl >= H - 1:
                    yh = yl = H - 1
                    y = f32(yl)
                else:
                    yh = yl + 1
                ly = y - f32(yl)
                hy = f32(1) - ly
                for pw in range(P):
                    g = top[n, :, ph, pw]
                    for ix in range(gw):
                        x = sw + f32(pw) * bw + f32(ix + .5) * bw / f32(gw)
                        if x < -1 or x > W:
                            continue
                        if x <= 0:
                            x = f32(0)
                        xl = int(x)
                        if xl >= W - 1:
                            xh = xl = W - 1
                            x = f32(xl)
                        else:
                            xh = xl + 1
                        lx = x - f32(xl)
                        hx = f32(1) - lx
                        plane[yl, xl] += g * (hy * hx) / count
                        plane[yl, xh] += g * (hy * lx) / count
                        plane[yh, xl] += g * (ly * hx) / count
                        if defect != "scatter tap dropped":
                            plane[yh, xh] += g * (ly * lx) / count
    return out.transpose(0, 3, 1, 2)


@pytest.mark.parametrize("name", BWD_NAMES)
def test_backward_restatement_and_its_planted_defect(name):
    i = R.bwd_inputs(name)
    ref = R.bwd_reference(name)
    got = backward_f32(i.top, i.rois, i.scale, i.shape, i.sr).astype(np.float64)
    assert np.array_equal(got, ref)
    # the same sum in another order: RoIs reversed
    rev = backward_f32(i.top[::-1], i.rois[::-1], i.scale, i.shape, i.sr).astype(np.float64)
    assert np.array_equal(rev, ref)
    bad = backward_f32(i.top, i.rois, i.scale, i.shape, i.sr, "scatter tap dropped")
    assert not np.array_equal(bad.astype(np.float64), ref)


# ------------------------------------------------------------------ why the lattice
def test_float32_orders_differ_on_real_data():
    """On randn features and continuous RoIs the reference's per-sample order (the oracle's C)
    and the separable order differ in the last bits: only a tolerance can compare them."""
    rng = np.random.default_rng(5)
    H, W = R.SIZES[1]
    f = rng.standard_normal((R.B, 8, H, W)).astype(f32)
    xy = rng.uniform(0, 250, (40, 2))
    rois = np.hstack([rng.integers(0, R.B, (40, 1)), xy, xy + rng.uniform(12, 120, (40, 2))])
    rois = rois.astype(f32)
    a = orc.roi_align(f, rois, 7, 7, R.SCALES[1], 2)
    b = separable_f32([f], rois, np.zeros(40, np.int32), [R.SCALES[1]], 7)
    assert not np.array_equal(a, b)
    np.testing.assert_allclose(b, a, rtol=1e-4, atol=1e-4)
    # and on lattice RoIs with randn features
    i = R.inputs("p7-c24-one-level")
    g = rng.standard_normal(i.feats[0].shape).astype(f32)
    a = orc.roi_align(g, i.rois, i.P, i.P, i.scales[0], i.sr)
    b = separable_f32([g], i.rois, i.levels, i.scales, i.P)
    assert not np.array_equal(a, b)
