"""The 3x3 conv kernels and the stem on integer-lattice inputs (tests/conv_exact_ref.py):
the output must EQUAL the float64 direct convolution, bit for bit, in every form -- the
implicit GEMM (csrc/conv3x3.hip), Winograd F(2x2) and its mosaics (conv3x3_wino.hip),
F(4x4) in its research forms, block plans, pairs, octets, row stacks, the grid, the
grouped and the dilated form (conv3x3_wino4.hip), both stem cores (stem.hip) -- with and
without bias and ReLU.  A dropped, duplicated or misplaced tap, a wrong transform
coefficient, a padding tap that is not zero or a skipped channel chunk fails at any
magnitude and any tile position; no tolerance is involved.

Guard zones: x and `out` are carved from the middle of larger flat buffers (more than
64 KiB on either side).  x's guards hold NaN, so an out-of-image tap read from memory
and not taken as zero poisons the output; `out` and its guards hold a bit pattern no
lattice result can equal, so an unwritten output and a store past either end show."""
import contextlib
import os

import pytest
import torch

from tests import conv_exact_ref as R
from tests.test_wino4_forms_gpu import FORMS

pytestmark = pytest.mark.gpu

GUARD = 16384 + 4      # floats on either side: 64 KiB and one 16-byte step
SENTINEL = -8388611    # 0xff7ffffd as int32: finite, about -3.4e38, not on any lattice


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _carve(shape):
    """(flat buffer, its middle as a channels_last [N][C][H][W] view)."""
    N, C, H, W = shape
    n = N * C * H * W
    buf = torch.empty(2 * GUARD + n, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n].view(N, H, W, C).permute(0, 3, 1, 2)
    assert view.is_contiguous(memory_format=torch.channels_last) or n == 0
    return buf, view


def _guarded_x(x_cpu):
    buf, x = _carve(tuple(x_cpu.shape))
    buf.fill_(float("nan"))
    x.copy_(x_cpu.cuda())
    return x


def _guarded_out(shape):
    buf, out = _carve(shape)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf, out


def _verify(buf, out, ref, what):
    bits = buf.view(torch.int32)
    n = out.numel()
    assert bool((bits[:GUARD] == SENTINEL).all()), "%s: a store before out" % (what,)
    assert bool((bits[GUARD + n:] == SENTINEL).all()), "%s: a store past out" % (what,)
    assert not bool(torch.isnan(out).any()), "%s: NaN in out" % (what,)
    if not torch.equal(out, ref):
        bad = (out != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d outputs differ, first at (n, c, y, x) = %s: %r, "
                             "float64 says %r" % (what, bad.shape[0], n, i, float(out[i]),
                                                   float(ref[i])))


def _reference(c, bias, dilation=1):
    ref = R.reference(c, bias, dilation)
    assert torch.equal(ref.float().double(), ref)
    return ref.float().cuda()


def _exact(c, launch, dilation=1, what=""):
    """launch(x, bias, relu, out) on the case's guarded lattice input, bias present and
    absent, ReLU off and on: `out` is returned, equals the float64 reference, its guards
    are untouched."""
    x_cpu, _, b_cpu = R.inputs(c)
    x = _guarded_x(x_cpu)
    for bias in (True, False):
        pre = _reference(c, bias, dilation)
        b = b_cpu.cuda() if bias else None
        for relu in (False, True):
            buf, out = _guarded_out((c.N, c.Co, c.H, c.W))
            y = launch(x, b, relu, out)
            torch.cuda.synchronize()
            assert y is out, (what, y)
            _verify(buf, out, torch.relu(pre) if relu else pre,
                    "%s %s bias=%s relu=%s" % (R.case_id(c), what, bias, relu))


def _ids(cases):
    return [R.case_id(c) for c in cases]


# ------------------------------------------------------------------ F(4x4)
@pytest.mark.parametrize("form", ["default"] + sorted(FORMS))
@pytest.mark.parametrize("c", R.W4_PLAIN, ids=_ids(R.W4_PLAIN))
def test_wino4_plain_exact(c, form):
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino4_weight(R.inputs(c)[1].cuda())
    run = lambda x, b, relu, out: ops.conv3x3_wino4_bias_act(x, u, b, relu=relu, out=out)
    with _env(FORMS.get(form, {})):
        _exact(c, run, what=form)
        for plan in R.W4_PLANS.get((c.N, c.C, c.H, c.W, c.Co), ()):
            with _env({"VOSDET_WINO4_PLAN": plan}):
                _exact(c, run, what="%s plan %s" % (form, plan))


@pytest.mark.parametrize("c", R.W4_PAIR + R.W4_OCTET, ids=_ids(R.W4_PAIR + R.W4_OCTET))
def test_wino4_pair_octet_exact(c):
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino4_weight(R.inputs(c)[1].cuda())
    _exact(c, lambda x, b, relu, out: ops.conv3x3_wino4_bias_act(x, u, b, relu=relu, out=out,
                                                                 mosaic="pair"), what="pair")


@pytest.mark.parametrize("c,plans", R.W4_ROWS, ids=_ids([c for c, _ in R.W4_ROWS]))
def test_wino4_rows_exact(c, plans):
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino4_weight(R.inputs(c)[1].cuda())
    for plan in plans:
        with _env({"VOSDET_WINO4_PLAN": plan}):
            _exact(c, lambda x, b, relu, out: ops.conv3x3_wino4_bias_act(
                x, u, b, relu=relu, out=out, mosaic="rows"), what="rows plan %s" % plan)


@pytest.mark.parametrize("c", R.W4_GRID, ids=_ids(R.W4_GRID))
def test_wino4_grid_exact(c):
    """The grid's tiles straddle maps (other tile offsets than one map per block): on
    real data only equal within Winograd rounding, on the lattice (the data-free
    condition) exact."""
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino4_weight(R.inputs(c)[1].cuda())
    _exact(c, lambda x, b, relu, out: ops.conv3x3_wino4_bias_act(x, u, b, relu=relu, out=out,
                                                                 mosaic="grid"), what="grid")


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("c", R.W4_GROUPED, ids=_ids(R.W4_GROUPED))
def test_wino4_grouped_exact(c, rows):
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino4_grouped_weight(R.inputs(c)[1].cuda(), c.groups)
    assert u is not None
    _exact(c, lambda x, b, relu, out: ops.conv3x3_wino4_bias_act(
        x, u, b, relu=relu, out=out, groups=c.groups, mosaic="rows" if rows else False),
        what="grouped rows=%s" % rows)


@pytest.mark.parametrize("layout", R.DILATED_LAYOUTS)
@pytest.mark.parametrize("c,served", R.W4_DILATED, ids=_ids([c for c, _ in R.W4_DILATED]))
def test_wino4_dilated2_exact(c, served, layout):
    """Dilation 2 / pad 2, read and written in place in the full maps; a (shape, layout)
    pair the entry does not serve answers None and nothing else."""
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino4_weight(R.inputs(c)[1].cuda())
    run = lambda x, b, relu, out: ops.conv3x3_wino4_dilated2_bias_act(x, u, b, relu=relu,
                                                                      out=out, layout=layout)
    if layout in served:
        _exact(c, run, dilation=2, what="dilated %s" % (layout,))
        return
    x = _guarded_x(R.inputs(c)[0])
    buf, out = _guarded_out((c.N, c.Co, c.H, c.W))
    assert run(x, None, False, out) is None
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENTINEL).all())


# ------------------------------------------------------------------ F(2x2)
W2 = [(c, False) for c in R.W2_PLAIN] + [(c, True) for c in R.W2_SEG] + [(c, "2d") for c in R.W2_2D]


@pytest.mark.parametrize("c,mosaic", W2, ids=["%s-%s" % (R.case_id(c), m) for c, m in W2])
def test_wino2_exact(c, mosaic):
    from vosdetectron_amd import ops
    u = ops.conv3x3_wino_weight(R.inputs(c)[1].cuda())
    _exact(c, lambda x, b, relu, out: ops.conv3x3_wino_bias_act(x, u, b, relu=relu, out=out,
                                                                mosaic=mosaic),
           what="F(2x2) mosaic=%s" % (mosaic,))


# ------------------------------------------------------------------ implicit GEMM
@pytest.mark.parametrize("env", R.GEMM_VARIANTS, ids=lambda e: "-".join(
    "%s%s" % (k.rsplit("_", 1)[1].lower(), v) for k, v in e.items()))
@pytest.mark.parametrize("c", R.GEMM, ids=_ids(R.GEMM))
def test_conv3x3_gemm_exact(c, env):
    from vosdetectron_amd import ops
    w2 = ops.conv3x3_weight(R.inputs(c)[1].cuda())
    with _env(env):
        _exact(c, lambda x, b, relu, out: ops.conv3x3_bias_act(x, w2, b, relu=relu, out=out),
               what=str(env))


# ------------------------------------------------------------------ stem
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("c", R.STEM, ids=_ids(R.STEM))
def test_stem_exact(c, split):
    """Both conv1 cores; the split-bf16 one keeps every bit of operands of 8 and 16
    significant bits (conv_exact_ref.STEM_BITS).  The entry allocates its output, so
    only the input is guarded."""
    from vosdetectron_amd import ops
    x_cpu, w, b = R.inputs(c)
    x = _guarded_x(x_cpu)
    got = ops.stem_conv_pool(x, ops.stem_pack(w.cuda(), split=split), b.cuda())
    torch.cuda.synchronize()
    ref = _reference(c, True)
    assert got.shape == ref.shape and not bool(torch.isnan(got).any())
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s split=%s: %d of %d differ, first at %s: %r, float64 says %r" % (
            R.case_id(c), split, bad.shape[0], got.numel(), i, float(got[i]), float(ref[i])))
