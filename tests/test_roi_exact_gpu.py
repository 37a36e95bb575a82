"""The RoIAlign kernels on dyadic RoI lattices (tests/roi_exact_ref.py): every output must
EQUAL the float64 reference, bit for bit -- the product kernel (variant 10) in its SIMPLE and
general forms, in row segments and workgroup parts, its siblings (variants 8, 11, 13), the
reference-order kernels (variants 3 and 30, the NCHW drop-in, the generic kernel), under
any RoI schedule and in both output layouts, and the atomics-based backward.  There is no
tolerance in this file: on the lattice the reference's order, the separable order and
atomics in any order all give the same float32 (tests/test_roi_exact_cpu.py shows that,
and which planted mistakes break it).  The float64 casts are compared on the device
(-0 equals 0, NaN equals nothing); a mismatch is reported from numpy.

Guard zones, as in tests/test_conv_exact_gpu.py: each level map is a contiguous view in the
middle of a larger buffer whose guards hold NaN, so a tap outside the map that reaches a
result poisons it; `out` is a view inside a buffer pre-filled, guards included, with a bit
pattern no result can equal, so an unwritten output and a store outside `out` show."""
import functools

import numpy as np
import pytest
import torch

from tests import roi_exact_ref as R
from tests.test_conv_exact_gpu import GUARD, SENTINEL

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ guarded buffers
def _carve(shape, fill):
    n = int(np.prod(shape))
    buf = torch.empty(2 * GUARD + n, dtype=torch.float32, device=DEV)
    if fill is None:
        buf.view(torch.int32).fill_(SENTINEL)
    else:
        buf.fill_(fill)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guarded(a):
    """A numpy array on the device between NaN guards, contiguous in a's own shape."""
    _, v = _carve(a.shape, float("nan"))
    v.copy_(torch.from_numpy(np.array(a)))
    return v


def _to_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the cached inputs are read-only


@functools.lru_cache(maxsize=None)
def _dev(name):
    """(NHWC level maps between NaN guards, rois, levels, float64 reference), on the device."""
    i = R.inputs(name)
    ref = R.reference(name)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    nhwc = [_guarded(f.transpose(0, 2, 3, 1)) for f in i.feats]
    return nhwc, _to_dev(i.rois), _to_dev(i.levels), _to_dev(ref)


def _equal64(out, ref, what):
    """out (float32, [R, C, P, P] as indexed) against the float64 reference, on the device."""
    assert tuple(out.shape) == tuple(ref.shape), (what, out.shape, ref.shape)
    if torch.equal(out.double(), ref):
        return
    a, b = out.double().cpu().numpy(), ref.cpu().numpy()
    assert not np.array_equal(a, b)
    bad = np.argwhere(a != b)
    raise AssertionError("%s: %d of %d outputs differ (%d RoIs), first at %s: %r, float64 says %r" % (
        what, len(bad), a.size, len(set(bad[:, 0].tolist())), tuple(bad[0]), a[tuple(bad[0])],
        b[tuple(bad[0])]))


def _verify(buf, out, ref, what, rows=None):
    """Guards untouched, every element of `out` written, rows [0, rows) equal to ref."""
    torch.cuda.synchronize()
    bits = buf.view(torch.int32)
    n = out.numel()
    assert bool((bits[:GUARD] == SENTINEL).all()), what + ": a store before out"
    assert bool((bits[GUARD + n:] == SENTINEL).all()), what + ": a store past out"
    assert not bool((bits[GUARD:GUARD + n] == SENTINEL).any()), what + ": an unwritten output"
    _equal64(out if rows is None else out[:rows], ref, what)


def _fpn(name, out_layout="nhwc", order=None, levels=True):
    """ops.roi_align_fpn on the case through out=, verified."""
    from vosdetectron_amd import ops
    nhwc, rois, lv, ref = _dev(name)
    i = R.inputs(name)
    n = len(i.rois)
    shape = (n, i.P, i.P, i.C) if out_layout == "nhwc" else (n, i.C, i.P, i.P)
    buf, out = _carve(shape, None)
    y = ops.roi_align_fpn(nhwc, list(i.scales), rois, lv if levels else None, i.P, i.sr,
                          roi_order=order, out=out, out_layout=out_layout)
    assert y is out
    _verify(buf, out.permute(0, 3, 1, 2) if out_layout == "nhwc" else out, ref,
            "%s out=%s order=%s" % (name, out_layout, order is not None))


def _orders(name):
    """The engine's XCD schedule and a random permutation."""
    from vosdetectron_amd import ops
    _, rois, lv, _ = _dev(name)
    perm = np.random.default_rng(len(rois)).permutation(len(rois)).astype(np.int32)
    return ops.xcd_roi_order(rois, lv), torch.from_numpy(perm).to(DEV)


# ------------------------------------------------------------------ forward over the pyramid
# name -> (environment, what it selects)
MODES = {
    "default": ({}, "the product launch: variant 10, SIMPLE for C <= 256, general above"),
    "general": ({"VOSDET_RA_GENERAL": "1"}, "variant 10's general form at any C"),
    "segs2": ({"VOSDET_RA_SEGS": "2"}, "each output row in two runs of bins"),
    "segs4-parts2": ({"VOSDET_RA_SEGS": "4", "VOSDET_RA_PARTS": "2"},
                     "four runs, a RoI's units over two workgroups"),
    "variant8": ({"VOSDET_ROIALIGN_VARIANT": "8"}, "the sweep through global loads"),
    "variant11": ({"VOSDET_ROIALIGN_VARIANT": "11"}, "pipelined two columns ahead (C <= 256)"),
    "variant13": ({"VOSDET_ROIALIGN_VARIANT": "13"}, "pipelined one column ahead (C <= 256)"),
    "variant3": ({"VOSDET_ROIALIGN_VARIANT": "3"}, "the reference-order row kernel"),
    "variant30": ({"VOSDET_ROIALIGN_VARIANT": "30"}, "the tile-binned kernel (C % 32 == 0)"),
    "variant30-chunk16": ({"VOSDET_ROIALIGN_VARIANT": "30", "VOSDET_RA_CHUNK": "16"},
                          "the tile-binned kernel, every tile in many items"),
}
ENV = ("VOSDET_ROIALIGN_VARIANT", "VOSDET_RA_GENERAL", "VOSDET_RA_SEGS", "VOSDET_RA_PARTS",
       "VOSDET_RA_CHUNK")


def _set_env(monkeypatch, mode):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode][0].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [c.name for c in R.SEPARABLE])
def test_fpn_forward_exact(name, mode, monkeypatch):
    """Each launch form on each sr = 2 pyramid case: NHWC output in RoI order, under the XCD
    schedule and under a random permutation, and NCHW output (variant 8's LDS tile where
    C P P floats fit, the row kernel above that).  The reference-order row kernel writes
    NHWC for P of 7 and 14 only; at another P it is run through its NCHW output, which has
    no schedule argument (the generic kernel).

    p14-c256-mask-head under variant 13 and the XCD schedule is the run that found the
    pipelined sweep storing pixel (0, 0) for a RoI wholly off the map (its padding loads
    were drained after the last stores; profiles/roi_exact/README.md)."""
    _set_env(monkeypatch, mode)
    P = R.BY_NAME[name].P
    rows_only = mode == "variant3" and P not in (7, 14)
    if not rows_only:
        _fpn(name, "nhwc")
        for order in _orders(name):
            _fpn(name, "nhwc", order)
    _fpn(name, "nchw")
    if not rows_only:
        _fpn(name, "nchw", _orders(name)[0])


@pytest.mark.parametrize("variant", [None, "3"])
def test_fpn_forward_adaptive_grid_exact(variant, monkeypatch):
    """sr = 0 over the pyramid (grids of 1, 2 and 4, count up to 16): the row kernel's
    runtime-grid form, whatever variant is selected."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if variant:
        monkeypatch.setenv("VOSDET_ROIALIGN_VARIANT", variant)
    name = "p7-c64-sr0-pyramid"
    _fpn(name, "nhwc")
    _fpn(name, "nchw")
    for order in _orders(name):
        _fpn(name, "nhwc", order)


# ------------------------------------------------------------------ single-level paths
@pytest.mark.parametrize("name", ["p7-c24-one-level", "p7-c24-sr0-one-level"])
def test_single_level_paths_exact(name, monkeypatch):
    """One level: roi_align_fpn on NHWC with and without a level index per RoI,
    layout='nchw', and the NCHW drop-in ops.roi_align_forward (it allocates its output:
    equality alone)."""
    from vosdetectron_amd import ops
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    i = R.inputs(name)
    _, rois, _, ref = _dev(name)
    for levels in (True, False):
        _fpn(name, "nhwc", levels=levels)
        _fpn(name, "nchw", levels=levels)
    nchw = _guarded(i.feats[0])
    buf, out = _carve((len(i.rois), i.C, i.P, i.P), None)
    y = ops.roi_align_fpn([nchw], list(i.scales), rois, None, i.P, i.sr, layout="nchw", out=out)
    assert y is out
    _verify(buf, out, ref, name + " layout=nchw")
    y = ops.roi_align_forward(nchw, rois, i.P, i.P, i.scales[0], i.sr)
    torch.cuda.synchronize()
    _equal64(y, ref, name + " roi_align_forward")


@pytest.mark.parametrize("name", ["p5-c24-sr0-generic", "p6-c24-sr4-generic"])
def test_generic_kernel_exact(name, monkeypatch):
    """PH == PW not in {7, 14} with sr != 2: the any-size kernel (NCHW output)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    _fpn(name, "nchw")
    _fpn(name, "nchw", levels=False)


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", [c.name for c in R.BWD_CASES])
def test_backward_exact(name):
    """ops.roi_align_backward on integer top_grad, dozens of RoIs scattering into the same
    pixels: atomics in any order give the float64 sum exactly.  top_grad between NaN guards;
    bottom_grad is allocated by the entry point."""
    from vosdetectron_amd import ops
    i = R.bwd_inputs(name)
    ref = _to_dev(R.bwd_reference(name))
    top = _guarded(i.top)
    rois = _to_dev(i.rois)
    for _ in range(2):   # the arrival order is free to differ between launches
        got = ops.roi_align_backward(top, rois, i.shape, i.scale, i.sr)
        torch.cuda.synchronize()
        _equal64(got, ref, name)


# ------------------------------------------------------------------ the engine's calls
ROI_LEVELS = (2, 3, 4, 5)


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("head,name", [("box", "p7-c256-simple-launch"),
                                       ("mask", "p14-c256-mask-head")])
def test_engine_calls_exact(head, name, fast, monkeypatch):
    """RoIAlign as vosdetectron_amd/engine.py calls it.  The pyramid is the permuted view of
    channels_last NCHW maps (nhwc_pyramid), the scales are 1 / 2 ** level, the RoIs a
    [frames, rois, 5] batch viewed flat with int32 levels.  Box head (_box_branch): P = 7,
    roi_order = xcd_roi_order(rois, levels), NHWC output on the fast path and NCHW otherwise.
    Mask head (_roi_head): P = 14, no schedule, the batch padded with zero boxes whose
    outputs are never read -- here they must be written, inside `out`, and leave the real
    rows exact."""
    from vosdetectron_amd import ops
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    i = R.inputs(name)
    nhwc, rois, lv, ref = _dev(name)
    feats = [t.permute(0, 3, 1, 2) for t in nhwc]
    assert all(t.is_contiguous(memory_format=torch.channels_last) for t in feats)
    pyr = [t.permute(0, 2, 3, 1) for t in feats]
    scales = [1. / 2 ** l for l in ROI_LEVELS]
    n = len(i.rois)
    pad = 0
    if head == "mask":
        pad = -n % 64
        rois = torch.cat([rois, rois.new_zeros((pad, 5))])
        lv = torch.cat([lv, lv.new_zeros((pad,))])
    rois3 = rois.view(1, n + pad, 5)
    flat_rois, flat_lvl = rois3.view(-1, 5), lv.view(-1)
    layout = "nhwc" if fast else "nchw"
    shape = (n + pad, i.P, i.P, i.C) if fast else (n + pad, i.C, i.P, i.P)
    buf, out = _carve(shape, None)
    if head == "box":
        y = ops.roi_align_fpn(pyr, scales, flat_rois, flat_lvl, i.P, i.sr,
                              roi_order=ops.xcd_roi_order(flat_rois, flat_lvl),
                              out_layout=layout, out=out)
    elif fast:
        y = ops.roi_align_fpn(pyr, scales, flat_rois, flat_lvl, i.P, i.sr, out_layout="nhwc",
                              out=out)
    else:
        y = ops.roi_align_fpn(pyr, scales, flat_rois, flat_lvl, i.P, i.sr, out=out)
    assert y is out
    _verify(buf, out.permute(0, 3, 1, 2) if fast else out, ref,
            "%s head fast=%s" % (head, fast), rows=n)
