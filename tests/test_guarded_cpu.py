"""Device-free half of the guarded-buffer tests:

  1. the harness itself (tests/guarded.py) on CPU tensors -- a fake op that writes one
     byte before, one byte after or one row after its carve is caught and the carve
     named; so is one that stores the canary's own value; a clean op passes; the reuse
     mode returns the same offsets;
  2. every case of tests/guarded_cases.py reaches the branch it is there for, shown
     from the oracle and host arithmetic alone, so a case that stops reaching its
     branch fails here instead of passing vacuously on the GPU;
  3. every workspace-taking C entry refuses a workspace one byte short, and a null
     one, with VD_ERR_WORKSPACE before it launches anything."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import guarded as G
from tests import guarded_capi
from tests import guarded_cases as GC


# --------------------------------------------------------------------------- 1. the arena
@pytest.fixture
def arena():
    return G.Arena("cpu", 1 << 20)


def _flat(arena, view):
    """The arena bytes from the view's first byte on (what a stray index reaches)."""
    off = view.data_ptr() - arena.buf.data_ptr()
    return off, arena.buf


def test_carve_is_exact_aligned_and_filled(arena):
    a = arena.carve((3, 5), torch.float32, G.ONES, "a")
    b = arena.carve((7,), torch.int32, G.ZERO, "b")
    z = arena.carve((0, 5), torch.float32, G.ONES, "z")
    assert a.shape == (3, 5) and a.is_contiguous() and bool(torch.isnan(a).all())
    assert b.tolist() == [0] * 7 and z.numel() == 0
    for v in (a, b):
        off = v.data_ptr() - arena.buf.data_ptr()
        assert off % 256 == 0 and off >= G.MIN_STRIP
    # exact: the byte after the 60 requested is canary, not carve
    off, buf = _flat(arena, a)
    assert buf[off + 60] != 0xFF or buf[off + 61] != 0xFF
    assert (b.data_ptr() - a.data_ptr()) >= 60 + G.MIN_STRIP
    arena.check()


def test_strip_is_at_least_one_leading_stride(arena):
    rows = arena.carve((4, 3000), torch.float32, G.ZERO, "rows")  # 12000-byte rows
    nxt = arena.carve((4,), torch.int32, G.ZERO, "next")
    assert nxt.data_ptr() - (rows.data_ptr() + rows.numel() * 4) >= 12000
    assert rows.data_ptr() - arena.buf.data_ptr() >= 12000


@pytest.mark.parametrize("where,side", [(-1, "BEFORE"), (0, "AFTER"), ("row", "AFTER")])
def test_stray_write_is_caught_and_named(arena, where, side):
    arena.carve((16,), torch.uint8, G.ZERO, "left neighbour")
    out = arena.carve((6, 40), torch.int32, G.ZERO, "the output")
    arena.carve((16,), torch.uint8, G.ZERO, "right neighbour")
    off, buf = _flat(arena, out)
    n = out.numel() * 4
    if where == "row":  # row index 6 of 6: one leading stride past the end
        buf[off + n:off + n + 160] = 7
    else:
        p = off + (where if where < 0 else n)
        buf[p] = (int(buf[p]) + 1) & 0xFF
    with pytest.raises(AssertionError) as e:
        arena.check("fake op")
    msg = str(e.value)
    assert "the output" in msg and side in msg and "neighbour" not in msg, msg
    assert ("1 canary bytes" in msg) if where != "row" else ("160 canary bytes" in msg or
                                                              "159 canary bytes" in msg), msg


def test_the_canarys_own_value_is_caught(arena):
    """A fake op that stores, as one 32-bit word, the canary byte it finds at a canary
    position: the pattern is position-dependent, so three of the four bytes differ.
    (A single byte that equals its own canary is no change of memory at all.)"""
    out = arena.carve((8,), torch.float32, G.ZERO, "out")
    off, buf = _flat(arena, out)
    p = off + 32  # the first canary byte after the carve
    buf[p:p + 4] = int(buf[p])
    with pytest.raises(AssertionError, match="out: 3 canary bytes AFTER"):
        arena.check()
    period = G._canary_period()
    assert (period[1:] != period[:-1]).all()
    words = period.view(np.uint32)
    assert (words[1:] != words[:-1]).all()          # neighbouring 32-bit words differ
    assert (period[256:] != period[:-256]).all()    # and so do bytes one 256-byte page apart


def test_clean_op_passes_and_fills_are_offered(arena):
    a = arena.carve((5, 5), torch.float32, G.ONES, "a")
    b = arena.carve((9,), torch.int64, G.ZERO, "b")
    a.copy_(torch.arange(25.).view(5, 5))
    b[:3] = torch.tensor([4, 5, 6])
    arena.check()
    G.assert_prefill(b[3:], G.ZERO, "b rows >= 3")
    with pytest.raises(AssertionError, match="b rows: 1 bytes"):
        G.assert_prefill(b[2:], G.ZERO, "b rows")
    i = arena.carve((4,), torch.int32, G.ONES, "i")
    assert i.tolist() == [-1] * 4


def test_reuse_returns_the_same_offsets_and_keeps_the_bytes(arena, monkeypatch):
    big = arena.carve((1000,), torch.uint8, G.ONES, "big", key="k")
    big[:] = 9
    other = arena.carve((10,), torch.uint8, G.ZERO, "other")
    small = arena.carve((300,), torch.uint8, G.KEEP, "small", key="k")
    assert small.data_ptr() == big.data_ptr() and bool((small == 9).all())
    # the bytes of the larger carve beyond the smaller one are canary again
    arena.check()
    off, buf = _flat(arena, small)
    buf[off + 300] ^= 0xFF
    with pytest.raises(AssertionError, match="small: 1 canary bytes AFTER"):
        arena.check()
    buf[off + 300] ^= 0xFF
    arena.check()
    assert other.data_ptr() > big.data_ptr()
    # guarded_ws: same call site -> same offset, no refill; exact sizes; 0 bytes -> length 0
    from vosdetectron_amd import ops
    arena.reset()
    log = G.guarded_ws(monkeypatch, arena, G.ONES, reuse=True)

    def site(n):
        return ops._ws(n, "cpu")

    w1 = site(1000)
    assert w1.numel() == 1000 and bool((w1 == 0xFF).all())
    w1[:] = 3
    w2 = site(999)
    assert w2.numel() == 999 and w2.data_ptr() == w1.data_ptr() and bool((w2 == 3).all())
    z = site(0)
    assert z.numel() == 0 and z.data_ptr() == w1.data_ptr()
    assert [n for _, n, _ in log] == [1000, 999, 0] and len({o for _, _, o in log}) == 1
    arena.check()
    log = G.guarded_ws(monkeypatch, arena, G.ZERO)  # not reuse: a fresh carve per request
    a, b = site(100), site(100)
    assert a.data_ptr() != b.data_ptr() and a.numel() == 100 and not bool(a.any())
    zero = site(0)  # 256 bytes of canary, length 0, a pointer into the arena
    assert zero.numel() == 0 and zero.data_ptr() > b.data_ptr()
    arena.check()


# --------------------------------------------------------------------------- 2. the cases
def test_nms_sizes_straddle_the_lds_limit():
    b = GC.nms_lds_boundary()
    max_n, lds = GC.nms_constants()
    words = lambda n: (n + 63) // 64  # noqa: E731
    assert 8 * b * words(b) + 2 * max_n + 256 <= lds < 8 * (b + 1) * words(b + 1) + 2 * max_n + 256
    assert 65 < b < b + 1 < max_n == GC.nms_sizes()[-1]
    for n in GC.nms_sizes():
        d = GC.nms_dets(n)
        keep = orc.nms(d, 0.5)
        assert len(np.unique(d[:, 4])) <= 16  # ties
        if n > 64:
            assert 1 < len(keep) < n
            # suppression in every 64-block of the processing order
            order = np.lexsort((np.arange(n), d[:, 4]))[::-1]
            gone = ~np.isin(order, keep)
            assert all(gone[i:i + 64].any() for i in range(0, n - 63, 64))


def _rpn_size(name, env, monkeypatch):
    from vosdetectron_amd import _lib
    for k in GC.RPN_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    levels, pre = GC.RPN_CASES[name][:2]
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    descs = (_lib.VdRpnLevel * len(levels))()
    for i, (A, H, W) in enumerate(levels):
        descs[i] = _lib.VdRpnLevel(p, p, p, A, H, W, 1. / 16)
    return _lib.lib().vd_generate_proposals_workspace_size(descs, len(levels), 2, pre)


def test_proposal_cases_reach_their_layouts(monkeypatch):
    """Sizes compared between cases, per slot: the split layout holds box and key arrays
    besides the mask, the unsplit one does not; PRESEL=0 drops the select slots; a large
    case's slot holds more than the largest small slot by at least what the box and key
    arrays of its pre take; pre = 40 is sized as pre = 64; the level past the large
    variant's rows cannot be planned."""
    nosel = {"VOSDET_RPN_PRESEL": "0"}
    unsplit_nosel = {"VOSDET_RPN_SPLIT": "0", "VOSDET_RPN_PRESEL": "0"}
    size = {n: _rpn_size(n, GC.RPN_CASES[n][5], monkeypatch) for n in GC.RPN_CASES}
    split = size["small-split"]
    assert size["small-unsplit"] < split                     # no box / key arrays
    assert size["small-presel0"] < split                     # no select slots
    slots = 2 * len(GC.RPN_LEVELS)
    boxes_keys_1000 = (size["small-presel0"] - _rpn_size("small-unsplit", unsplit_nosel,
                                                         monkeypatch)) // slots
    assert boxes_keys_1000 > 0                               # per slot at pre 1000
    # the largest small slot: the mask alone at pre = kPreMax = 2048, one level, two images
    monkeypatch.setitem(GC.RPN_CASES, "mask2048", (((15, 24, 30),), 2048, 300, 0.7, 0, {}, ""))
    mask_2048 = _rpn_size("mask2048", unsplit_nosel, monkeypatch) // 2
    by_pre = _rpn_size("large-by-pre", nosel, monkeypatch) // 2
    take_all = _rpn_size("large-take-all", nosel, monkeypatch) // 2
    source = _rpn_size(GC.RPN_LEFTOVER, nosel, monkeypatch) // 2
    assert by_pre >= mask_2048 + 2 * boxes_keys_1000         # pre 2049: arrays of > 2x1000 rows
    assert take_all > by_pre + 3 * boxes_keys_1000 and source > take_all   # 7935, 8100 rows
    assert size["small-pre40"] < split
    monkeypatch.setitem(GC.RPN_CASES, "pre64", (GC.RPN_LEVELS, 64, 300, 0.7, 0, {}, ""))
    assert _rpn_size("pre64", {}, monkeypatch) == size["small-pre40"]      # laid out as p = 64
    # take-all of 8640 anchors is past the large variant's rows: "cannot plan" (256 bytes)
    monkeypatch.setitem(GC.RPN_CASES, "refused", GC.RPN_REFUSED + ({}, ""))
    assert _rpn_size("refused", {}, monkeypatch) == 256
    # the leftover source is larger than every case it precedes, under that case's switches
    for n, case in GC.RPN_CASES.items():
        if n in GC.RPN_CASES and n != GC.RPN_LEFTOVER and case[6]:
            assert _rpn_size(GC.RPN_LEFTOVER, case[5], monkeypatch) > \
                _rpn_size(n, case[5], monkeypatch), n
    # levels: the last small level is take-all at pre 1000, the others are not
    assert [a * h * w > 1000 for a, h, w in GC.RPN_LEVELS] == [True, True, False]


def test_proposal_cases_reach_their_counts():
    for name in GC.RPN_CASES:
        post = GC.RPN_CASES[name][2]
        counts = [[len(r) for r, _ in lv] for lv in GC.rpn_reference(name)]
        if name == "all-filtered":
            assert counts == [[0, 0]] * 3
        else:
            assert all(0 < c <= post for lv in counts for c in lv), (name, counts)
            # a full level and a partly filled one: rows past the count exist
            assert any(c < post for lv in counts for c in lv) or len(counts) == 1, (name, counts)
    p = GC.rpn_inputs("all-tied")[0]
    assert all(len(np.unique(x)) == 1 for x in p)
    info = GC.rpn_inputs("small-split")[4]
    assert not np.array_equal(info[0], info[1])


def test_detection_cases_reach_their_limits():
    for name, (N, R, K, counts, per_im, det_cap, thr) in GC.DET_CASES.items():
        refs = [GC.det_reference(name, i) for i in range(N)]
        assert all(len(r[0]) <= det_cap for r in refs)
        if name == "r1000":
            assert per_im == det_cap and all(r[3] > per_im and len(r[0]) == per_im for r in refs)
        if name == "r2048":
            assert R == 2048 and refs[0][3] > per_im == len(refs[0][0]) < det_cap
        if name == "r65":
            assert counts[1] == 0 and len(refs[1][0]) == 0 < len(refs[0][0]) < det_cap
        if name == "r65-nothing":
            assert all(len(r[0]) == 0 for r in refs)
    # the post-filter removes rows in place
    for cross, pre in ((0.3, 0), (0.0, 2), (0.5, 1)):
        a = len(GC.det_reference("r65", 0)[0])
        b = len(GC.det_reference("r65", 0, nms_cross_class=cross, num_det_per_class_pre=pre)[0])
        assert 0 < b < a


def test_union_case_overflows_one_class():
    u = GC.UNION
    cand0, cand1 = GC.union_reference(0)[3], GC.union_reference(1)[3]
    assert u["cand_cap"] < cand0[0] <= u["big_cap"] and cand0[1] == 0  # class 1 over, class 2 empty
    assert 0 < cand1[0] <= u["cand_cap"] and cand1[1] == 0
    # the overflow happens in the second view: the first alone fits
    rois, cls, pred, counts = GC.union_inputs()
    first = int((cls[0, 0, :counts[0, 0], 1] >= 0.05).sum())
    assert 0 < first <= u["cand_cap"]
    assert u["hflip"][1] and u["ar"][1] is not None and u["K"] == 3 and u["F"] == 2


@pytest.mark.parametrize("H,W", GC.RLE_FRAMES)
def test_rle_cases_overflow_where_planned(H, W):
    for need, cap in (GC.rle_planes(H, W)[1:], GC.rle_masks(H, W)[3:]):
        assert need[0] <= cap and need[-1] > cap            # row 0 fits, the last overflows
        assert (need[1:-1] > cap).any() and (need == cap).any()
        assert need.min() == 1                              # an all-zero row: one run
    planes, need, cap = GC.rle_planes(H, W)
    assert need[2] == H * W                                  # the checkerboard
    assert planes[3].all() and need[3] == 2                 # all ones: [0, H * W]
    masks, boxes, ref, need, cap = GC.rle_masks(H, W)
    assert ref[1].sum() == 0 and ref[5].sum() == 1          # all-zero mask; the 1-pixel box
    assert boxes[:, 0].min() == 0 and boxes[:, 1].min() == 0 and boxes[:, 2].max() == W - 1 \
        and boxes[:, 3].max() == H - 1                      # boxes touch all four frame edges
    assert ref[:, H - 1, :].any() and ref[:, :, W - 1].any()  # pasted pixels reach the far edges


def test_rle_ragged_and_string_cases():
    need, cap = GC.rle_ragged()[4:]
    assert need[0] <= cap and need[-1] > cap and (need[1:-1] > cap).any() and (need == cap).any()
    rows = GC.RLE_STRING_ROWS
    assert any(len(r) == 0 for r in rows) and [2 ** 31 - 1] in [list(r) for r in rows]
    assert len(rows[0]) > 0 and len(rows[-1]) > 0


def test_mask_nms_cases():
    for n, H, W in GC.MASK_NMS_CASES:
        masks, dets, cls = GC.mask_nms_inputs(n, H, W)
        keep = orc.nms_with_mask_iou(dets, cls, masks, 0.5, 2)
        assert masks[-1, -1, -1] == 1
        assert len(keep) >= 1 and (n == 1 or len(keep) < n)
        if n == 9:
            unlimited = orc.nms_with_mask_iou(dets, cls, masks, 0.5, 99)
            assert (cls[unlimited] == 1).sum() > 2 == (cls[keep] == 1).sum()
    assert [W % 64 for _, _, W in GC.MASK_NMS_CASES] == [53, 2, 0]


# --------------------------------------------------------------------------- 3. VD_ERR_WORKSPACE
@pytest.fixture(scope="module")
def ws_statuses():
    """tests/guarded_capi.py in a child process that sees no device."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for k in GC.RPN_ENV:
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "tests.guarded_capi"], cwd=GC.ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("WS_STATUSES ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(lines[-1][len("WS_STATUSES "):])


@pytest.mark.parametrize("name", guarded_capi.ENTRY_NAMES)
def test_short_or_null_workspace_is_refused(ws_statuses, name):
    """workspace_bytes = size - 1, a null workspace of the full size and a null one of
    0 bytes: VD_ERR_WORKSPACE, checked before any launch (so this needs no device).
    vd_gemm_bias_act is not here: what it needs depends on the hipBLASLt plan of the
    shape, found on the device, and its workspace is the cached global the exact GEMM
    tests guard."""
    from vosdetectron_amd import _lib
    size, short, null, null0 = ws_statuses[name]
    assert size > 0
    assert (short, null, null0) == (_lib.VD_ERR_WORKSPACE,) * 3, (short, null, null0)


def test_guarded_alloc_serves_the_wrappers_own_tensors(arena, monkeypatch):
    """guarded_alloc: torch.empty / empty_like / zeros as vosdetectron_amd.ops sees them
    are carves (channels_last included), pre-filled; everything else is torch's."""
    from vosdetectron_amd import ops
    log = G.guarded_alloc(monkeypatch, arena, G.ONES)
    t = ops.torch
    a = t.empty((2, 3), dtype=torch.int32, device="cpu")
    b = t.empty((1, 4, 2, 3), dtype=torch.float32, device="cpu", memory_format=torch.channels_last)
    c = t.empty_like(b)
    z = t.zeros((5,), dtype=torch.float32, device="cpu")
    assert a.tolist() == [[-1] * 3] * 2 and bool(torch.isnan(b).all()) and not bool(z.any())
    for v in (b, c):
        assert v.shape == (1, 4, 2, 3) and v.is_contiguous(memory_format=torch.channels_last)
    assert len(log) == 4 and t.Tensor is torch.Tensor and t.float32 is torch.float32
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.nbytes
    assert all(lo <= v.data_ptr() < hi for v in (a, b, c, z))
    arena.check()
    c.flatten()  # a view of the arena like any other
    off = c.data_ptr() - lo
    arena.buf[off + c.numel() * 4] ^= 0xFF
    with pytest.raises(AssertionError, match="own tensor 2"):
        arena.check()
