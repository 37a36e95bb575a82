"""vd_mask_iou_nms_frames without a device: the test inputs exercise what the GPU
test claims (checked on the oracle alone), the workspace size function, and the C
entry's refusals."""
import ctypes

import numpy as np
import pytest

from tests import mask_nms_frames_ref as mr


@pytest.mark.parametrize("H,W,n", mr.CPU_SIZES)
def test_generator_gives_discards_survivors_cap_removals_and_ties(H, W, n):
    """On the oracle alone, for every seed and frame size in use: each frame the
    statistics were stated for -- the full ones, n and n - 5 detections; a frame of
    one detection can neither discard nor keep two -- has at least 2 rows discarded
    and at least 2 kept by the NMS at each threshold, loses at least one more row to
    the caps 1 and 2, and holds a score tie."""
    for seed in mr.SEEDS:
        masks, dets, classes, counts = mr.gen_step(seed, H, W, mr.step_counts(n))
        base, cnt = mr.frame_rows(counts, mr.CAP, len(masks))
        for f in (0, 2):
            k, b = int(cnt[f]), int(base[f])
            assert k == counts[f] >= 8
            s = dets[f, :k, 4]
            assert len(np.unique(s)) < k, ("no score tie", seed, f)
            for iou_th, mpc in mr.SETTINGS:
                if mpc == 0:
                    continue
                total, nms, capped = mr.frame_stats(masks[b:b + k], dets[f, :k], classes[f, :k],
                                                    H, W, iou_th, mpc)
                assert total - nms >= 2 and nms >= 2, (seed, f, iou_th, total, nms)
                if mpc <= 2:
                    assert capped < nms, (seed, f, iou_th, mpc, nms, capped)
                else:
                    assert capped == nms


def _bound(F, cap, rows, h, w):
    """The issue's bound: rows x ceil(im_w / 64 + 1) x im_h x 8 bytes of bit rows, an
    O(F cap^2) pair table (4-byte entries, a full square) and O(rows) + O(F) scalars
    (at most 32 bytes per row and per frame); each of the six arrays may round up to
    256 bytes."""
    bits = rows * int(np.ceil(w / 64 + 1)) * h * 8
    return bits + 4 * F * cap * cap + 32 * rows + 32 * F + 6 * 256


def test_workspace_size_function():
    from vosdetectron_amd import _lib
    size = _lib.lib().vd_mask_iou_nms_frames_workspace_size
    ok = (4, 32, 57, 70, 100)
    assert size(*ok) > 0
    for bad in ((0, 32, 57, 70, 100), (65536, 32, 57, 70, 100), (4, 0, 57, 70, 100),
                (4, 1025, 57, 70, 100), (4, 32, -1, 70, 100), (4, 32, 57, 0, 100),
                (4, 32, 57, 70, 0), (4, 32, 57, 65536, 65536)):
        assert size(*bad) == 0, bad
    # non-decreasing in each argument, and inside the bound
    steps = ((1, 2, 3, 16, 64), (1, 31, 32, 33, 256, 1024), (0, 1, 57, 128, 1600),
             (1, 37, 64, 70, 480, 800), (1, 45, 63, 64, 65, 100, 128, 129, 854, 1333))
    for arg, values in enumerate(steps):
        prev = 0
        for v in values:
            a = list(ok)
            a[arg] = v
            s = size(*a)
            assert s >= prev and s > 0, (arg, v, s, prev)
            assert s <= _bound(*a), (a, s, _bound(*a))
            prev = s
    # no term of rows x im_h x im_w bytes: the planes of this step alone are 656 MB
    big = (16, 256, 1600, 480, 854)
    assert size(*big) <= _bound(*big) < 1600 * 480 * 854 // 4
    assert size(64, 256, 6400, 800, 1333) < 1 << 30  # the largest benchmark shape fits the budget


def test_c_entry_refusals_without_a_device():
    """Every refusal comes before the first launch; the pointers are never followed."""
    from vosdetectron_amd import _lib
    L = _lib.lib()
    F, cap, rows, h, w = 3, 24, 31, 37, 83
    size = L.vd_mask_iou_nms_frames_workspace_size(F, cap, rows, h, w)
    assert size > 0
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(masks=p, rows=rows, R=28, dets=p, classes=p, counts=p, F=F, cap=cap, h=h, w=w,
             keep=p, keep_counts=p, valid=p, pd=p, pc=p, pn=p, pcap=cap, ws=p, wsb=size):
        return L.vd_mask_iou_nms_frames(masks, rows, R, dets, classes, counts, F, cap, h, w, 0.5,
                                        0.5, 1, keep, keep_counts, valid, pd, pc, pn, pcap, ws,
                                        wsb, None)

    for name in ("masks", "dets", "classes", "counts", "keep", "keep_counts", "ws"):
        assert call(**{name: None}) == _lib.VD_ERR_ARG, name
    for some in ({"pd": None}, {"pc": None}, {"pn": None}, {"pd": None, "pn": None}):
        assert call(**some) == _lib.VD_ERR_ARG, some  # all three record outputs or none
    assert call(rows=-1) == _lib.VD_ERR_ARG
    for kw in ({"cap": 1025}, {"cap": 0}, {"R": 63}, {"R": 0}, {"h": 0}, {"w": 0}, {"F": 65536},
               {"pcap": cap - 1}):
        assert call(**kw) == _lib.VD_ERR_SHAPE, kw
    assert call(wsb=size - 1) == _lib.VD_ERR_WORKSPACE
    assert call(wsb=0) == _lib.VD_ERR_WORKSPACE
    assert call(ws=p + 4) == _lib.VD_ERR_ARG  # not 16-byte aligned
    assert call(F=0) == _lib.VD_OK  # nothing to do, nothing launched
