"""The F(4x4) Winograd block plan (vd_conv3x3_wino4_plan, csrc/conv3x3_wino4.hip): which
output block (wide 16 x 32 or tall 32 x 16 pixels) and how many maps g per stack row a
launch uses.  Host code only: checked against a brute-force restatement of the rule
(fewest rounds of workgroups over the CUs, then fewest blocks, then today's layout
wide / g = 1, then the earlier candidate in the order wide 1.., tall 1..), the plans of
the benched shapes pinned, and the VOSDET_WINO4_PLAN switch."""
import numpy as np
import pytest


def _plan(N, H, W, Cout, stacked, n_cu=256, C=64):
    from vosdetectron_amd import ops
    return ops.conv3x3_wino4_plan(N, H, W, C, Cout, stacked, n_cu)


def _brute(N, H, W, Cout, stacked, n_cu):
    """(shape, g, blocks, rounds) by listing every candidate."""
    ncb = Cout // 64
    hp, wp = -(-(H + 1) // 4) * 4, -(-(W + 1) // 4) * 4
    g = np.arange(1, (min(N, 64) if stacked else 1) + 1, dtype=np.int64)
    cands = []
    for shape, (bh, bw) in (("wide", (16, 32)), ("tall", (32, 16))):
        if stacked:
            rows, cols = -(-N // g) * hp, (g - 1) * wp + W
            blocks = -(-rows // bh) * -(-cols // bw)
        else:
            blocks = np.full(1, N * -(-H // bh) * -(-W // bw), dtype=np.int64)
        rounds = -(-(blocks * ncb) // n_cu)
        cands += [(int(r), int(b), i, shape, int(c))
                  for i, (r, b, c) in enumerate(zip(rounds, blocks, g), len(cands))]
    r, b, _, shape, c = min(cands)  # index i: the first of equals, wide g = 1 first of all
    return shape, c, b, r


def test_plan_matches_brute_force():
    Ns = [1, 2, 3, 5, 8, 16, 33, 64, 70]
    Hs = sorted(set(range(1, 341, 13)) | {4, 15, 16, 25, 50, 100, 200, 340})
    Ws = sorted(set(range(1, 341, 17)) | {4, 15, 16, 42, 84, 168, 336, 340})
    n = 0
    for N in Ns:
        for H in Hs:
            for W in Ws:
                for Cout in (64, 256, 512):
                    for stacked in (False, True):
                        n_cu = 256 if (N + H + W) % 3 else 104
                        got = _plan(N, H, W, Cout, stacked, n_cu)
                        assert got == _brute(N, H, W, Cout, stacked, n_cu), \
                            (N, H, W, Cout, stacked, n_cu, got)
                        n += 1
    assert n > 30000


@pytest.mark.parametrize("H,W,shape,g,blocks,today", [
    (200, 336, "tall", 1, 8568, 8976), (100, 168, "wide", 8, 2236, 2496),
    (50, 84, "wide", 4, 572, 624), (25, 42, "wide", 8, 154, 224)])
def test_plan_of_benched_shapes(H, W, shape, g, blocks, today, monkeypatch):
    """64 frames on 256 CUs, the stacked entry (the FPN / RPN convs' 256 channels)."""
    monkeypatch.delenv("VOSDET_WINO4_PLAN", raising=False)
    got = _plan(64, H, W, 256, True)
    assert got == (shape, g, blocks, -(-blocks * 4 // 256)), got
    monkeypatch.setenv("VOSDET_WINO4_PLAN", "0")
    assert _plan(64, H, W, 256, True) == ("wide", 1, today, -(-today * 4 // 256))


def test_plan_ties_keep_todays_layout(monkeypatch):
    monkeypatch.delenv("VOSDET_WINO4_PLAN", raising=False)
    # 16 frames of 120 x 216: 124 x 7 wide blocks = 62 x 14 tall ones
    assert _plan(16, 120, 216, 256, True) == ("wide", 1, 868, 14)
    monkeypatch.setenv("VOSDET_WINO4_PLAN", "tall,1")
    assert _plan(16, 120, 216, 256, True) == ("tall", 1, 868, 14)
    monkeypatch.delenv("VOSDET_WINO4_PLAN")
    # the plain entry: 32 x 32 is 2 x 1 wide blocks or 1 x 2 tall ones
    assert _plan(3, 32, 32, 64, False) == ("wide", 1, 6, 1)
    assert _plan(3, 32, 16, 64, False) == ("tall", 1, 3, 1)


def test_plan_switch(monkeypatch):
    monkeypatch.setenv("VOSDET_WINO4_PLAN", "0")
    assert _plan(64, 25, 42, 512, True) == ("wide", 1, 224, 7)
    assert _plan(64, 200, 336, 64, False) == ("wide", 1, 64 * 13 * 11, -(-64 * 13 * 11 // 256))
    monkeypatch.setenv("VOSDET_WINO4_PLAN", "tall,3")
    # 22 stack rows of 28 = 616 rows = 20 blocks; 2 x 44 + 42 = 130 columns = 9 blocks
    assert _plan(64, 25, 42, 512, True) == ("tall", 3, 180, -(-180 * 8 // 256))
    assert _plan(2, 25, 42, 512, True)[:2] == ("tall", 2)  # g clamped to N
    assert _plan(64, 25, 42, 512, False)[:3] == ("tall", 1, 64 * 1 * 3)  # plain: shape only
    monkeypatch.setenv("VOSDET_WINO4_PLAN", "wide,2")
    assert _plan(64, 25, 42, 512, True) == ("wide", 2, 56 * 3, -(-56 * 3 * 8 // 256))
    monkeypatch.setenv("VOSDET_WINO4_PLAN", "wide")
    assert _plan(64, 25, 42, 512, True)[:2] == ("wide", 1)
    for bad in ("1", "tall,0", "tall,x", "high,2", "wide2"):
        monkeypatch.setenv("VOSDET_WINO4_PLAN", bad)
        with pytest.raises(RuntimeError):
            _plan(64, 25, 42, 512, True)


def test_plan_refuses_unserved_shapes(monkeypatch):
    monkeypatch.delenv("VOSDET_WINO4_PLAN", raising=False)
    with pytest.raises(RuntimeError):
        _plan(4, 25, 42, 96, True)       # Cout not a multiple of 64
    with pytest.raises(RuntimeError):
        _plan(0, 25, 42, 64, True)
