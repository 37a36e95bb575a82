"""The F(4x4) Winograd block plan on the device (csrc/conv3x3_wino4.hip): the tall
32 x 16 output block and the tile-aligned 2-D stack (g maps per stack row) give the
bits of today's layout (VOSDET_WINO4_PLAN=0: the wide 16 x 32 block, one map per stack
row) -- every tile keeps its offset inside its map, so each output goes through the same
arithmetic in the same order.  The shapes are the smallest at which the addressing can
go wrong: a row / column past a block, a half-empty last stack row, two channel blocks,
a full and a one-column separator, maps of one tile, grouped input."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _with_plan(plan, fn):
    old = os.environ.get("VOSDET_WINO4_PLAN")
    if plan is None:
        os.environ.pop("VOSDET_WINO4_PLAN", None)
    else:
        os.environ["VOSDET_WINO4_PLAN"] = plan
    try:
        y = fn()
        torch.cuda.synchronize()
        return y
    finally:
        if old is None:
            os.environ.pop("VOSDET_WINO4_PLAN", None)
        else:
            os.environ["VOSDET_WINO4_PLAN"] = old


def _case(N, C, H, W, Co, groups=1):
    from vosdetectron_amd import ops
    g = torch.Generator(device="cuda").manual_seed(N * 131 + C + 7 * H + W)
    x = torch.randn(N, C, H, W, device="cuda", generator=g).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(Co, C // groups, 3, 3, device="cuda", generator=g) / (3. * (C // groups) ** .5)
    b = torch.randn(Co, device="cuda", generator=g)
    u = ops.conv3x3_wino4_grouped_weight(w, groups) if groups > 1 else ops.conv3x3_wino4_weight(w)
    assert u is not None
    return x, u, b


def _check(x, u, b, plans, mosaics=("rows",), groups=1):
    """Every plan == VOSDET_WINO4_PLAN=0 of the same entry, bit for bit, with ReLU on and
    off and bias present and absent; outputs outside the maps' stores do not exist (the
    output tensor is exactly the maps), so equality covers the unstored separators too."""
    from vosdetectron_amd import ops
    for mosaic in mosaics:
        for relu in (True, False):
            for bias in (b, None):
                run = lambda: ops.conv3x3_wino4_bias_act(x, u, bias, relu=relu, mosaic=mosaic,
                                                         groups=groups)
                ref = _with_plan("0", run)
                assert ref is not None
                for plan in plans:
                    y = _with_plan(plan, run)
                    assert y is not None
                    assert torch.equal(ref, y), (mosaic, relu, bias is not None, plan,
                                                 float((ref - y).abs().max()))


def test_one_past_a_block_both_shapes():
    # 33 x 17: one row past the tall block and two 16-row blocks + 1, one column past 16
    x, u, b = _case(1, 24, 33, 17, 64)
    _check(x, u, b, ["tall,1", "wide,1"], mosaics=(False, "rows"))


def test_stack_25x42():
    x, u, b = _case(3, 16, 25, 42, 64)
    # wide g 2: the last stack row holds one map and an empty cell
    _check(x, u, b, ["tall,1", "wide,2", "wide,3"])


def test_two_channel_blocks_every_g():
    x, u, b = _case(5, 8, 9, 11, 128)
    _check(x, u, b, ["%s,%d" % (s, g) for s in ("wide", "tall") for g in range(1, 6)])


@pytest.mark.parametrize("S", [16, 15])
def test_separator_widths(S):
    # 16 x 16: pitch 20, a full 4-column separator; 15 x 15: pitch 16, a single column
    x, u, b = _case(4, 16, S, S, 64)
    _check(x, u, b, ["wide,2", "wide,4", "tall,2", "tall,3", "tall,4"])


def test_one_tile_maps():
    x, u, b = _case(7, 8, 4, 4, 64)
    _check(x, u, b, ["wide,1", "wide,3", "wide,7", "tall,1", "tall,2", "tall,7"])


def test_grouped_rows_entry():
    x, u, b = _case(2, 64, 50, 84, 64, groups=8)
    _check(x, u, b, ["tall,1", "tall,2", "wide,2"], groups=8)


def test_automatic_plan_p2():
    """Unset: the planner's own choice (200 x 336 stacks best in the tall block)."""
    from vosdetectron_amd import ops
    assert _with_plan(None, lambda: ops.conv3x3_wino4_plan(2, 200, 336, 8, 64, True, 256))[:3] \
        == ("tall", 1, 273)
    x, u, b = _case(2, 8, 200, 336, 64)
    run = lambda: ops.conv3x3_wino4_bias_act(x, u, b, relu=True, mosaic="rows")
    ref = _with_plan("0", run)
    y = _with_plan(None, run)
    assert torch.equal(ref, y), float((ref - y).abs().max())
    y = _with_plan(None, lambda: ops.conv3x3_wino4_bias_act(x, u, b, relu=True))
    assert torch.equal(ref, y), float((ref - y).abs().max())


def test_planned_launch_graph_replay():
    """A captured planned launch replays the grid it was captured with."""
    from vosdetectron_amd import ops
    x, u, b = _case(3, 16, 25, 42, 64)
    run = lambda: ops.conv3x3_wino4_bias_act(x, u, b, relu=True, mosaic="rows")
    ref = _with_plan("0", run)
    eager = _with_plan("tall,2", run)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()

    def capture():
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                return run()
    out = _with_plan("tall,2", capture)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert torch.equal(eager, ref)
