"""The segm and VOS kernels inside guarded, poisoned buffers (tests/guarded.py; DESIGN
section 2, item 10): mask-IoU NMS, the RLE kernels at their capacity limit, mask
pasting, GroupNorm / ConvGRU on dirty statistics workspaces, and the tiled RoIAlign
workspace.  The properties are those of tests/test_guarded_box_gpu.py; for the
GroupNorm family the values are bounded (tests/gn_ref.py), and what is asserted bit for
bit is that the result does not depend on what the workspace held."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import gn_ref as gr
from tests import guarded as G
from tests import guarded_cases as GC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_t, _np, _stream, sweep, rows_equal = G.to_dev, G.to_np, G.stream, G.sweep, G.rows_equal


@pytest.fixture(scope="module")
def arena():
    return G.Arena(DEV, 160 << 20)


# --------------------------------------------------------------------------- mask-IoU NMS
def _mask_iou_nms(arena, masks, dets, cls, iou_th, per_class, ws_fill, out_fill):
    """vd_mask_iou_nms as ops.mask_iou_nms calls it."""
    from vosdetectron_amd._lib import check, lib
    n, H, W = masks.shape
    keep = arena.carve((max(n, 1),), torch.int64, out_fill, "vd_mask_iou_nms keep_out", key="keep")
    num = arena.carve((1,), torch.int32, out_fill, "vd_mask_iou_nms num_out", key="num")
    wsb = lib().vd_mask_iou_nms_workspace_size(n, H, W)
    ws = arena.carve((wsb,), torch.uint8, ws_fill, "vd_mask_iou_nms workspace (%d bytes)" % wsb,
                     key="ws", strip=wsb // n)
    pl, d, c = _t(masks), _t(dets), _t(cls)
    check(lib().vd_mask_iou_nms(pl.data_ptr(), n, H, W, d.data_ptr(), 5, c.data_ptr(),
                                float(iou_th), int(per_class), keep.data_ptr(), num.data_ptr(),
                                ws.data_ptr(), wsb, _stream()), "vd_mask_iou_nms")
    return keep, num


@pytest.mark.parametrize("n,H,W", GC.MASK_NMS_CASES)
def test_mask_iou_nms(arena, n, H, W):
    """Widths that are no multiple of 64 (the packed row's last word is partial); with
    n = 9 class 1 holds more survivors than max_per_class."""
    masks, dets, cls = GC.mask_nms_inputs(n, H, W)
    ref = orc.nms_with_mask_iou(dets, cls, masks, 0.5, 2)
    rng = np.random.default_rng(9)
    big = ((rng.uniform(0, 1, (n + 3, H, W)) < 0.5).astype(np.uint8),
           rng.uniform(0, 1, (n + 3, 5)).astype(np.float32), np.ones(n + 3, np.int32))

    def verify(res, out_fill, tag):
        keep, num = res
        assert int(num.item()) == len(ref), tag
        rows_equal(_np(keep[:len(ref)]), ref, tag)
        G.assert_prefill(keep[len(ref):], out_fill, "keep_out rows >= count, " + tag)

    sweep(arena, lambda w, o: _mask_iou_nms(arena, masks, dets, cls, 0.5, 2, w, o),
          lambda w, o: _mask_iou_nms(arena, *big, 0.5, 2, w, o), verify)


# --------------------------------------------------------------------------- RLE
def _verify_rle(counts, ncounts, refs, need, cap, out_fill, what):
    """Fitting rows complete and correct with their tail untouched; an overflowing row
    reports -need and leaves all its cap slots as pre-filled."""
    n = _np(ncounts)
    for i, want in enumerate(need):
        if want <= cap:
            assert n[i] == want, (what, i, n[i], want)
            rows_equal(_np(counts[i, :want]).astype(np.int64), np.asarray(refs[i], np.int64),
                       "%s row %d" % (what, i))
            G.assert_prefill(counts[i, want:], out_fill, "%s row %d past its counts" % (what, i))
        else:
            assert n[i] == -want, (what, i, n[i], -want)
            G.assert_prefill(counts[i], out_fill, "%s overflowing row %d" % (what, i))


def _roles(need, cap):
    """Row 0 fits, a middle row and the last row overflow, one row needs exactly cap."""
    assert need[0] <= cap and need[-1] > cap and (need[1:-1] > cap).any() and (need == cap).any()


def _mask_rle(arena, planes, cap, out_fill):
    from vosdetectron_amd._lib import check, lib
    M, H, W = planes.shape
    counts = arena.carve((M, cap), torch.int32, out_fill, "vd_mask_rle counts [M, cap]")
    n = arena.carve((M,), torch.int32, out_fill, "vd_mask_rle ncounts")
    check(lib().vd_mask_rle(planes.data_ptr(), M, H, W, counts.data_ptr(), cap, n.data_ptr(),
                            _stream()), "vd_mask_rle")
    return counts, n


@pytest.mark.parametrize("H,W", GC.RLE_FRAMES)
def test_mask_rle_at_capacity(arena, H, W):
    planes, need, cap = GC.rle_planes(H, W)
    _roles(need, cap)
    refs = [orc.rle_encode(p)[1] for p in planes]
    pt = _t(planes)
    for out_fill in G.FILLS:
        arena.reset()
        counts, n = _mask_rle(arena, pt, cap, out_fill)
        arena.check("vd_mask_rle %dx%d cap %d" % (H, W, cap))
        _verify_rle(counts, n, refs, need, cap, out_fill, "vd_mask_rle")


@pytest.mark.parametrize("H,W", GC.RLE_FRAMES)
def test_segm_rle_and_paste_at_capacity(arena, H, W):
    """vd_segm_rle on the 37 x 53 frame; the 24 x 9000 frame is wider than its column
    table: the entry refuses it (VD_ERR_SHAPE) without writing, and the planes path
    runs -- vd_paste_masks into a carve, vd_mask_rle on it."""
    from vosdetectron_amd import _lib, ops
    masks, boxes, ref, need, cap = GC.rle_masks(H, W)
    _roles(need, cap)
    refs = [orc.rle_encode(p)[1] for p in ref]
    mt, bt = _t(masks), _t(boxes)
    M = len(masks)
    for out_fill in G.FILLS:
        arena.reset()
        counts = arena.carve((M, cap), torch.int32, out_fill, "vd_segm_rle counts [M, cap]")
        n = arena.carve((M,), torch.int32, out_fill, "vd_segm_rle ncounts")
        st = _lib.lib().vd_segm_rle(mt.data_ptr(), M, GC.RLE_R, bt.data_ptr(), 5, H, W, 0.5,
                                    counts.data_ptr(), cap, n.data_ptr(), _stream())
        arena.check("vd_segm_rle %dx%d" % (H, W))
        if W <= 8192:
            _lib.check(st, "vd_segm_rle")
            _verify_rle(counts, n, refs, need, cap, out_fill, "vd_segm_rle")
        else:
            assert st == _lib.VD_ERR_SHAPE
            G.assert_prefill(counts, out_fill, "refused vd_segm_rle counts")
            G.assert_prefill(n, out_fill, "refused vd_segm_rle ncounts")
        planes = arena.carve((M, H, W), torch.uint8, out_fill, "vd_paste_masks out")
        assert ops.paste_masks(mt, bt, H, W, out=planes) is planes
        arena.check("vd_paste_masks %dx%d" % (H, W))
        rows_equal(_np(planes), ref, "vd_paste_masks")
        counts2, n2 = _mask_rle(arena, planes, cap, out_fill)
        arena.check("vd_mask_rle on the pasted planes")
        _verify_rle(counts2, n2, refs, need, cap, out_fill, "paste + vd_mask_rle")


def test_segm_rle_ragged_at_capacity(arena):
    from vosdetectron_amd._lib import check, lib
    masks, boxes, hw, ref, need, cap = GC.rle_ragged()
    _roles(need, cap)
    refs = [orc.rle_encode(p)[1] for p in ref]
    mt, bt, ht = _t(masks), _t(boxes), _t(hw)
    M = len(masks)
    for out_fill in G.FILLS:
        arena.reset()
        counts = arena.carve((M, cap), torch.int32, out_fill, "vd_segm_rle_ragged counts")
        n = arena.carve((M,), torch.int32, out_fill, "vd_segm_rle_ragged ncounts")
        check(lib().vd_segm_rle_ragged(mt.data_ptr(), M, GC.RLE_R, bt.data_ptr(), 5,
                                       ht.data_ptr(), 0.5, counts.data_ptr(), cap, n.data_ptr(),
                                       _stream()), "vd_segm_rle_ragged")
        arena.check("vd_segm_rle_ragged")
        _verify_rle(counts, n, refs, need, cap, out_fill, "vd_segm_rle_ragged")


def test_rle_strings_exact_chars(arena):
    """chars carved at exactly the total of lens; rows of 0 counts next to a row of one
    2^31 - 1 count; the first row overall and the last are checked like the rest."""
    from vosdetectron_amd._lib import check, lib
    rows = [np.asarray(r, np.int64) for r in GC.RLE_STRING_ROWS]
    want = [orc.rle_to_string(r) for r in rows]
    cap = max(len(r) for r in rows)
    M = len(rows)
    counts = np.zeros((M, cap), np.int32)
    for i, r in enumerate(rows):
        counts[i, :len(r)] = r
    n = np.array([len(r) for r in rows], np.int32)
    ct, nt = _t(counts), _t(n)
    for out_fill in G.FILLS:
        arena.reset()
        lens = arena.carve((M,), torch.int32, out_fill, "vd_rle_strings lens")
        check(lib().vd_rle_strings(ct.data_ptr(), nt.data_ptr(), M, cap, lens.data_ptr(), None,
                                   _stream()), "vd_rle_strings")
        arena.check("vd_rle_strings lengths")
        assert _np(lens).tolist() == [len(w) for w in want]
        total = sum(len(w) for w in want)
        chars = arena.carve((total,), torch.uint8, out_fill, "vd_rle_strings chars (exact total)")
        check(lib().vd_rle_strings(ct.data_ptr(), nt.data_ptr(), M, cap, lens.data_ptr(),
                                   chars.data_ptr(), _stream()), "vd_rle_strings")
        arena.check("vd_rle_strings chars")
        assert _np(chars).tobytes().decode("ascii") == "".join(want)


# --------------------------------------------------------------------------- GroupNorm / ConvGRU
FMT = {"nchw": torch.contiguous_format, "nhwc": torch.channels_last}
GN_SHAPES = ((2, 64, 5, 7), (1, 256, 8, 8))
GN_G = 32
# allowances for the device sigmoid / tanhf: twice the errors measured on an MI355X over
# [-8, 8] (8.8e-8, 4.5e-8), the constants tests/test_gn_kernels_gpu.py measures and uses
SIGMOID_S = 2 * 8.8e-8
TANH_T = 2 * 4.5e-8


def _affine(gen, C):
    """gamma in [-1.25, 1.25], beta in [-1, 1]: pre-activations stay inside [-8, 8]."""
    return torch.rand(C, generator=gen) * 2.5 - 1.25, torch.rand(C, generator=gen) * 2 - 1


def _gn_inputs(shape, batch=None):
    """Inputs as tests/gn_ref.gn_inputs builds them, at a shape of this file."""
    B, C, H, W = shape
    B = batch or B
    gen = torch.Generator().manual_seed(77 + C + H)
    r = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    d = {"x": r(B, C, H, W)}
    d["gamma"], d["beta"] = _affine(gen, C)
    d["x2"], d["res"] = r(B, C, H, W), r(B, C, H, W)
    if H % 2 == 0 and W % 2 == 0:
        d["res_up"] = r(B, C, H // 2, W // 2)
    d["res_g"] = r(B, C, H, W) * 2
    d["gamma_r"], d["beta_r"] = _affine(gen, C)
    return d


def _gru_inputs(shape, batch=None):
    B, C, H, W = shape
    B = batch or B
    gen = torch.Generator().manual_seed(91 + C + H)
    d = {k: torch.randn((B, C, H, W), generator=gen) for k in
         ("zx", "zh", "rx", "rh", "hx", "hh", "h")}
    d["z"] = torch.rand((B, C, H, W), generator=gen) * 0.998 + 0.001
    d["finer"] = torch.randn((B, C, 2 * H, 2 * W), generator=gen)
    for k in "zrh":
        d["gamma_" + k], d["beta_" + k] = _affine(gen, C)
    return d


def _epilogue_kwargs(kind, dd):
    """ops.group_norm_act keywords of an epilogue of tests/gn_ref.EPILOGUES."""
    return {"none": {}, "relu": {"act": "relu"},
            "sigmoid": {"act": "sigmoid", "x2": dd.get("x2")},
            "tanh": {"act": "tanh", "x2": dd.get("x2")},
            "res": {"act": "relu", "residual": dd.get("res")},
            "res_up": {"residual": dd.get("res_up"), "upsample_residual": True},
            "res_gn": {"act": "relu", "residual": dd.get("res_g"),
                       "residual_gn": (dd.get("gamma_r"), dd.get("beta_r"))}}[kind]


def _dev(t, layout):
    return t.to(DEV).contiguous(memory_format=FMT[layout]) if t.dim() == 4 else t.to(DEV)


def _fill_sweep(arena, monkeypatch, run_small, run_large, check_values, what):
    """run_small under workspace fills 0x00, 0xFF and the larger instance's leftover,
    times output prefills 0x00 and 0xFF.  Outputs the wrapper allocates itself are carves
    too (G.guarded_alloc).  Canaries intact, every result within its bound, and all six
    results the same bits: nothing depends on what workspace or output held."""
    results = []
    for out_fill in G.FILLS:
        for ws in G.WS_MODES:
            arena.reset()
            alloc = G.guarded_alloc(monkeypatch, arena, out_fill)
            if ws == "leftover":
                G.guarded_ws(monkeypatch, arena, G.ONES, reuse=True)
                run_large()
                arena.check(what + ": the larger instance")
                log = G.guarded_ws(monkeypatch, arena, G.KEEP, reuse=True)
                del alloc[:]
            else:
                log = G.guarded_ws(monkeypatch, arena, ws, reuse=True)
            outs = run_small()
            arena.check("%s, workspace %s, outputs 0x%02X" % (what, ws, out_fill))
            assert len(log) == 1 and len(alloc) == len(outs)
            assert all(o.data_ptr() == v.data_ptr() for o, v in zip(outs, alloc))
            check_values(outs)
            results.append([o.clone() for o in outs])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                what + ": the result depends on what the workspace or the output held"


def _within(out, ref, bound, what):
    err = (out.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), (what, float((err / bound).max()))


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_group_norm_workspace_fills(arena, monkeypatch, shape, layout):
    """vd_group_norm_act in every residual mode (mode 3 zeroes and uses two sets of
    statistics; the half-size residual needs the even map) and activation.  The output
    is the wrapper's own tensor, carved."""
    from vosdetectron_amd import ops
    d = _gn_inputs(shape)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    big = {k: _dev(v, layout) for k, v in _gn_inputs(shape, batch=shape[0] + 2).items()}
    for kind in gr.EPILOGUES:
        if kind == "res_up" and "res_up" not in d:
            continue
        ref, bound = gr.epilogue64(kind, d, GN_G, SIGMOID_S, TANH_T)[:2]

        def run(t):
            return [ops.group_norm_act(t["x"], GN_G, t["gamma"], t["beta"], gr.EPS,
                                       **_epilogue_kwargs(kind, t))]

        _fill_sweep(arena, monkeypatch, lambda: run(dd), lambda: run(big),
                    lambda outs: _within(outs[0], ref, bound, kind),
                    "group_norm_act %s %s" % (kind, layout))


@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_convgru_workspace_fills(arena, monkeypatch, shape, layout, state):
    """convgru_gates (two sets of statistics; z and h * r are the wrapper's own tensors,
    carved) and convgru_update with and without the state and the finer level."""
    from vosdetectron_amd import ops
    d = _gru_inputs(shape)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    big = {k: _dev(v, layout) for k, v in _gru_inputs(shape, batch=shape[0] + 2).items()}
    gates = gr.gates64(d, GN_G, SIGMOID_S, state=state)

    def run_gates(t):
        a = [t["zx"], t["rx"], t["h"], t["zh"], t["rh"]] if state else [t["zx"]] + [None] * 4
        z, hr = ops.convgru_gates(*a, GN_G, t["gamma_z"], t["beta_z"], t["gamma_r"],
                                  t["beta_r"], gr.EPS)
        return [z, hr] if state else [z]

    def check_gates(outs):
        _within(outs[0], *gates["z"], "z")
        if state:
            _within(outs[1], *gates["hr"], "hr")

    _fill_sweep(arena, monkeypatch, lambda: run_gates(dd), lambda: run_gates(big), check_gates,
                "convgru_gates %s state=%s" % (layout, state))

    for finer in (True, False):
        ref, bound = gr.update64(d, GN_G, TANH_T, state=state, finer=finer)[:2]

        def run_update(t):
            return [ops.convgru_update(t["hx"], t["hh"] if state else None, t["z"],
                                       t["h"] if state else None, GN_G, t["gamma_h"],
                                       t["beta_h"], finer=t["finer"] if finer else None,
                                       eps=gr.EPS)]

        _fill_sweep(arena, monkeypatch, lambda: run_update(dd), lambda: run_update(big),
                    lambda outs: _within(outs[0], ref, bound, "update"),
                    "convgru_update %s state=%s finer=%s" % (layout, state, finer))


# --------------------------------------------------------------------------- tiled RoIAlign
ROI_TILED = {"variant30": {}, "variant30-chunk16": {"VOSDET_RA_CHUNK": "16"}}
ROI_ENV = ("VOSDET_ROIALIGN_VARIANT", "VOSDET_RA_GENERAL", "VOSDET_RA_SEGS", "VOSDET_RA_PARTS",
           "VOSDET_RA_CHUNK")


def _roi_case(name):
    """(NHWC level maps, rois, levels, float64 reference, inputs) of a case of
    tests/roi_exact_ref.py on the device."""
    from tests import roi_exact_ref as R
    i = R.inputs(name)
    nhwc = [_t(np.ascontiguousarray(f.transpose(0, 2, 3, 1))) for f in i.feats]
    return nhwc, _t(np.array(i.rois)), _t(np.array(i.levels)), _t(np.array(R.reference(name))), i


@pytest.mark.parametrize("mode", list(ROI_TILED))
def test_tiled_roi_align_workspace(arena, monkeypatch, mode):
    """The variants that take a workspace (the tile-binned kernel, and with 16-row
    chunks) on the C = 64 case of tests/roi_exact_ref.py: the workspace carved at exactly
    vd_roi_align_fpn_tiled_workspace_size bytes and filled 0x00, 0xFF and with the
    leftover of the larger P = 14, C = 256 case, the output a carve pre-filled 0x00 and
    0xFF; equal to the float64 reference bit for bit."""
    from vosdetectron_amd import ops
    for k in ROI_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VOSDET_ROIALIGN_VARIANT", "30")
    for k, v in ROI_TILED[mode].items():
        monkeypatch.setenv(k, v)
    small_case, large_case = _roi_case("p7-c64-lanes-past-c"), _roi_case("p14-c256-mask-head")
    logs = []

    def run(case, w, o):
        nhwc, rois, lv, ref, i = case
        log = G.guarded_ws(monkeypatch, arena, w, reuse=True)
        out = arena.carve((len(i.rois), i.P, i.P, i.C), torch.float32, o, "roi_align_fpn out",
                          key="out")
        y = ops.roi_align_fpn(nhwc, list(i.scales), rois, lv, i.P, i.sr, out=out,
                              out_layout="nhwc")
        assert y is out and len(log) == 1 and log[0][1] > 0, log  # the tiled entry was sized
        logs.append(log[0])
        return out

    def verify(out, out_fill, tag):
        ref = small_case[3]
        got = out.permute(0, 3, 1, 2).double()
        assert tuple(got.shape) == tuple(ref.shape)
        assert torch.equal(got, ref), "%s: %d outputs differ from float64" % (
            tag, int((got != ref).sum()))

    sweep(arena, lambda w, o: run(small_case, w, o), lambda w, o: run(large_case, w, o), verify)
    pairs = [(a, b) for a, b in zip(logs, logs[1:]) if a[1] > b[1]]
    assert len(pairs) >= 2 and all(a[2] == b[2] for a, b in pairs), logs


# --------------------------------------------------------------------------- vd_gemm_bias_act
def test_gemm_bias_act_workspace_status(monkeypatch):
    """vd_gemm_bias_act's workspace check needs the device: it comes after the shape's
    hipBLASLt plan is found (launch_gemm_bias_act), and it is against the bytes THAT plan
    uses, of which vd_gemm_workspace_size() is only the upper bound the search may use.
    So for every shape planned here: the full workspace succeeds; a plan that uses p > 0
    bytes refuses p - 1 bytes and a null workspace with VD_ERR_WORKSPACE before it
    launches; a plan that uses none accepts both (size - 1 bytes of the upper bound is
    refused only by a plan that uses all of it).  The hand-written kernel is kept out
    (VOSDET_GEMM_MFMA=0) so that every shape goes through a hipBLASLt plan."""
    from vosdetectron_amd import _lib, ops
    monkeypatch.setenv("VOSDET_GEMM_MFMA", "0")
    L = _lib.lib()
    size = L.vd_gemm_workspace_size()
    assert size > 0
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    gen = torch.Generator().manual_seed(3)
    shapes = [(1003, 100, 72), (4096, 96, 2048), (37, 1000, 4096), (64, 24, 8192), (1, 32, 100)]
    seen = {}
    for M, N, K in shapes:
        a = torch.randn((M, K), generator=gen).to(DEV)
        w = (torch.randn((N, K), generator=gen) / K ** 0.5).to(DEV)
        b = torch.randn(N, generator=gen).to(DEV)
        out = torch.full((M, N), float("nan"), device=DEV)

        def call(p, n):
            return L.vd_gemm_bias_act(a.data_ptr(), M, K, w.data_ptr(), N, b.data_ptr(), None, 0,
                                      out.data_ptr(), p, n, _stream())

        assert call(ws.data_ptr(), size) == _lib.VD_OK
        torch.cuda.synchronize()
        want = a.double() @ w.double().t() + b.double()
        assert bool(((out.double() - want).abs() <= 1e-3 * (1 + want.abs())).all())
        plan = [r for r in ops.gemm_plan_list() if r[:5] == (M, N, K, 0, 0)]
        assert len(plan) == 1, plan
        need = plan[0][6]
        seen[(M, N, K)] = need
        assert 0 <= need <= size
        if need > 0:
            assert call(ws.data_ptr(), need - 1) == _lib.VD_ERR_WORKSPACE
            assert call(None, size) == _lib.VD_ERR_WORKSPACE
            assert call(ws.data_ptr(), need) == _lib.VD_OK
        else:
            assert call(None, 0) == _lib.VD_OK
        torch.cuda.synchronize()
    print("GEMM_PLAN_WORKSPACE " + repr(seen))
