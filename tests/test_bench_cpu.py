"""bench.py's measurement arithmetic on the CPU (no GPU): the SURVEY 8(d) step
roofline, the RoIAlign algorithmic-byte formula and the CPU-share probe."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_step_roofline_sums_stage_bounds():
    r = bench.step_roofline(528e9, 100, 16, 72.0, {"algorithmic_bytes_per_launch": 2.0e9},
                            (800, 1333), (800, 1344))
    mfma_ms = 528e9 * 16 / 157.3e12 * 1e3
    blob = 16 * (800 * 1333 * 3 + 3 * 4 * 800 * 1344)
    hbm_ms = (blob + 2.0e9) / 8e12 * 1e3
    assert abs(r["mfma_bound_ms"] - round(mfma_ms, 3)) < 1e-6
    assert abs(r["hbm_bound_ms"] - round(hbm_ms, 3)) < 1e-6
    assert abs(r["frac"] - round((mfma_ms + hbm_ms) / 72.0, 4)) < 1e-9
    assert r["frac"] < 1.0
    # executed work: the Winograd convolutions' share at 1/2.25 of its direct FLOPs
    r2 = bench.step_roofline(528e9, 100, 16, 72.0, {"algorithmic_bytes_per_launch": 2.0e9},
                             (800, 1333), (800, 1344), wino_flops_frame=300e9)
    ex = (528e9 - 300e9 * (1 - 1 / 2.25)) * 16 / 157.3e12 * 1e3
    assert abs(r2["mfma_bound_ms"] - round(ex, 3)) < 1e-6
    assert r2["frac"] < r["frac"]
    # F(4x4) convolutions at 1/4 of theirs
    r3 = bench.step_roofline(528e9, 100, 16, 72.0, {"algorithmic_bytes_per_launch": 2.0e9},
                             (800, 1333), (800, 1344), wino_flops_frame=100e9,
                             wino4_flops_frame=200e9)
    ex = (528e9 - 100e9 * (1 - 1 / 2.25) - 200e9 * 0.75) * 16 / 157.3e12 * 1e3
    assert abs(r3["mfma_bound_ms"] - round(ex, 3)) < 1e-6


def _fracs(d, path=""):
    """Every (path, value) whose key is 'frac' or starts with 'frac' in a nested line."""
    out = []
    if isinstance(d, dict):
        for k, v in d.items():
            if isinstance(v, (dict, list)):
                out += _fracs(v, path + "." + k)
            elif k.startswith("frac") and isinstance(v, (int, float)):
                out.append((path + "." + k, v))
    elif isinstance(d, list):
        for i, v in enumerate(d):
            out += _fracs(v, "%s[%d]" % (path, i))
    return out


def test_no_fraction_above_one():
    """a step 1.5x faster than the direct-conv FLOPs allow at
    the peak (Winograd) must still report frac <= 1 -- the direct-form figure is a
    rate (direct_conv_equivalent.TFs), never a fraction."""
    ms = 528e9 * 16 / 157.3e12 * 1e3 / 1.5  # 1.5x the direct-form bound
    r = bench.step_roofline(528e9, 100, 16, ms, {"algorithmic_bytes_per_launch": 1e9},
                            (800, 1333), (800, 1344), wino_flops_frame=330e9)
    assert r["direct_conv_equivalent"]["TFs"] > bench.MFMA_FP32_PEAK_TFS
    fr = _fracs(r)
    assert fr and all(v <= 1.0 for _, v in fr), fr
    # the committed bench line of this round obeys the same rule
    import glob
    import json
    for p in sorted(glob.glob(os.path.join(bench.ROOT, "profiles", "r04", "bench_default*.json"))):
        line = json.load(open(p))
        bad = [(k, v) for k, v in _fracs(line) if v > 1.0]
        assert not bad, (p, bad)


def test_winograd_flop_classifier():
    """bench._WinoFlops counts exactly the 3x3 / stride-1 / pad-1 convolutions
    the engine routes to Winograd (modeling.conv3x3_route on the 16-frame batch:
    Cout % 64 == 0, Cin % 8 == 0, and >= 2^12 batch output pixels in blocks >= 60 %
    real output, or below 2^18 pixels, where the alternative is MIOpen)."""
    import torch
    import torch.nn.functional as F
    x = torch.randn(1, 8, 64, 64)
    with bench._WinoFlops(frames=16) as wf:
        F.conv2d(x, torch.randn(64, 8, 3, 3), None, 1, 1)        # counted: 16*4096 px
        F.conv2d(x, torch.randn(64, 8, 3, 3), None, 2, 1)        # stride 2
        F.conv2d(x, torch.randn(32, 8, 3, 3), None, 1, 1)        # Cout 32
        F.conv2d(x, torch.randn(64, 8, 1, 1))                    # 1x1
        F.conv2d(x[:, :, :8, :8], torch.randn(64, 8, 3, 3), padding=1)  # 16*64 px
        # 16 x 16 maps: 16 * 256 = 2^12 batch pixels in full 8 x 16 blocks -> Winograd
        F.conv2d(x[:, :, :16, :16], torch.randn(64, 8, 3, 3), padding=1)
    assert wf.flops == 2 * 4096 * 64 * 8 * 9 + 2 * 256 * 64 * 8 * 9 + 2 * 64 * 64 * 8 * 9


def test_roi_align_algorithmic_bytes_counts_union_once():
    # two identical RoIs on level 0 (P2): the footprint is counted once, outputs twice
    rois = np.array([[0, 8, 8, 40, 40], [0, 8, 8, 40, 40]], np.float32)
    lv = np.zeros(2, np.int32)
    C, P = 4, 7
    got = bench.roi_align_algorithmic_bytes(rois, lv, [(200, 336), (1, 1), (1, 1), (1, 1)], C, P)
    # scale 1/4: [2, 10] x [2, 10] -> rows/cols floor(2)..floor(10)+1 = 2..11 inclusive
    touched = 10 * 10
    assert got == 4 * C * touched + 2 * 4 * C * P * P + 2 * 20


def test_winograd4_route_gate():
    """modeling.conv3x3_route sends a 3x3 to Winograd F(4x4) where the launch has
    >= 1024 16 x 32 x 64 workgroups (4 per CU) and its blocks are >= 50 % real
    output: at the benched 32 frames P2-P4 and res2-res5 conv2; not P5 / P6, the
    mask head's 14 x 14 RoI maps (38 %) or a 1-frame P2 (572 workgroups);
    VOSDET_WINO4=0 turns it off.  Counted by bench._WinoFlops at 1/4 of the
    direct form."""
    import torch
    import torch.nn.functional as F
    from vosdetectron_amd import modeling
    r = modeling.conv3x3_route
    for args in [(32, 256, 256, 192, 320), (32, 64, 64, 192, 320)]:
        assert r(*args) == ("wino4", None), args  # blocks already full: no stack
    # P3 / P4-sized maps: the row stack wastes less of the 16-row blocks (84 vs 78 / 68 %;
    # res5 59 vs 51 % at 896 workgroups)
    for args in [(32, 256, 256, 100, 168), (32, 256, 256, 50, 84), (32, 128, 128, 100, 168),
                 (32, 512, 512, 25, 42), (32, 256, 256, 200, 336), (32, 64, 64, 200, 336)]:
        assert r(*args) == ("wino4", "rows"), args
    assert abs(modeling._wino4_rows_use(32, 50, 84) - 32 * 50 * 84 / (104 * 16 * 96)) < 1e-12
    for args in [(32, 256, 256, 25, 42), (32, 256, 256, 13, 21), (1000, 512, 512, 7, 7),
                 (1, 256, 256, 200, 336), (32, 256, 96, 200, 336), (100, 256, 256, 14, 14)]:
        assert r(*args)[0] != "wino4", args
    # the mask head's RoI maps: F(4x4) on the shared-separator grid (>= 1024 pair
    # workgroups, maps >= half
    # a 16 x 16 cell); VOSDET_WINO4_MOSAIC=0 keeps the F(2x2) 2-D mosaic
    assert r(3200, 256, 256, 14, 14) == ("wino4", "grid")
    assert r(1600, 256, 256, 14, 14) == ("wino4", "grid")
    assert r(3200, 256, 256, 14, 14, mosaic=False)[0] != "wino4"
    # C4's res5 head: 7 x 7 maps eight per block (8 x 8 cells, 77 % real)
    assert r(8000, 512, 512, 7, 7) == ("wino4", "pair")
    assert abs(modeling._wino4_block_use(25, 42) - 1050 / 2048) < 1e-12
    old = os.environ.get("VOSDET_WINO4")
    try:
        os.environ["VOSDET_WINO4"] = "0"
        assert r(32, 256, 256, 200, 336) == ("wino", False)
    finally:
        if old is None:
            os.environ.pop("VOSDET_WINO4", None)
        else:
            os.environ["VOSDET_WINO4"] = old
    # the recorded decisions (tests/golden/conv3x3_routes.json, tools/gen_goldens.py
    # conv3x3_routes): the whole shape grid with no switch set, a subsample per switch
    import itertools
    import json
    with open(os.path.join(os.path.dirname(__file__), "golden", "conv3x3_routes.json")) as f:
        tab = json.load(f)
    flags = [tuple(fl) for fl in tab["flags"]]
    route_calls = [(n, ci, co, h, w, mos, w4) for n, (h, w), (ci, co), (mos, w4)
                   in itertools.product(tab["N"], tab["HW"], tab["C"], flags)]
    grouped_calls = [(n, ci, co, h, w, g) for n, (h, w), (ci, co), g
                     in itertools.product(tab["N"], tab["HW"], tab["C"], tab["groups"])]
    pick_calls = [(n, h, w, allow) for n, (h, w), allow
                  in itertools.product(tab["N"], tab["HW"], (True, False))]
    assert len(route_calls) == 5280 and len(tab["sets"]) == 10
    switches = sorted({k for s in tab["sets"] for k in s["env"]})
    saved = {k: os.environ.pop(k) for k in switches if k in os.environ}
    try:
        for s in tab["sets"]:
            os.environ.update(s["env"])
            ri = s["route_idx"] if s["route_idx"] is not None else range(len(route_calls))
            gi = s["grouped_idx"] if s["grouped_idx"] is not None else range(len(grouped_calls))
            assert len(ri) == len(s["route"]) and len(gi) == len(s["grouped"])
            for i, c in zip(ri, s["route"]):
                got, want = r(*route_calls[i]), tab["route_codes"][c]
                # `is`: a layout of False (one map per launch) is not 0 and not None
                assert got[0] == want[0] and (got[1] is want[1] or (
                    isinstance(want[1], str) and got[1] == want[1])), (s["env"], route_calls[i], got)
            for i, c in zip(gi, s["grouped"]):
                got, want = modeling.conv3x3_grouped_route(*grouped_calls[i]), tab["grouped_codes"][c]
                assert got is want or (isinstance(want, str) and got == want), \
                    (s["env"], grouped_calls[i], got)
            for c, want in zip(pick_calls, s["pick_mosaic"]):
                got = modeling._pick_mosaic(*c)
                assert (got[0] is want[0] or (isinstance(want[0], str) and got[0] == want[0])) \
                    and got[1] == want[1], (s["env"], c, got)
            for k in s["env"]:
                del os.environ[k]
    finally:
        for k in switches:
            os.environ.pop(k, None)
        os.environ.update(saved)
    x = torch.randn(1, 64, 50, 84)
    with bench._WinoFlops(frames=32) as wf:
        F.conv2d(x, torch.randn(256, 64, 3, 3), None, 1, 1)  # 32 x 4 x 3 x 4 WGs: F(4x4)
        F.conv2d(x[:, :, :25, :42], torch.randn(256, 64, 3, 3), None, 1, 1)  # 512: F(2x2)
    assert wf.flops4 == 2 * 50 * 84 * 256 * 64 * 9
    assert wf.flops == 2 * 25 * 42 * 256 * 64 * 9


def test_cpu_share_is_positive():
    n, caps = bench.cpu_share()
    assert n >= 1 and "affinity" in caps


def test_winograd_block_occupancy_gate():
    """modeling._conv3x3_mfma sends a 3x3 conv to Winograd only where its pixel
    blocks (8 x 16 for maps <= 16 wide, else 4 x 32) are >= 60 % real work: the C4
    head's 7 x 7 RoI maps (38 %) stay on the implicit GEMM, the mask head's 14 x 14
    maps (77 %) and the FPN levels go to Winograd."""
    from vosdetectron_amd.modeling import _WINO_MIN_BLOCK_USE, _wino_block_use
    assert _wino_block_use(7, 7) < _WINO_MIN_BLOCK_USE
    for hw in [(14, 14), (200, 336), (100, 168), (50, 84), (120, 214), (60, 107)]:
        assert _wino_block_use(*hw) >= _WINO_MIN_BLOCK_USE, hw
    assert abs(_wino_block_use(14, 14) - 196 / 256) < 1e-12
    assert _wino_block_use(8, 32) == 1.0
    # res5 / P5 25 x 42 maps: the 8 x 16 blocks (68 %) beat 4 x 32 (59 %)
    assert abs(_wino_block_use(25, 42) - 25 * 42 / (32 * 48)) < 1e-12


def test_winograd_mosaic_choice():
    """modeling._pick_mosaic: a batch runs per image when its blocks are already
    full (P2 200 x 336), else as the 2-D mosaic, whose use counts the phantom
    row / column of an odd side as waste: C4's 7 x 7 RoI maps 49 / 64 (over the
    0.6 gate), res5 25 x 42 maps 16 * 1050 / (52 * 352), the mask head's 14 x 14
    maps and the P3 / P4 batches 100 %; one map never mosaics; VOSDET_WINO_MOSAIC=1
    allows the one-column form only (even H), 0 none."""
    import os
    from vosdetectron_amd.modeling import _WINO_MIN_BLOCK_USE, _pick_mosaic
    assert _pick_mosaic(16, 200, 336) == (False, 1.0)
    m, u = _pick_mosaic(8000, 7, 7)
    assert m == "2d" and abs(u - 49 / 64) < 1e-12 and u >= _WINO_MIN_BLOCK_USE
    m, u = _pick_mosaic(16, 25, 42)
    assert m == "2d" and abs(u - 16 * 25 * 42 / (52 * 352)) < 1e-12  # 4 x 32 blocks
    for shape in [(1600, 14, 14), (16, 100, 168), (16, 50, 84)]:
        assert _pick_mosaic(*shape) == ("2d", 1.0), shape
    assert _pick_mosaic(1, 7, 7)[0] is False
    old = os.environ.get("VOSDET_WINO_MOSAIC")
    try:
        os.environ["VOSDET_WINO_MOSAIC"] = "1"
        assert _pick_mosaic(1600, 14, 14)[0] is True
        assert _pick_mosaic(8000, 7, 7)[0] is False
        os.environ["VOSDET_WINO_MOSAIC"] = "0"
        assert _pick_mosaic(1600, 14, 14)[0] is False
    finally:
        if old is None:
            os.environ.pop("VOSDET_WINO_MOSAIC", None)
        else:
            os.environ["VOSDET_WINO_MOSAIC"] = old


def test_bench_engines_accept_the_step_calls():
    """Weak r3 #9: bench.make_pipeline builds the engine each BASELINE config is
    timed on (C4 configs[0], FPN configs[1], VOS configs[3]) on CPU, and every
    call the timed step makes binds against that engine's signature (the round-3
    `VOSPipeline.run() got an unexpected keyword argument 'sync'` cost a GPU run)."""
    import inspect
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.weights import build_model
    for name in ("e2e_mask_rcnn_R-50-C4_1x", "e2e_mask_rcnn_R-50-FPN_1x",
                 "vos_R-101-FPN_3x_gn_dynamic_davis"):
        cfg = vcfg.get(name)
        model, _ = build_model(cfg, device="cpu", fold=False)
        pipe, fh, fw = bench.make_pipeline(cfg, model, 2, "nchw", "cpu")
        vos = bool(cfg.get("VOS", False))
        assert (fh, fw) == ((480, 854) if vos else (800, 1333)), name
        assert type(pipe).__name__ == ("VOSPipeline" if vos else "C4FramePipeline"
                                       if not cfg.FPN.FPN_ON else "FramePipeline"), name
        for fn, args, kw in bench.step_calls(pipe, vos):
            inspect.signature(fn).bind(*args, **kw)  # raises TypeError on a drift


def test_winograd_input_channel_limit():
    """The Winograd kernel's zero lanes read a 4096-float zero buffer at the chunk's
    channel offset (csrc/conv3x3_wino.hip), so conv3x3_route keeps a conv with more
    input channels off it (the implicit GEMM or MIOpen / CK take it)."""
    from vosdetectron_amd import modeling, ops
    assert ops.WINO_MAX_CIN == 4096
    assert modeling.conv3x3_route(16, 4096, 256, 200, 336)[0] == "wino4"
    assert modeling.conv3x3_route(1, 4096, 256, 200, 336)[0] == "wino"
    for n in (1, 16):
        assert modeling.conv3x3_route(n, 4104, 256, 200, 336)[0] not in ("wino", "wino4")


class _FakePipe:
    """An ASYNC engine stand-in: run() queues, complete() is the host read."""
    ASYNC = True

    def __init__(self, events):
        self.events = events

    def run(self, frames, sync=True):
        self.events.append(("run", int(frames[0])))
        return {"frame": int(frames[0])}

    def complete(self, out):
        if "counts_host" not in out:
            self.events.append(("complete", out["frame"]))
            out["counts_host"] = [1]
        return out


def test_timed_region_includes_last_complete():
    """the last timed step's complete() (the counts read and
    any overflow batch) runs inside the timed region, before the clock stops."""
    import torch
    events = []
    pipe = _FakePipe(events)
    frames = [torch.tensor([i]) for i in range(4)]
    loop = bench.StepLoop(pipe, None, None, resident=frames)
    clock_calls = []

    def clock():
        events.append(("clock",))
        clock_calls.append(len(events))
        return float(len(clock_calls))

    dt, out = bench.timed_region(loop, 3, lambda: events.append(("sync",)), clock=clock)
    t0, t1 = events.index(("clock",)), len(events) - 1 - events[::-1].index(("clock",))
    inside = events[t0:t1]
    assert [e for e in inside if e[0] == "run"] == [("run", 0), ("run", 1), ("run", 2)]
    # every step's host read, the last one included, happens between the clocks
    assert [e for e in inside if e[0] == "complete"] == [("complete", 0), ("complete", 1),
                                                         ("complete", 2)]
    assert inside.index(("complete", 2)) < len(inside) and out["frame"] == 2
    assert ("sync",) in events[t0:t1] and dt == 1.0


def test_step_loop_gathers_each_step_once():
    """StepLoop with a collective: one gather per step, at most one in flight,
    each drained (on_gathered) before the next is issued, the last by finish()."""
    import torch
    events = []

    class G:
        collective = True

        def gather_async(self, *a):
            events.append(("gather", len([e for e in events if e[0] == "gather"])))

            class P:
                def wait(self, views=True):
                    events.append(("wait",))
            return P()

    class Pipe(_FakePipe):
        def run(self, frames, sync=True):
            super().run(frames, sync)
            return {"frame": int(frames[0]), "dets": 0, "classes": 0, "counts": 0, "masks": 0}

    seen = []
    loop = bench.StepLoop(Pipe(events), None, G(), resident=[torch.tensor([i]) for i in range(2)],
                          on_gathered=lambda t, p: seen.append(t))
    for _ in range(3):
        loop.step()
    loop.finish()
    assert seen == [0, 1, 2]
    kinds = [e[0] for e in events if e[0] in ("gather", "wait")]
    assert kinds == ["gather", "wait", "gather", "wait", "gather", "wait"]


def test_bench_model_is_calibrated_on_the_host():
    """bench.build_bench_model: build_model's calibration pass is handed the model on
    the CPU, device "cpu", at CALIBRATE_THREADS threads, whatever device the model is
    built for ("meta" stands in for the GPU here) and whatever the caller's thread
    count; the model goes back to its device, weights.calibrate and the thread count
    are put back, and a build_model that stops calling weights.calibrate is an error."""
    import pytest
    import torch
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd import weights
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    seen = []

    def stub(model, frame_u8, device):
        seen.append((str(device), {p.device.type for p in model.parameters()},
                     torch.get_num_threads(), frame_u8.shape))

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(2))
            self.moves = []

        def to(self, device):
            self.moves.append(str(device))
            return self

    def fake_build(cfg, seed=0, device="cuda", channels_last=False):
        m = Model()
        m.to(device)
        weights.calibrate(m, np.zeros((4, 4, 3), np.uint8), device)
        return m, {"seed": seed, "channels_last": channels_last}

    cal, build, n = weights.calibrate, weights.build_model, torch.get_num_threads()
    try:
        torch.set_num_threads(3)
        weights.calibrate, weights.build_model = stub, fake_build
        m, sd = bench.build_bench_model(cfg, "meta", True)
        assert weights.calibrate is stub and torch.get_num_threads() == 3
        assert seen == [("cpu", {"cpu"}, bench.CALIBRATE_THREADS, (4, 4, 3))]
        assert m.moves == ["meta", "cpu", "meta"] and sd == {"seed": 0, "channels_last": True}
        weights.build_model = lambda cfg, **kw: (Model(), {})  # calibrates some other way
        with pytest.raises(RuntimeError, match="did not run on the host"):
            bench.build_bench_model(cfg, "meta", True)
        assert weights.calibrate is stub
    finally:
        weights.calibrate, weights.build_model = cal, build
        torch.set_num_threads(n)


def test_step_outputs_and_dump(tmp_path):
    """--dump-outputs: the caller-visible arrays of a completed step (rows past a
    frame's count zeroed, masks cut to sum(counts)) written as float32 .npy, and an
    array over its share of the byte budget cut to the same seeded sample twice."""
    import torch
    dets = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5) + 1
    dets[1, 2, 0] = float("nan")  # past frame 1's count: never part of the result
    out = {"dets": dets, "classes": torch.tensor([[7, 8, 9], [4, 5, 6]], dtype=torch.int32),
           "counts": torch.tensor([3, 1]), "counts_host": [3, 1],
           "masks": torch.rand(6, 4, 4)}
    arrays = bench.step_outputs(out)
    assert sorted(arrays) == ["classes", "counts", "dets", "masks"]
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert np.array_equal(arrays["dets"][0], dets[0].numpy())
    assert np.array_equal(arrays["dets"][1, 0], dets[1, 0].numpy())
    assert not arrays["dets"][1, 1:].any() and not arrays["classes"][1, 1:].any()
    assert arrays["classes"][1, 0] == 4 and arrays["counts"].tolist() == [3.0, 1.0]
    assert np.array_equal(arrays["masks"], out["masks"][:4].numpy())
    bench.dump_outputs(arrays, str(tmp_path / "a"))
    for k, a in arrays.items():
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), a), k
    big = {"x": np.random.default_rng(1).random(100000).astype(np.float32), "y": np.ones(3)}
    for d in ("b", "c"):
        bench.dump_outputs(big, str(tmp_path / d), budget=80000)
    xb, xc = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert xb.dtype == np.float32 and np.array_equal(xb, xc) and 0 < xb.size < big["x"].size
    assert np.isin(xb, big["x"]).all()
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 80000
    bench.dump_outputs(big, str(tmp_path / "d"), budget=100)  # no room: empty samples
    assert np.load(tmp_path / "d" / "x.npy").size == 0


def test_step_watchdog_trips_on_a_stalled_iteration():
    """runner.StepWatchdog: iterations within 10x the median pass; one that runs
    past max(10 x median, floor) trips with its index (on_trip instead of the
    process exit the bench uses)."""
    import time
    from vosdetectron_amd.runner import StepWatchdog
    trips = []
    wd = StepWatchdog(factor=10.0, floor_s=0.05, first_s=5.0, poll_s=0.005,
                      on_trip=lambda i, ran, lim: trips.append((i, ran, lim)))
    try:
        for i in range(4):
            wd.start_step(i)
            time.sleep(0.004)
            wd.end_step()
        assert wd.limit() == 0.05 or wd.limit() >= 10 * 0.004
        wd.start_step(4)
        deadline = time.time() + 3.0
        while not trips and time.time() < deadline:
            time.sleep(0.01)
        assert trips and trips[0][0] == 4 and trips[0][1] > trips[0][2]
    finally:
        wd.stop()
