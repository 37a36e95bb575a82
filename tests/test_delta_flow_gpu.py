"""The delta-flow head (MODEL.USE_DELTA_FLOW) on the GPU: vd_delta_flow_features
and vd_delta_flow_to_levels against the float64 restatement (tests/delta_flow_ref.py)
within a-priori float32 bounds, and VOSPipeline with the option on."""
import json

import numpy as np
import pytest
import torch

from tests import delta_flow_ref as dref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# (B, C, blob H x W, valid) -- what each row catches:
CASES = {
    "border": (2, 64, (64, 128), (1, 1)),       # P6 is 1 x 2: every pixel is a border pixel
    "edges": (1, 256, (192, 320), (1,)),        # 48 x 80 .. 3 x 5: tile edges inside the maps
    "valid": (3, 64, (128, 64), (1, 0, 1)),     # a row without a previous feature
}
# The device tanhf against float64 tanh over [-6, 6] (the range of the tests'
# pre-activations: weights N(0, 0.02), features N(0, 1), C <= 256), measured by
# test_device_tanh_allowance below through the kernel itself (a one-hot weight
# makes the pre-activation exactly the input): 6.27e-8 (1.05 ulp at 1) on an MI355X.  No OCML ulp
# table ships with the toolchain, so the allowance is twice the measurement.
TANH_MEASURED = 6.3e-8
TANH_T = 2 * TANH_MEASURED
_REF = {}


def _case(name):
    """Inputs (float32, CPU) and the float64 references of a case, computed once."""
    if name not in _REF:
        B, C, (Hp, Wp), valid = CASES[name]
        gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 70)
        feats = [torch.randn((B, C, Hp // k, Wp // k), generator=gen) for k in dref.STRIDES]
        weights = [torch.randn((2, C, 3, 3), generator=gen) * 0.02 for _ in dref.STRIDES]
        prev = [torch.rand((B, 2, Hp // k, Wp // k), generator=gen) * 2 - 1 for k in dref.STRIDES]
        pa = [dref.pre(x, w) for x, w in zip(feats, weights)]
        ref = [torch.tanh(p) for p, _ in pa]
        bound = [dref.feature_bound(a, C, TANH_T) for _, a in pa]
        _REF[name] = (feats, weights, prev, ref, bound)
    return _REF[name]


def _features(name, nhwc):
    from vosdetectron_amd import ops
    B, C, (Hp, Wp), valid = CASES[name]
    feats, weights, prev, _, _ = _case(name)
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = [f.to(DEV).contiguous(memory_format=fmt) for f in feats]
    w = [t.to(DEV) for t in weights]
    state = [p.clone().to(DEV) for p in prev]
    ptrs = [s.data_ptr() for s in state]
    v = torch.tensor(valid, dtype=torch.int32, device=DEV)
    deltas = ops.delta_flow_features(x, w, state, v, layout=int(nhwc))
    torch.cuda.synchronize()
    assert [s.data_ptr() for s in state] == ptrs
    return [s.cpu() for s in state], [d.cpu() for d in deltas]


@pytest.mark.parametrize("name", sorted(CASES))
def test_features_within_bound_and_delta_exact(name):
    """Per element |feat - tanh64(pre64)| <= gamma_(9C) * sum|w x| + t in both
    layouts (and the two layouts within that bound of each other); delta is
    float32(new) - float32(previous) bit for bit where valid and exactly zero
    where not; the state holds the new feature in the buffer it was given."""
    B, C, (Hp, Wp), valid = CASES[name]
    _, _, prev, ref, bound = _case(name)
    got = {nhwc: _features(name, nhwc) for nhwc in (False, True)}
    rec = {"case": name, "max_err": {}, "min_margin": {}, "nchw_vs_nhwc": []}
    for nhwc, (state, deltas) in got.items():
        errs = [(s.double() - r).abs() for s, r in zip(state, ref)]
        rec["max_err"]["nhwc" if nhwc else "nchw"] = [float(e.max()) for e in errs]
        rec["min_margin"]["nhwc" if nhwc else "nchw"] = [float((b - e).min())
                                                         for e, b in zip(errs, bound)]
    rec["nchw_vs_nhwc"] = [float((a - b).abs().max()) for a, b in zip(got[False][0], got[True][0])]
    print("DELTAFLOW_FEAT " + json.dumps(rec))
    for nhwc, (state, deltas) in got.items():
        for i, (s, d, p, r, b) in enumerate(zip(state, deltas, prev, ref, bound)):
            assert s.shape == p.shape == d.shape and s.dtype == d.dtype == torch.float32
            assert bool(((s.double() - r).abs() <= b).all()), (nhwc, i)
            want = s - p  # one IEEE float32 subtraction of the stored values
            for row, ok in enumerate(valid):
                if ok:
                    assert torch.equal(d[row].view(torch.int32), want[row].view(torch.int32)), \
                        (nhwc, i, row)
                else:
                    assert not d[row].any(), (nhwc, i, row)
    for a, c, b in zip(got[False][0], got[True][0], bound):
        assert bool(((a.double() - c.double()).abs() <= b).all())


def test_device_tanh_allowance():
    """Measures the device tanhf through the kernel: with a weight that is 1 at the
    centre tap of one channel and 0 elsewhere the pre-activation is exactly the
    input (one product by 1, sums with zeros), so feat = tanhf(x).  Prints the
    largest |tanhf(x) - tanh64(x)| over [-6, 6] and asserts the constant the other
    tests use is at least the measurement and at most a few ulp."""
    from vosdetectron_amd import ops
    B, C, H, W = 1, 64, 48, 80
    xs = torch.linspace(-6, 6, H * W).reshape(1, 1, H, W)
    x = torch.zeros((B, C, H, W))
    x[:, 3] = xs[:, 0]
    x[:, 5] = xs[:, 0].flip(-1)
    w = torch.zeros((2, C, 3, 3))
    w[0, 3, 1, 1] = 1
    w[1, 5, 1, 1] = 1
    worst = 0.0
    for nhwc in (False, True):
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        state = [torch.zeros((B, 2, H, W), device=DEV)]
        ops.delta_flow_features([x.to(DEV).contiguous(memory_format=fmt)], [w.to(DEV)], state,
                                torch.ones(1, dtype=torch.int32, device=DEV), layout=int(nhwc))
        s = state[0].cpu().double()
        e0 = (s[0, 0] - torch.tanh(xs[0, 0].double())).abs().max()
        e1 = (s[0, 1] - torch.tanh(xs[0, 0].flip(-1).double())).abs().max()
        worst = max(worst, float(e0), float(e1))
    print("DELTAFLOW_TANH " + json.dumps({"max_abs_err": worst, "ulp_at_1": worst / 2.0 ** -24}))
    assert worst <= TANH_MEASURED * 1.0000001
    assert TANH_T <= 8 * 2.0 ** -24


def _rand_deltas(name):
    B, C, (Hp, Wp), _ = CASES[name]
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 90)
    return [torch.rand((B, 2, Hp // k, Wp // k), generator=gen) * 4 - 2 for k in dref.STRIDES]


@pytest.mark.parametrize("name", sorted(CASES))
def test_to_levels_within_bound(name):
    """data_flow and the five level flows against the float64 restatement.

    Bound per blob pixel: c * u * sum_i (1/s_i) * bilerp_i(|d_i|) with c = 8 -- the
    kernel computes hy0 * (hx0 * a + hx1 * b) + hy1 * (hx0 * c + hx1 * d) with exact
    weights (4 roundings on the path of any source value), the product by 1/s is
    exact, and the five terms are added coarsest first into a zero accumulator (at
    most 4 more roundings): (1 + u)^8 - 1 <= gamma_8.  Through the block sums the
    count grows by the depth of the fixed tree (4 inside a thread's 4 x 4 block, 2
    per coarser level): gamma_(8 + depth) * s^3 * blocksum(the same sum).
    Also printed, without a threshold: the largest error of the kernel and of the
    torch float32 composition on the device against float64.  With blob NULL the
    levels are bit-identical."""
    from vosdetectron_amd import ops
    B, C, (Hp, Wp), _ = CASES[name]
    deltas = _rand_deltas(name)
    dd = [d.to(DEV) for d in deltas]
    levels, blob = ops.delta_flow_to_levels(dd, Hp, Wp, want_blob=True)
    levels2, none = ops.delta_flow_to_levels(dd, Hp, Wp)
    assert none is None
    ref_blob = dref.upsample_sum(deltas)
    ref_levels = dref.levels(ref_blob)
    # the torch composition in float32 on the device
    t_blob = torch.zeros((B, 2, Hp, Wp), device=DEV)
    for d, s in zip(dd, dref.SCALES):
        t_blob = t_blob + torch.nn.functional.interpolate(
            d, scale_factor=1. / s, mode="bilinear", align_corners=False) / s
    t_levels = []
    for k in dref.STRIDES:
        w = torch.zeros((2, 2, k, k), device=DEV)
        w[0, 0] = w[1, 1] = (1.0 / k) ** 3
        t_levels.append(torch.nn.functional.conv2d(t_blob, w, stride=k))
    rec = {"case": name, "max_abs": float(ref_blob.abs().max()),
           "kernel_err": [float((blob.cpu().double() - ref_blob).abs().max())],
           "torch_err": [float((t_blob.cpu().double() - ref_blob).abs().max())]}
    for l, t, r in zip(levels, t_levels, ref_levels):
        rec["kernel_err"].append(float((l.cpu().double() - r).abs().max()))
        rec["torch_err"].append(float((t.cpu().double() - r).abs().max()))
    print("DELTAFLOW_LEVELS " + json.dumps(rec))
    assert blob.shape == (B, 2, Hp, Wp)
    assert bool(((blob.cpu().double() - ref_blob).abs() <= dref.pixel_bound(deltas)).all())
    for k, l, l2, r, b in zip(dref.STRIDES, levels, levels2, ref_levels,
                              dref.level_bounds(deltas)):
        assert l.shape == (B, 2, Hp // k, Wp // k)
        assert bool(((l.cpu().double() - r).abs() <= b).all()), k
        assert torch.equal(l.view(torch.int32), l2.view(torch.int32)), k


def test_to_levels_rejects_a_blob_side_of_96():
    from vosdetectron_amd import _lib, ops
    d = [torch.zeros((1, 2, 2, 2), device=DEV) for _ in range(5)]
    out = [torch.zeros((1, 2, 2, 2), device=DEV) for _ in range(5)]
    st = _lib.lib().vd_delta_flow_to_levels(*[t.data_ptr() for t in d], 1, 96, 128,
                                            *[t.data_ptr() for t in out], None,
                                            torch.cuda.current_stream().cuda_stream)
    assert st == _lib.VD_ERR_SHAPE
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.delta_flow_to_levels(d, 96, 128)
    x = [torch.zeros((1, 32, 2, 2), device=DEV)]
    with pytest.raises(ValueError, match="multiple of 64"):  # C % 64
        ops.delta_flow_features(x, [torch.zeros((2, 32, 3, 3), device=DEV)],
                                [torch.zeros((1, 2, 2, 2), device=DEV)],
                                torch.ones(1, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------ pipeline
FRAME_HW, BATCH = (120, 200), 2  # TEST.SCALE 128: resized 128 x 213, blob 128 x 256


@pytest.fixture(scope="module")
def delta_setup():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import VOSPipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_delta_flow_davis")
    cfg.MODEL.CONV_BODY = "FPN.fpn_ResNet50_conv5_body"  # the head does not depend on depth
    cfg.TEST.SCALE = 128
    H, W = FRAME_HW
    frames = [np.random.RandomState(900 + i).randint(0, 256, (BATCH, H, W, 3), np.uint8)
              for i in range(3)]
    model, _ = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=frames[0][0])
    pipe = VOSPipeline(model, cfg, frame_hw=FRAME_HW, batch=BATCH, device=DEV, channels_last=True)
    assert (pipe.Hp, pipe.Wp) == (128, 256)
    return cfg, model, pipe, [torch.from_numpy(f).to(DEV) for f in frames]


def _composition_levels(model, delta_flow, feats):
    """model.delta_flow(fused=False) + the five conv_flow_downsample convs."""
    flow = delta_flow(feats, fused=False)
    return [m.conv_flow_downsample(flow) for m in model.FlowAligns]


def test_pipeline_flows_match_the_composition(delta_setup, monkeypatch):
    """Three steps of two sequences.  Step 1: zero flows, flow_valid becomes all
    one.  Steps 2, 3: the level flows are non-zero and equal the torch composition
    on the same pre-fusion pyramids within the sum of the two kernel bounds: the
    feature bound (for the new and the previous feature, plus the rounding of their
    difference) carried through the linear upsample / block sums, plus the
    to-levels bound.  The state buffers do not move.  After reset(rows=[1]) row 1's
    flows are exactly zero and row 0's are not."""
    cfg, model, pipe, frames = delta_setup
    C = cfg.FPN.DIM
    weights = [m[0].weight.detach().cpu() for m in model.Conv_Delta_Flows_Features]
    seen = []
    delta_flow = model.delta_flow

    def recording(feats):
        seen.append(list(feats))
        return delta_flow(feats)

    monkeypatch.setattr(model, "delta_flow", recording)
    pipe.reset()
    model.clean_flow_features()
    prev = prev_b = ptrs = None
    for step in range(3):
        out = pipe.run(frames[step])
        pipe.complete(out)
        for k in ("dets", "classes", "counts"):
            assert bool(torch.isfinite(out[k].float()).all())
        got = [l.clone() for l in pipe.level_flows]
        feats = seen[-1]
        with torch.no_grad():
            comp = _composition_levels(model, delta_flow, feats)
        pa = [dref.pre(x.cpu(), w) for x, w in zip(feats, weights)]
        cur = [torch.tanh(p) for p, _ in pa]
        cur_b = [dref.feature_bound(a, C, TANH_T) for _, a in pa]
        assert bool((model.flow_valid == 1).all())
        if step == 0:
            assert all(not g.any() for g in got) and all(not c.any() for c in comp)
            ptrs = [s.data_ptr() for s in model.flow_state]
        else:
            assert [s.data_ptr() for s in model.flow_state] == ptrs
            d = [c - p for c, p in zip(cur, prev)]
            e = [x + y + dref.U * dd.abs() for x, y, dd in zip(cur_b, prev_b, d)]
            tol = [a + b for a, b in zip(dref.propagate(e), dref.level_bounds(d))]
            ref = dref.levels(dref.upsample_sum(d))
            rec = {"step": step + 1, "max_abs": [], "kernel_vs_comp": [], "kernel_vs_f64": [],
                   "comp_vs_f64": [], "min_tol": []}
            for g, c, r, t in zip(got, comp, ref, tol):
                assert g.shape == c.shape and g.any()
                rec["max_abs"].append(float(r.abs().max()))
                rec["kernel_vs_comp"].append(float((g - c).abs().max()))
                rec["kernel_vs_f64"].append(float((g.cpu().double() - r).abs().max()))
                rec["comp_vs_f64"].append(float((c.cpu().double() - r).abs().max()))
                rec["min_tol"].append(float(t.min()))
            print("DELTAFLOW_PIPE " + json.dumps(rec))
            for g, c, r, t in zip(got, comp, ref, tol):
                assert bool(((g.cpu().double() - r).abs() <= t).all())
                assert bool(((g - c).abs().cpu().double() <= t).all())
        prev, prev_b = cur, cur_b
    # a new sequence in row 1
    pipe.reset(rows=[1])
    assert model.flow_valid.tolist() == [1, 0]
    pipe.run(frames[0])
    for l in pipe.level_flows:
        assert not l[1].any() and l[0].any()
    assert model.flow_valid.tolist() == [1, 1]
    pipe.reset()
    assert model.flow_valid.tolist() == [0, 0]
    model.clean_flow_features()


def test_flow_is_consumed_and_arguments_refused(delta_setup, monkeypatch):
    """The P2 hidden state after step 3 differs from the same run with the head's
    flows replaced by None by more than 10 times the difference between two runs of
    the delta route itself; flow= and raw_flow= raise."""
    cfg, model, pipe, frames = delta_setup

    def three_steps():
        pipe.reset()
        for f in frames:
            pipe.complete(pipe.run(f))
        h = model.hidden_states[4].clone()
        pipe.reset()
        return h

    a, b = three_steps(), three_steps()
    fusion = model.temporal_fusion
    with monkeypatch.context() as mp:
        mp.setattr(model, "temporal_fusion", lambda feats, *args, **kw: fusion(feats))
        c = three_steps()
    repeat = float((a - b).abs().max())
    without = float((a - c).abs().max())
    print("DELTAFLOW_CONSUMED " + json.dumps({"run_to_run": repeat, "without_flow": without}))
    assert bool(torch.isfinite(a).all())
    assert without > 10 * repeat and without > 0
    with pytest.raises(ValueError, match="flow"):
        pipe.run(frames[0], flow=torch.zeros((BATCH, 2, pipe.Hp, pipe.Wp), device=DEV))
    with pytest.raises(ValueError, match="raw_flow"):
        pipe.run(frames[0], raw_flow=torch.zeros((BATCH,) + FRAME_HW + (2,), device=DEV))
    assert all(h is None for h in model.hidden_states)  # nothing ran
