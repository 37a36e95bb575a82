"""vd_group_norm_act, vd_convgru_gates, vd_convgru_update and the NHWC FlowAlign
at the model's layouts: every element against the float64 restatement of
tests/gn_ref.py within its a-priori float32 bound (inputs built on the CPU, so the
reference does not depend on the device), FlowAlign bit for bit against the
oracle's C restatement.  torch's fp32 GroupNorm on the device is recorded beside
each figure and never asserted on: it misses these bounds where they bite (a group
mean of 4000 sigma, var << eps)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as orc
from tests import gn_ref as gr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# The device's 1 / (1 + expf(-v)) and tanhf against float64 over [-8, 8], measured
# through vd_group_norm_act itself by test_activation_allowances (on an MI355X:
# sigmoid 8.74e-8 = 1.47 ulp at 1, tanhf 4.42e-8 = 0.74 ulp, the same in both
# layouts).  No OCML ulp table ships with the toolchain, so the allowances are twice
# the measurements.
SIGMOID_MEASURED = 8.8e-8
TANH_MEASURED = 4.5e-8
SIGMOID_S = 2 * SIGMOID_MEASURED
TANH_T = 2 * TANH_MEASURED

FMT = {"nchw": torch.contiguous_format, "nhwc": torch.channels_last}
_REF = {}


def _dev(t, layout):
    return t.to(DEV).contiguous(memory_format=FMT[layout]) if t.dim() == 4 else t.to(DEV)


def _gn_case(name):
    """(inputs, {epilogue: (reference, bound)}) of a GroupNorm case, computed once."""
    if name not in _REF:
        G, epis = gr.GN_CASES[name][4], gr.GN_CASES[name][8]
        d = gr.gn_inputs(name)
        _REF[name] = (d, {e: gr.epilogue64(e, d, G, SIGMOID_S, TANH_T)[:2] for e in epis})
    return _REF[name]


def _kwargs(kind, dd):
    """ops.group_norm_act keywords of an epilogue on the device inputs dd."""
    return {"none": {}, "relu": {"act": "relu"},
            "sigmoid": {"act": "sigmoid", "x2": dd.get("x2")},
            "tanh": {"act": "tanh", "x2": dd.get("x2")},
            "res": {"act": "relu", "residual": dd.get("res")},
            "res_up": {"residual": dd.get("res_up"), "upsample_residual": True},
            "res_gn": {"act": "relu", "residual": dd.get("res_g"),
                       "residual_gn": (dd.get("gamma_r"), dd.get("beta_r"))}}[kind]


def _run(kind, dd, G, **extra):
    from vosdetectron_amd import ops
    kw = _kwargs(kind, dd)
    kw.update(extra)
    return ops.group_norm_act(dd["x"], G, dd["gamma"], dd["beta"], gr.EPS, **kw)


def _torch(kind, dd, G):
    """The same epilogue composed from torch's fp32 ops on the device."""
    gn = lambda x, g, b: F.group_norm(x, G, g, b, gr.EPS)  # noqa: E731
    if kind in ("sigmoid", "tanh"):
        y = gn(dd["x"] + dd["x2"], dd["gamma"], dd["beta"])
        return torch.sigmoid(y) if kind == "sigmoid" else torch.tanh(y)
    y = gn(dd["x"], dd["gamma"], dd["beta"])
    if kind == "relu":
        y = F.relu(y)
    elif kind == "res":
        y = F.relu(y + dd["res"])
    elif kind == "res_up":
        y = y + gr.up2(dd["res_up"])
    elif kind == "res_gn":
        y = F.relu(y + gn(dd["res_g"], dd["gamma_r"], dd["beta_r"]))
    return y


def _figures(out, ref, bound):
    err = (out.cpu().double() - ref).abs()
    return err, {"max_err": float(err.max()), "min_margin": float((bound - err).min()),
                 "max_ratio": float((err / bound).max())}


def test_activation_allowances():
    """The device sigmoid and tanhf at 2048 known points.  eps = 0, x alternating
    +1 / -1 along W, beta = 0: every group has mean 0 and variance 1 exactly, rstd
    is 1, and the pre-activation is exactly +-gamma_c (each product is by 1, the
    sum with 0; an FMA changes nothing), gamma a sweep of [-8, 8] over 1024
    channels.  Prints the largest error in both layouts; the constants above must
    cover the measurement, and the allowances must stay within 8 u."""
    from vosdetectron_amd import ops
    B, C, H, W, G = 1, 1024, 2, 2, 32
    gamma = torch.linspace(-8, 8, C)
    x = torch.ones((B, C, H, W))
    x[..., 1::2] = -1
    pre = x.double() * gamma.double().view(1, C, 1, 1)
    rec = {}
    for act, fn in (("sigmoid", torch.sigmoid), ("tanh", torch.tanh)):
        for layout in ("nchw", "nhwc"):
            out = ops.group_norm_act(_dev(x, layout), G, gamma.to(DEV), torch.zeros(C, device=DEV),
                                     0.0, act=act)
            rec[act + "_" + layout] = float((out.cpu().double() - fn(pre)).abs().max())
    rec["ulp_at_1"] = {k: v / gr.U for k, v in rec.items()}
    print("GN_ALLOWANCE " + json.dumps(rec))
    assert max(rec["sigmoid_nchw"], rec["sigmoid_nhwc"]) <= SIGMOID_MEASURED
    assert max(rec["tanh_nchw"], rec["tanh_nhwc"]) <= TANH_MEASURED
    assert SIGMOID_S <= 8 * gr.U and TANH_T <= 8 * gr.U


@pytest.mark.parametrize("name,layout", [(n, l) for n in gr.GN_CASES for l in gr.GN_CASES[n][7]])
def test_group_norm_within_bound(name, layout):
    """Per element |kernel - float64| <= bound for every epilogue of the case."""
    G, epis = gr.GN_CASES[name][4], gr.GN_CASES[name][8]
    d, refs = _gn_case(name)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    bad = []
    for kind in epis:
        ref, bound = refs[kind]
        out = _run(kind, dd, G)
        assert out.is_contiguous(memory_format=FMT[layout]) and out.shape == dd["x"].shape
        err, rec = _figures(out, ref, bound)
        rec.update(case=name, layout=layout, epilogue=kind,
                   torch_max_err=float((_torch(kind, dd, G).cpu().double() - ref).abs().max()))
        print("GN_CASE " + json.dumps(rec))
        if not bool((err <= bound).all()):
            bad.append((kind, rec["max_ratio"]))
    if name == "big":
        del _REF[name]  # 0.6 GB of float64
    assert not bad, bad


def test_upsample_residual_refuses_odd_map():
    """The nearest-2x residual needs even H and W; the C layer says so."""
    from vosdetectron_amd import ops
    x = torch.randn((1, 64, 7, 7), device=DEV)
    r = torch.randn((1, 64, 3, 3), device=DEV)
    w = torch.ones(64, device=DEV)
    from vosdetectron_amd._lib import VosdetError
    with pytest.raises(VosdetError, match="vd_group_norm_act"):
        ops.group_norm_act(x, 32, w, w, residual=r, upsample_residual=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,G,layout", [((2, 128, 12, 20), 32, "nchw"),
                                            ((2, 128, 12, 20), 32, "nhwc"),
                                            ((1, 96, 10, 12), 32, "nhwc"),
                                            ((2, 2048, 4, 6), 32, "nhwc"),
                                            ((1, 64, 34, 46), 32, "nhwc")])
def test_constant_group_gives_beta_bits(shape, G, layout):
    """x constant per group and exactly representable (1.5, 1.75, ...): every sum
    is exact, var is exactly 0, v - mean is 0 and the output is beta bit for bit."""
    from vosdetectron_amd import ops
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(5)
    val = 1.5 + 0.25 * torch.arange(B * G, dtype=torch.float32).view(B, G, 1)
    x = val.expand(B, G, (C // G) * H * W).reshape(shape).contiguous()
    gamma = torch.randn(C, generator=gen)
    beta = torch.randn(C, generator=gen) + 3.0  # no zero: -0 + 0 would hide a sign
    out = ops.group_norm_act(_dev(x, layout), G, gamma.to(DEV), beta.to(DEV), gr.EPS).cpu()
    assert bool(torch.isfinite(out).all())
    want = beta.view(1, C, 1, 1).expand(shape)
    assert torch.equal(out.view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", ["p6", "stem"])
def test_in_place_matches_out_of_place(name, layout):
    """out=x, as the model's GroupNorm epilogue calls it, gives the bits of the
    out-of-place call for every epilogue -- the GroupNorm'd residual included, whose
    statistics must be read before x is overwritten.  (A reordering of the double
    sums moves a mean by 1e-16 of itself; it changes the float it rounds to about
    once in 1e8 groups, so the bits are compared.)"""
    G, epis = gr.GN_CASES[name][4], gr.GN_CASES[name][8]
    d, _ = _gn_case(name)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    for kind in epis:
        want = _run(kind, dd, G)
        x = dd["x"].clone(memory_format=torch.preserve_format)
        got = _run(kind, dict(dd, x=x), G, out=x)
        assert got.data_ptr() == x.data_ptr()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), kind
        assert torch.equal(dd["x"].cpu(), d["x"]), kind  # the out-of-place input is intact


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_two_calls_agree_within_bound(layout):
    """The double atomics may reorder the sums: two calls agree within 2 b_gn
    (bit equality is recorded, not asserted)."""
    name = "stem"
    d, refs = _gn_case(name)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    a, b = _run("none", dd, 32).cpu(), _run("none", dd, 32).cpu()
    diff = (a.double() - b.double()).abs()
    print("GN_REPEAT " + json.dumps({"case": name, "layout": layout, "max_diff": float(diff.max()),
                                     "bit_equal": bool(torch.equal(a.view(torch.int32),
                                                                   b.view(torch.int32)))}))
    assert bool((diff <= 2 * refs["none"][1]).all())


# --------------------------------------------------------------------------- ConvGRU
def _gru_case(name):
    key = "gru_" + name
    if key not in _REF:
        d = gr.gru_inputs(name)
        ref = {}
        for state in (True, False):
            ref["gates", state] = gr.gates64(d, gr.GRU_G, SIGMOID_S, state=state)
            for finer in (True, False):
                ref["update", state, finer] = gr.update64(d, gr.GRU_G, TANH_T, state=state,
                                                          finer=finer)[:2]
        _REF[key] = (d, ref)
    return _REF[key]


def _gates(dd, state):
    from vosdetectron_amd import ops
    a = [dd["zx"], dd["rx"], dd["h"], dd["zh"], dd["rh"]] if state else [dd["zx"]] + [None] * 4
    return ops.convgru_gates(*a, gr.GRU_G, dd["gamma_z"], dd["beta_z"], dd["gamma_r"],
                             dd["beta_r"], gr.EPS)


def _update(dd, state, finer):
    from vosdetectron_amd import ops
    return ops.convgru_update(dd["hx"], dd["hh"] if state else None, dd["z"],
                              dd["h"] if state else None, gr.GRU_G, dd["gamma_h"], dd["beta_h"],
                              finer=dd["finer"] if finer else None, eps=gr.EPS)


def _torch_gn(x, dd, k):
    return F.group_norm(x, gr.GRU_G, dd["gamma_" + k], dd["beta_" + k], gr.EPS)


@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", sorted(gr.GRU_CASES))
def test_convgru_gates_within_bound(name, layout, state):
    d, ref = _gru_case(name)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    z, hr = _gates(dd, state)
    got = {"z": z}
    tz = torch.sigmoid(_torch_gn(dd["zx"] + dd["zh"] if state else dd["zx"], dd, "z"))
    tref = {"z": tz}
    if state:
        got["hr"] = hr
        tref["hr"] = dd["h"] * torch.sigmoid(_torch_gn(dd["rx"] + dd["rh"], dd, "r"))
    else:
        assert hr is None
    bad = []
    for k, out in got.items():
        r, bound = ref["gates", state][k]
        assert out.is_contiguous(memory_format=FMT[layout])
        err, rec = _figures(out, r, bound)
        rec.update(case="gru_" + name, layout=layout, epilogue="gates_" + k, state=state,
                   torch_max_err=float((tref[k].cpu().double() - r).abs().max()))
        print("GN_CASE " + json.dumps(rec))
        if not bool((err <= bound).all()):
            bad.append((k, rec["max_ratio"]))
    assert not bad, bad


@pytest.mark.parametrize("finer", [True, False])
@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("name", sorted(gr.GRU_CASES))
def test_convgru_update_within_bound(name, layout, state, finer):
    """The update stage on its own inputs: an arbitrary z in (0, 1), not the gate
    kernel's output.  Zero state: z * tanh(GN(hx))."""
    d, ref = _gru_case(name)
    dd = {k: _dev(v, layout) for k, v in d.items()}
    out = _update(dd, state, finer)
    assert out.is_contiguous(memory_format=FMT[layout])
    r, bound = ref["update", state, finer]
    t = torch.tanh(_torch_gn(dd["hx"] + dd["hh"] if state else dd["hx"], dd, "h"))
    t = (1 - dd["z"]) * dd["h"] + dd["z"] * t if state else dd["z"] * t
    if finer:
        t = t / 2 + F.avg_pool2d(dd["finer"], 2) / 2
    err, rec = _figures(out, r, bound)
    rec.update(case="gru_" + name, layout=layout, epilogue="update", state=state, finer=finer,
               torch_max_err=float((t.cpu().double() - r).abs().max()))
    print("GN_CASE " + json.dumps(rec))
    assert bool((err <= bound).all()), rec["max_ratio"]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_convgru_zero_state_writes_only_its_outputs(layout):
    """h=None: no input buffer is written by either stage."""
    d, _ = _gru_case("odd")
    dd = {k: _dev(v, layout) for k, v in d.items()}
    keep = {k: v.clone(memory_format=torch.preserve_format) for k, v in dd.items()}
    z, hr = _gates(dd, False)
    out = _update(dd, False, True)
    torch.cuda.synchronize()
    assert hr is None
    ptrs = {v.data_ptr() for v in dd.values()}
    assert z.data_ptr() not in ptrs and out.data_ptr() not in ptrs
    for k, v in dd.items():
        assert torch.equal(v.view(torch.int32), keep[k].view(torch.int32)), k


# --------------------------------------------------------------------------- FlowAlign
def _plant(fl):
    """Boundary values in a B x 2 x H x W flow (H >= 6, W >= 7), all finite: the C
    restatement's int conversion is undefined for NaN and inf."""
    H, W = fl.shape[2:]
    f = np.float32
    below1 = np.nextafter(f(1), f(0))
    tiny = np.nextafter(f(0), f(1))
    spots = [  # (h, w, flow_x, flow_y)
        (1, 2, f(W - 1 - 2), f(0.25)),      # lands exactly on W - 1
        (2, 1, f(0.25), f(H - 1 - 2)),      # exactly on H - 1
        (1, 3, f(-3), f(0.5)),              # exactly on 0 from a negative flow
        (3, 1, f(0.5), f(-3)),
        (3, 2, f(-2), f(-3)),
        (0, 0, f(-0.0), f(-0.0)),
        (0, 1, f(0.5), f(-0.0)),
        (2, 0, f(-0.0), f(0.5)),
        (1, 0, -tiny, f(0)),                # one float below 0
        (0, 2, f(0), -tiny),
        (2, 3, np.nextafter(f(-3), f(-4)), f(0)),
        (3, 3, f(0), np.nextafter(f(-3), f(-4))),
        (2, W - 2, below1, f(0)),           # w + flow rounds up to W - 1
        (H - 2, 2, f(0), below1),           # h + flow rounds up to H - 1
        (3, 4, f(1e9), f(0)), (4, 3, f(-1e9), f(0)),
        (4, 4, f(0), f(1e9)), (4, 1, f(0), f(-1e9)),
        (5, 3, f(1e9), f(-1e9)),
    ]
    for h, w, fx, fy in spots:
        fl[:, 0, h, w] = fx
        fl[:, 1, h, w] = fy
    assert np.isfinite(fl).all()
    return fl


def _flow_case(B, C, H, W, amp, plant):
    rng = np.random.default_rng(B * 1000 + C * 10 + H)
    f = rng.standard_normal((B, C, H, W)).astype(np.float32)
    fl = rng.uniform(-amp, amp, (B, 2, H, W)).astype(np.float32)
    fl[:, :, ::3] = np.round(fl[:, :, ::3])
    return f, (_plant(fl) if plant else fl)


def _flow_check(f, fl, layouts):
    from vosdetectron_amd import ops
    ref = orc.flow_align(f, fl)
    ft, flt = torch.from_numpy(f).to(DEV), torch.from_numpy(fl).to(DEV)
    for layout in layouts:
        out = ops.flow_align(ft.contiguous(memory_format=FMT[layout]), flt)
        assert out.is_contiguous(memory_format=FMT[layout])
        assert np.array_equal(out.cpu().contiguous().numpy().view(np.int32), ref.view(np.int32)), \
            layout
    return ref


def test_flow_align_nhwc_grid_stride():
    """270,400 pixels > 65536 blocks x 4 waves: the grid-stride loop of the NHWC
    kernel, which the model's P2 takes."""
    f, fl = _flow_case(1, 4, 520, 520, 3.0, True)
    ref = _flow_check(f, fl, ("nhwc", "nchw"))
    # rows from 505 on belong to the second trip of the loop; they are really sampled
    assert np.count_nonzero(ref[0, 0, 505:519]) > 0.9 * 14 * 520


@pytest.mark.parametrize("B,C,H,W", [(2, 512, 6, 7), (1, 512, 9, 13), (2, 12, 6, 7),
                                     (1, 12, 9, 13)])
def test_flow_align_lane_loop_and_boundary_values(B, C, H, W):
    """C = 512: two trips of the lane loop; C = 12: 3 of 64 lanes active; boundary
    displacements planted in the flow (see _plant)."""
    _flow_check(*_flow_case(B, C, H, W, 2.5, True), ("nhwc", "nchw"))


def test_flow_align_two_rows():
    """H - 1 = 1: the smallest map with a sampled row ((1, 8, 1, 7) only checks zeros)."""
    f, fl = _flow_case(1, 8, 2, 7, 1.0, False)
    fl[0, 1, 0, :4] = [0.0, 0.5, -0.0, np.nextafter(np.float32(1), np.float32(0))]
    ref = _flow_check(f, fl, ("nhwc", "nchw"))
    assert np.count_nonzero(ref[0, :, 0, :4]) == 8 * 4  # h + flow in [0, 1): sampled
