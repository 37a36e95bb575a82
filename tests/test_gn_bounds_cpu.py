"""The bounds of tests/gn_ref.py, checked without a device: a numpy float32
restatement of every kernel stage stays inside its bound on every case that
tests/test_gn_kernels_gpu.py runs (the bounds admit a correct kernel), the bounds
are never weaker than the tolerances of the older tests, and two deliberately
wrong restatements land outside them (the bounds can fail)."""
import pytest
import torch

from tests import gn_ref as gr
from tests.test_gn_kernels_gpu import SIGMOID_S, TANH_T

GN_NAMES = sorted(gr.GN_CASES) + ["legacy"]


def _spec(name):
    return gr.LEGACY_GN if name == "legacy" else gr.GN_CASES[name]


def _ratio(got32, ref, bound):
    return float(((torch.from_numpy(got32).double() - ref).abs() / bound).max())


@pytest.mark.parametrize("name", GN_NAMES)
def test_restatement_inside_gn_bounds(name):
    """All epilogues of the case; the sigmoid and tanh pre-activations stay inside
    the range the allowances are measured on."""
    G, epis = _spec(name)[4], _spec(name)[8]
    d = gr.gn_inputs(name)
    for kind in epis:
        ref, bound, pre = gr.epilogue64(kind, d, G, SIGMOID_S, TANH_T)
        r = _ratio(gr.epilogue32(kind, d, G), ref, bound)
        print("GN_CPU %s %s restatement/bound %.3f" % (name, kind, r))
        assert r <= 1.0, (kind, r)
        if pre is not None and name != "legacy":
            assert float(pre.abs().max()) <= gr.ACT_RANGE, kind


@pytest.mark.parametrize("state", [True, False])
@pytest.mark.parametrize("name", sorted(gr.GRU_CASES))
def test_restatement_inside_gru_bounds(name, state):
    d = gr.gru_inputs(name)
    ref = gr.gates64(d, gr.GRU_G, SIGMOID_S, state=state)
    z, hr = gr.gates32(d, gr.GRU_G, state=state)
    assert _ratio(z, *ref["z"]) <= 1.0
    if state:
        assert _ratio(hr, *ref["hr"]) <= 1.0
    else:
        assert hr is None and "hr" not in ref
    for finer in (True, False):
        out, bound, pre = gr.update64(d, gr.GRU_G, TANH_T, state=state, finer=finer)
        assert _ratio(gr.update32(d, gr.GRU_G, state=state, finer=finer), out, bound) <= 1.0
        ref["pre"].append(pre)
    assert max(float(p.abs().max()) for p in ref["pre"]) <= gr.ACT_RANGE


def test_bounds_not_weaker_than_the_older_tolerances():
    """On the inputs of test_vos_gpu.py's kernel tests every bound's maximum is
    below that test's flat tolerance: 2e-5 for GroupNorm, 1e-5 for the GRU."""
    d = gr.gn_inputs("legacy")
    for kind in gr.LEGACY_GN[8]:
        _, bound, _ = gr.epilogue64(kind, d, gr.LEGACY_GN[4], SIGMOID_S, TANH_T)
        print("GN_CPU legacy %s bound max %.3g" % (kind, float(bound.max())))
        assert float(bound.max()) < gr.LEGACY_GN_TOL, kind
    g = gr.gru_inputs("c64")
    for state in (True, False):
        for _, bound in (v for k, v in gr.gates64(g, gr.GRU_G, SIGMOID_S, state=state).items()
                         if k != "pre"):
            assert float(bound.max()) < gr.LEGACY_GRU_TOL
        for finer in (True, False):
            bound = gr.update64(g, gr.GRU_G, TANH_T, state=state, finer=finer)[1]
            assert float(bound.max()) < gr.LEGACY_GRU_TOL


def test_float32_statistics_land_outside_the_bound():
    """Sum and sum of squares accumulated in float32: on the high-mean case
    (mean = 4000 sigma) the variance is lost and the bound is missed."""
    d = gr.gn_inputs("highmean")
    ref, bound, _ = gr.epilogue64("none", d, 32, SIGMOID_S, TANH_T)
    assert _ratio(gr.epilogue32("none", d, 32), ref, bound) <= 1.0
    assert _ratio(gr.epilogue32("none", d, 32, stats=gr.stats_float32), ref, bound) > 1.0


@pytest.mark.parametrize("name", ["roi7", "quad", "stem"])
def test_count_of_one_channel_lands_outside_the_bound(name):
    """count = H*W instead of (C/G)*H*W (8, 4 and 2 channels per group)."""
    G = gr.GN_CASES[name][4]
    d = gr.gn_inputs(name)
    ref, bound, _ = gr.epilogue64("none", d, G, SIGMOID_S, TANH_T)
    assert _ratio(gr.epilogue32("none", d, G, stats=gr.stats_count_hw), ref, bound) > 1.0
