"""The path bench.py times, tested as timed (VERDICT r3 "do this" item 1, weak #1).

bench.py captures the BATCH-frame FramePipeline step once per upload slot as a
hipGraph (bench.capture_graphs) and replays it with new frames copied into the
captured slot.  Any state baked in at capture time (a workspace re-allocated
afterwards, a cached permutation, a GEMM / conv plan chosen during capture) would
give wrong outputs at a plausible speed, so here:

* two slots are captured exactly as bench.capture_graphs does, two different
  BATCH-frame batches (bench.synthetic_frames, the bench's own seeds) are uploaded
  into the slots in turn and replayed; dets / classes / counts / class-selected
  masks / mask RoIs / RoI features must equal an eager ``pipe.run(sync=True)``
  on the same frames bit for bit;
* the replayed frame then goes through the stage-wise oracle checks
  (engine_checks.stagewise: proposals and detections bit-exact vs the oracle,
  RoIAlign within 1e-4);
* complete()'s overflow path (more detections than the padded mask batch: a
  second batch from vd_mask_rois at row0 > 0) against a run with a large cap,
  and vd_mask_rois at row0 > 0 against the host-built rows.
Reference: lib/core/test.py:50-111 (im_detect_all), :893-927 (mask rois)."""
import numpy as np
import pytest
import torch

from tests.engine_checks import stagewise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BATCH = __import__("bench").DEFAULT_FRAMES  # the batch bench.py times
KEYS = ("dets", "classes", "counts", "rois", "roi_counts", "masks", "mask_rois", "mask_feat")


@pytest.fixture(scope="module")
def graph_setup():
    import bench
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    model, sd = build_model(cfg, seed=0, device=DEV, channels_last=True)
    pipe = FramePipeline(model, cfg, batch=BATCH, channels_last=True, device=DEV)
    # four distinct host batches, as bench.py cycles through (seeds 1 + i*F)
    host = [bench.synthetic_frames(BATCH, 1 + i * BATCH, 800, 1333) for i in range(4)]
    slots = [torch.from_numpy(host[0]).to(DEV), torch.from_numpy(host[1]).to(DEV)]
    for x in slots:  # bench.py's eager warm-up steps before the capture
        pipe.complete(pipe.run(x, sync=False))
    torch.cuda.synchronize()
    graphs, note = {}, [None]
    bench.capture_graphs(pipe, slots, graphs, note)
    assert note[0] == "captured", note[0]
    return cfg, sd, pipe, host, slots, graphs


def _replay(pipe, graphs, slot, frames_np):
    """bench.step's graph branch: new frames into the captured slot, replay,
    the previous-step host read (complete) on a copy of the static outputs."""
    slot.copy_(torch.from_numpy(frames_np).to(DEV))
    g, gout = graphs[slot.data_ptr()]
    g.replay()
    out = pipe.complete(dict(gout))
    torch.cuda.synchronize()
    # the static outputs are overwritten by the next replay: keep copies
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _assert_same(a, b, what):
    assert a["counts_host"] == b["counts_host"], what
    for k in KEYS:
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        assert torch.equal(x, y), (what, k, float((x.float() - y.float()).abs().max()))


@pytest.mark.parametrize("order", [(2, 3), (3, 2), (0, 1)])
def test_graph_replay_matches_eager(graph_setup, order):
    """Slot 0 then slot 1 replayed with batches the capture never saw (and, for
    (0, 1), the capture batches themselves): bit-identical to eager steps."""
    cfg, sd, pipe, host, slots, graphs = graph_setup
    got = [_replay(pipe, graphs, slots[s], host[b]) for s, b in enumerate(order)]
    for s, b in enumerate(order):
        ref = pipe.run(torch.from_numpy(host[b]).to(DEV), sync=True)
        torch.cuda.synchronize()
        assert sum(ref["counts_host"]) > 0
        _assert_same(got[s], ref, "slot %d batch %d" % (s, b))


def test_graph_replay_stagewise(graph_setup):
    """A replayed frame through the stage-wise oracle checks.  The replay's
    outputs are asserted bit-identical to an eager keep_intermediates step first;
    the upstream tensors the checks feed forward (RPN maps, pyramid) come from
    that eager step, i.e. they equal the graph's own."""
    cfg, sd, pipe, host, slots, graphs = graph_setup
    rep = _replay(pipe, graphs, slots[1], host[3])
    eager = pipe.run(torch.from_numpy(host[3]).to(DEV), keep_intermediates=True)
    torch.cuda.synchronize()
    _assert_same(rep, eager, "stagewise batch")
    for k in ("cls_prob", "bbox_pred"):
        assert torch.equal(rep[k], eager[k]), k
    chk = dict(eager)
    chk.update({k: rep[k] for k in KEYS + ("cls_prob", "bbox_pred", "counts_host")})
    for f in (0, 9):
        rois, _ = stagewise(cfg, pipe, chk, host[3][f], f=f)
        assert len(rois) == 1000


def test_mask_overflow_complete(graph_setup, monkeypatch):
    """complete() with M > mask rows: a 64-row mask batch from
    run(sync=False), the rest through the second vd_mask_rois batch at row0 = 64;
    detections, mask RoIs and mask RoI features bit-identical to the full-cap
    run, masks within 1e-5 (the mask head's GEMM may pick another algorithm for
    the other batch size), and the pyramid reference dropped afterwards."""
    cfg, sd, pipe, host, slots, graphs = graph_setup
    frames = torch.from_numpy(host[2][:3]).to(DEV)
    ref = pipe.run(frames, sync=True)
    torch.cuda.synchronize()
    assert sum(ref["counts_host"]) > 64, ref["counts_host"]
    monkeypatch.setattr(pipe, "mask_rows", lambda F: 64)
    out = pipe.run(frames, sync=False)
    assert out["masks"].shape[0] == 64 and "_pyrs" in out
    out = pipe.complete(out)
    torch.cuda.synchronize()
    assert "_pyrs" not in out
    assert out["counts_host"] == ref["counts_host"]
    for k in ("dets", "classes", "counts", "mask_rois", "mask_feat"):
        assert torch.equal(out[k], ref[k]), k
    assert out["masks"].shape == ref["masks"].shape
    assert float((out["masks"] - ref["masks"]).abs().max()) <= 1e-5


def test_mask_rois_row0_vs_host(graph_setup):
    """vd_mask_rois for global rows [row0, row0 + rows) against the rows built on
    the host from the same detections (_project_im_rois: float64 product, float32
    store; fpn level map), padding rows zero boxes of class 1."""
    from oracle import oracle as orc
    from vosdetectron_amd import ops
    cfg, sd, pipe, host, slots, graphs = graph_setup
    g = torch.Generator().manual_seed(7)
    F, D = 5, 40
    counts = torch.tensor([7, 0, 40, 13, 22], dtype=torch.int32)
    xy = torch.rand(F, D, 2, generator=g) * 1200
    wh = torch.rand(F, D, 2, generator=g) * 400 + 1
    dets = torch.cat([xy, xy + wh, torch.rand(F, D, 1, generator=g)], 2).float()
    cls = torch.randint(1, 81, (F, D), generator=g, dtype=torch.int32)
    scale = torch.tensor([1.0, 0.75, 1.5, 2.2660439, 0.6], dtype=torch.float64)
    host_rows = []
    for f in range(F):
        for j in range(int(counts[f])):
            b = (dets[f, j, :4].double() * scale[f]).float()
            host_rows.append((f, b.numpy(), int(cls[f, j])))
    total = len(host_rows)
    for row0, rows in [(0, 128), (30, 64), (64, 64), (70, 20)]:
        r, lv, c, tot = ops.mask_rois(dets.to(DEV), cls.to(DEV), counts.to(DEV),
                                      scale.to(DEV), rows, 2, 5, row0=row0)
        torch.cuda.synchronize()
        assert int(tot.item()) == total
        r, lv, c = r.cpu().numpy(), lv.cpu().numpy(), c.cpu().numpy()
        for o in range(rows):
            i = row0 + o
            if i < total:
                f, b, k = host_rows[i]
                assert r[o, 0] == f and np.array_equal(r[o, 1:], b), (row0, o)
                want = int(orc.map_rois_to_fpn_levels(b[None], 2, 5)[0]) - 2
                assert lv[o] == want and c[o] == k, (row0, o)
            else:
                assert not r[o].any() and lv[o] == 0 and c[o] == 1, (row0, o)
