"""vd_label_pngs: every stream is read back by the strict reader (tests/label_png_ref.py:
all CRC-32s, the Adler-32 and the bit stream through zlib) and by PIL, and decodes to the
label map and palette that went in -- at the smallest shapes at which each path of the
encoder can go wrong, inside guarded buffers, under graph replay, and through the engine."""
import io

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import label_png_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RNG = np.random.default_rng(11)
PAL = RNG.integers(0, 256, (256, 3), dtype=np.uint8)  # not the default: the palette is data


def _rand(lo, hi, shape):
    return RNG.integers(lo, hi, shape, dtype=np.uint8)


def _const(shape, v):
    return np.full(shape, v, np.uint8)


def _halves(shape, a, b, cut):
    lab = np.full(shape, a, np.uint8)
    lab[:, cut:] = b
    return lab


# name -> [F, H, W]: frames of one call differ in content, so their lengths differ
CASES = {
    "1x1": np.stack([_const((1, 1), 200), _const((1, 1), 0), _const((1, 1), 143)]),
    "9x1": np.stack([_rand(0, 3, (9, 1)), _const((9, 1), 0), _rand(140, 150, (9, 1))]),
    "5x3": np.stack([_const((5, 3), 0), _rand(0, 256, (5, 3)), _const((5, 3), 255)]),
    # runs of 520 per row with the filter byte: matches of 258 and the 1-2 byte tail rule
    "3x519": np.stack([_const((3, 519), 0), _const((3, 519), 7), _halves((3, 519), 0, 9, 259)]),
    "17x40": np.stack([R.blobs(17, 40, 2, seed=1), R.blobs(17, 40, 2, seed=2),
                       _const((17, 40), 1)]),
    # every literal 9 bits: incompressible, the bound's worst case
    "37x53-high": np.stack([_rand(144, 256, (37, 53)) for _ in range(3)]),
    "37x53-any": np.stack([_rand(0, 256, (37, 53)), _rand(0, 2, (37, 53)),
                           _rand(143, 145, (37, 53))]),
    "64x96": np.stack([_const((64, 96), 255), _rand(0, 256, (64, 96)), R.blobs(64, 96, 3)]),
    "96x160": np.stack([R.blobs(96, 160, 5), _const((96, 160), 0), R.blobs(96, 160, 5, seed=7)]),
    # more bytes (17 KB) than one chunk of the join moves (16 KiB), next to a tiny stream
    "96x160-any": np.stack([_rand(0, 256, (96, 160)), _const((96, 160), 9),
                            _rand(100, 200, (96, 160))]),
    # more strips (1026) than the frame kernel has threads: two per thread in its scan
    "8203x1": np.stack([_rand(0, 2, (8203, 1)), _const((8203, 1), 0), _rand(0, 256, (8203, 1))]),
    # the widest row: 64 chunks of 64 bytes, the last lane of the last chunk in use
    "2x4095": np.stack([_const((2, 4095), 0), _rand(0, 256, (2, 4095)),
                        _halves((2, 4095), 3, 4, 4094)]),
}
for _w in (258, 259, 260, 261, 262):  # a run of w + 1 (zeros, with the filter byte) or w
    CASES["3x%d" % _w] = np.stack([_const((3, _w), 0), _const((3, _w), 200),
                                   _halves((3, _w), 5, 6, _w - 2)])


def _encode(labs, palette=PAL, out=None):
    from vosdetectron_amd import ops, vis
    streams, lengths = ops.label_pngs(torch.from_numpy(labs).to(DEV),
                                      torch.from_numpy(palette).to(DEV), out)
    return vis.png_bytes(streams, lengths), streams, lengths


def _verify(files, labs, palette=PAL):
    from vosdetectron_amd import ops
    F, H, W = labs.shape
    assert len(files) == F
    for f, data in enumerate(files):
        assert len(data) <= ops.label_png_bound(H, W)
        h, w, pal, px = R.read(data)  # strict: four chunks, one IDAT, every CRC, zlib
        assert (h, w) == (H, W) and np.array_equal(px, labs[f]), f
        assert np.array_equal(pal, palette), f


def _verify_pil(files, labs, palette=PAL):
    Image = pytest.importorskip("PIL.Image")
    for f, data in enumerate(files):
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.mode == "P" and np.array_equal(np.asarray(im), labs[f]), f
        assert np.array_equal(np.array(im.getpalette()[:768], np.uint8).reshape(256, 3), palette)


@pytest.mark.parametrize("name", sorted(CASES))
def test_streams_decode(name):
    labs = CASES[name]
    files, streams, lengths = _encode(labs)
    assert streams.dtype == torch.uint8 and lengths.dtype == torch.int32
    from vosdetectron_amd import ops
    assert tuple(streams.shape) == (3, ops.label_png_bound(*labs.shape[1:]))
    _verify(files, labs)
    _verify_pil(files, labs)


def test_incompressible_stays_inside_the_bound():
    """37 x 53 of bytes >= 144: 9 bits per filtered byte.  The stream comes close to the
    bound (which adds only the unused header and padding bits) and never passes it."""
    from vosdetectron_amd import ops
    labs = CASES["37x53-high"]
    files, _, lengths = _encode(labs)
    bound = ops.label_png_bound(37, 53)
    n = lengths.cpu().numpy()
    assert (n <= bound).all() and (n > bound - 64).all(), (n, bound)
    assert (n >= R.literal_only_size(37, 53)).all()


def test_run_length_coding_is_on():
    """96 x 160 of zeros: the IDAT payload is under 1/8 of the 15360 raw bytes (a
    literal-only coder needs at least that many)."""
    files, _, _ = _encode(CASES["96x160"])
    assert len(R.idat_payload(files[1])) < 96 * 160 // 8
    assert len(files[1]) < len(files[0])


def test_default_palette_and_files(tmp_path):
    from vosdetectron_amd import ops, vis
    labs = CASES["17x40"]
    streams, lengths = ops.label_pngs(torch.from_numpy(labs).to(DEV))
    files = vis.png_bytes(streams, lengths)
    _verify(files, labs, vis.davis_palette().numpy())
    paths = [str(tmp_path / ("%05d.png" % f)) for f in range(3)]
    vis.write_pngs(paths, streams, lengths)
    assert [open(p, "rb").read() for p in paths] == files
    with pytest.raises(ValueError, match="paths"):
        vis.write_pngs(paths[:2], streams, lengths)
    s0, n0 = ops.label_pngs(torch.zeros((0, 5, 3), dtype=torch.uint8, device=DEV))
    assert vis.png_bytes(s0, n0) == []
    # the colour image and the overlay, on the device
    pal = vis.davis_palette()
    clr = vis.label_colors(torch.from_numpy(labs).to(DEV), pal)
    assert clr.is_cuda and np.array_equal(clr.cpu().numpy(), pal.numpy()[labs][..., ::-1])
    im = torch.from_numpy(_rand(0, 256, (3, 17, 40, 3)))
    assert torch.equal(vis.overlay(im.to(DEV), clr).cpu(), vis.overlay(im, clr.cpu()))


# --------------------------------------------------------------------------- guarded
def _guarded(arena, labs, ws_fill, out_fill):
    """vd_label_pngs with out exactly F x bound bytes and the workspace exactly the
    reported size, each between canary strips."""
    from vosdetectron_amd._lib import check, lib
    F, H, W = labs.shape
    lab = arena.carve(labs.shape, torch.uint8, G.ZERO, "vd_label_pngs labels", key="labels")
    lab.copy_(torch.from_numpy(labs))
    pal = arena.carve((256, 3), torch.uint8, G.ZERO, "vd_label_pngs palette", key="palette")
    pal.copy_(torch.from_numpy(PAL))
    bound = lib().vd_label_png_bound(H, W)
    out = arena.carve((F, bound), torch.uint8, out_fill, "vd_label_pngs out", key="out")
    lengths = arena.carve((F,), torch.int32, out_fill, "vd_label_pngs lengths", key="lengths")
    wsb = lib().vd_label_pngs_workspace(F, H, W)
    ws = arena.carve((wsb,), torch.uint8, ws_fill, "vd_label_pngs workspace (%d bytes)" % wsb,
                     key="ws", strip=16)
    check(lib().vd_label_pngs(lab.data_ptr(), F, H, W, pal.data_ptr(), out.data_ptr(), bound,
                              lengths.data_ptr(), ws.data_ptr(), wsb, G.stream()), "vd_label_pngs")
    return out, lengths


@pytest.mark.parametrize("name", ["17x40", "37x53-high", "3x519"])
def test_guarded_buffers(name):
    """Workspace 0x00 / 0xFF / the leftover of a larger instance, out pre-filled 0x00 /
    0xFF: no canary byte changes, and out[f, :lengths[f]] is the same bytes every time."""
    from vosdetectron_amd import vis
    arena = G.Arena(DEV, 4 << 20)
    labs, big = CASES[name], CASES["96x160"]
    seen = []

    def verify(res, out_fill, tag):
        files = vis.png_bytes(*res)
        _verify(files, labs)
        seen.append(files)
        assert files == seen[0], tag

    G.sweep(arena, lambda w, o: _guarded(arena, labs, w, o),
            lambda w, o: _guarded(arena, big, w, o), verify)
    assert len(seen) == 6
    assert seen[0] == _encode(labs)[0]  # and the wrapper's own buffers give them too


# --------------------------------------------------------------------------- determinism
def test_repeatable_and_graph_replay():
    from vosdetectron_amd import ops, vis
    labs = CASES["96x160"]
    lab = torch.from_numpy(labs).to(DEV)
    pal = torch.from_numpy(PAL).to(DEV)
    first = vis.png_bytes(*ops.label_pngs(lab, pal))
    assert vis.png_bytes(*ops.label_pngs(lab, pal)) == first
    out = torch.full((3, ops.label_png_bound(96, 160)), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        streams, lengths = ops.label_pngs(lab, pal, out)
    assert streams.data_ptr() == out.data_ptr()
    for fill in (0x00, 0xFF):
        out.fill_(fill)
        lengths.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert vis.png_bytes(streams, lengths) == first, fill
    # other maps through the same graph: the replay reads the buffer it captured
    lab.copy_(torch.from_numpy(CASES["96x160"][[2, 0, 1]]))
    g.replay()
    torch.cuda.synchronize()
    assert vis.png_bytes(streams, lengths) == [first[2], first[0], first[1]]


# --------------------------------------------------------------------------- engine
def _thresholds(scores):
    s = np.sort(np.asarray(scores, np.float32))
    assert len(s) >= 8, "the step found too few detections to test with"
    return float(s[len(s) // 2]), float(s[3 * len(s) // 4])


def _decoded(res):
    from vosdetectron_amd import vis
    files = vis.png_bytes(res["streams"], res["lengths"])
    px = []
    for data in files:
        h, w, pal, p = R.read(data)
        assert np.array_equal(pal, vis.davis_palette().numpy())
        px.append(p)
    return torch.from_numpy(np.stack(px))


def test_engine_before_and_after_complete():
    """The smallest FPN step of tests/test_label_map_gpu.py: the files decode to exactly
    frame_label_maps' label, for a run(sync=False) output and for the completed one."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd import engine
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.e2e_mask_rcnn_R_50_FPN_1x()
    cfg.TEST.SCALE = 480
    vcfg.check_supported(cfg)
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True)
    pipe = FramePipeline(model, cfg, frame_hw=(480, 640), batch=2, device=DEV,
                         channels_last=True)
    frames = np.stack([np.random.RandomState(900 + r).randint(0, 256, (480, 640, 3), np.uint8)
                       for r in range(2)])
    out = pipe.run(torch.from_numpy(frames).to(DEV), sync=False)
    ks = out["counts"].cpu().tolist()  # the test's own read; `out` stays un-completed
    dets = out["dets"].cpu().numpy()
    thresh, gt_thresh = _thresholds(np.concatenate([dets[f, :k, 4] for f, k in enumerate(ks)]))
    res = engine.frame_label_pngs(pipe, out, thresh, gt_thresh)
    assert "counts_host" not in out and sorted(res) == ["gt", "label", "lengths", "streams"]
    label, gt = engine.frame_label_maps(pipe, out, thresh, gt_thresh)
    assert label.any() and torch.equal(res["label"], label) and torch.equal(res["gt"], gt)
    assert torch.equal(_decoded(res), label.cpu())
    pipe.complete(out)
    res2 = engine.frame_label_pngs(pipe, out, thresh, gt_thresh)
    assert torch.equal(_decoded(res2), engine.frame_label_maps(pipe, out, thresh)[0].cpu())
    with pytest.raises(NotImplementedError, match="RaggedFramePipeline"):
        engine.frame_label_pngs(pipe, dict(out, frame_hw=[(480, 640)] * 2))


def test_vos_files_show_the_kept_rows():
    """The smallest VOS step, TEST.NMS_WITH_MASK_IOU on: the files decode to exactly
    VOSPipeline.frame_label_maps' label, which differs from the unfiltered map."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd import engine
    from vosdetectron_amd.engine import VOSPipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.get("vos_R-101-FPN_3x_gn_dynamic_davis")
    cfg.TEST.SCALE = 240
    cfg.TEST.NMS_WITH_MASK_IOU = 0.5
    cfg.TEST.NUM_DET_PER_CLASS_POST = 1
    vcfg.check_supported(cfg)
    frame = np.random.RandomState(300).randint(0, 256, (240, 427, 3), np.uint8)
    model, _ = build_model(cfg, device=DEV, channels_last=True, calibrate_frame=frame)
    pipe = VOSPipeline(model, cfg, frame_hw=(240, 427), batch=1, device=DEV, channels_last=True)
    out = pipe.run(torch.from_numpy(frame[None]).to(DEV))
    s = np.sort(out["dets"][0, :out["counts_host"][0], 4].cpu().numpy())
    thresh, gt_thresh = float(s[len(s) // 4]), float(s[len(s) // 2])
    res = pipe.frame_label_pngs(out, thresh, gt_thresh)
    label, gt = pipe.frame_label_maps(out, thresh, gt_thresh)
    assert label.any() and torch.equal(res["label"], label) and torch.equal(res["gt"], gt)
    assert torch.equal(_decoded(res), label.cpu())
    unfiltered = engine.frame_label_pngs(pipe, out, thresh, gt_thresh)
    assert torch.equal(_decoded(unfiltered), engine.frame_label_maps(pipe, out, thresh)[0].cpu())
    k = out["counts_host"][0]
    assert not bool(pipe.finalize(out)["valid"][0, :k].all()), "the mask-IoU NMS dropped nothing"
