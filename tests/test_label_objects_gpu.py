"""vd_label_objects on the device against the numpy restatement (tests/
label_objects_ref.py) and the golden recorded from the reference's davis_db code, bit for
bit: ids, rects, areas, boxes (as float32 words), counts, rle_n and rle_counts[:n]; rows
past a count and the counts of an object over rle_cap keep their prefill."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import guarded
from tests import label_objects_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_objects.npz")
FIELDS = (("ids", torch.uint8, ()), ("rects", torch.int32, (4,)), ("areas", torch.int32, ()),
          ("boxes", torch.float32, (4,)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _out(F, obj_cap, rle_cap, fill, alloc=None):
    """The output dict pre-filled with one byte value (alloc(name, shape, dtype): from an
    arena)."""
    def make(name, shape, dt):
        if alloc is not None:
            return alloc(name, shape, dt)
        item = torch.empty((), dtype=dt).element_size()
        return torch.full(shape + (item,), fill, dtype=torch.uint8, device=DEV).view(dt).reshape(shape)
    out = {n: make(n, (F, obj_cap) + tail, dt) for n, dt, tail in FIELDS}
    out["counts"] = make("counts", (F,), torch.int32)
    if rle_cap:
        out["rle_counts"] = make("rle_counts", (F, obj_cap, rle_cap), torch.int32)
        out["rle_n"] = make("rle_n", (F, obj_cap), torch.int32)
    return out


def _verify(res, labels, expand, remap255, obj_cap, rle_cap, fill=None, what=""):
    """res (device dict) equals the restatement; with `fill`, everything past the defined
    region still holds the prefill byte."""
    objs, counts = R.batch(labels, expand, remap255, obj_cap)
    got = {k: (v.cpu().numpy() if v is not None else None) for k, v in res.items()}
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    for f, o in enumerate(objs):
        k = max(int(counts[f]), 0)
        tag = "%s frame %d" % (what, f)
        if counts[f] >= 0:
            for name in ("ids", "rects", "areas", "boxes"):
                guarded.rows_equal(got[name][f, :k], o[name], "%s: %s" % (tag, name))
        if fill is not None:
            for name in ("ids", "rects", "areas", "boxes"):
                guarded.assert_prefill(res[name][f, k:], fill, "%s: %s past the count" % (tag, name))
        if not rle_cap:
            continue
        for i in range(k):
            runs = o["rle"][i]
            n = len(runs)
            if n <= rle_cap:
                assert got["rle_n"][f, i] == n, (tag, i, got["rle_n"][f, i], n)
                assert np.array_equal(got["rle_counts"][f, i, :n].view(np.uint32), runs), (tag, i)
                if fill is not None:
                    guarded.assert_prefill(res["rle_counts"][f, i, n:], fill, tag + ": rle tail")
            else:
                assert got["rle_n"][f, i] == -n, (tag, i, got["rle_n"][f, i], -n)
                if fill is not None:
                    guarded.assert_prefill(res["rle_counts"][f, i], fill, tag + ": rle over cap")
        if fill is not None:
            guarded.assert_prefill(res["rle_n"][f, k:], fill, tag + ": rle_n past the count")
            guarded.assert_prefill(res["rle_counts"][f, k:], fill, tag + ": rle past the count")
    return objs, counts


def _check(labels, expand=0.05, remap255=False, obj_cap=255, rle_cap=None, what=""):
    """Both prefills, explicit rle_cap (no host read): equal to the restatement and to each
    other, nothing written past the defined region."""
    from vosdetectron_amd import ops
    labels = np.ascontiguousarray(labels, np.uint8)
    F, H, W = labels.shape
    cap = rle_cap or (H * W + 1)
    lab = _dev(labels)
    res = None
    for fill in guarded.FILLS:
        out = _out(F, obj_cap, cap, fill)
        res = ops.label_objects(lab, expand=expand, remap255=remap255, obj_cap=obj_cap,
                                rle_cap=cap, out=out)
        assert all(res[k] is out[k] for k in out)
        objs, counts = _verify(res, labels, expand, remap255, obj_cap, cap, fill,
                               "%s fill 0x%02X" % (what, fill))
    return res, objs, counts


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# --------------------------------------------------------------------------- cases
def test_golden_frame_both_forms(golden):
    """F = 3 copies (37 * 83 is odd: the frames start at three different alignments)."""
    lab = np.stack([golden["labels"]] * 3)
    for remap255, tag in ((False, "raw"), (True, "gt")):
        res, objs, counts = _check(lab, float(golden["expand"]), remap255, what=tag)
        k = len(golden[tag + "_boxes"])
        assert counts.tolist() == [k] * 3
        for f in range(3):
            guarded.rows_equal(res["boxes"][f, :k].cpu().numpy(), golden[tag + "_boxes"], tag)
            assert np.array_equal(res["areas"][f, :k].cpu().numpy().astype(np.float32),
                                  golden[tag + "_seg_areas"])
            assert np.array_equal(res["ids"][f, :k].cpu().numpy(), golden[tag + "_instance_id"])
            n = res["rle_n"][f, :k].cpu().numpy()
            assert np.array_equal(n, golden[tag + "_rle_n"])
            runs = np.concatenate([res["rle_counts"][f, i, :n[i]].cpu().numpy() for i in range(k)])
            assert np.array_equal(runs.view(np.uint32), golden[tag + "_rle"])
    res, _, _ = _check(lab, None, True, what="rect")
    k = len(golden["rect_boxes"])
    guarded.rows_equal(res["boxes"][2, :k].cpu().numpy(), golden["rect_boxes"], "rect boxes")
    assert np.array_equal(res["rects"][2, :k].cpu().numpy(), golden["bboxes_xywh"])


@pytest.mark.parametrize("hw", ((1, 1), (1, 7), (7, 1), (65, 3), (130, 2), (64, 64), (700, 3),
                                (2000, 1)))
def test_small_shapes(hw):
    """65 x 3 and 130 x 2: the RLE pass's 64-row chunk boundary; 700 x 3 and 2000 x 1: a
    wave's 1024 equal bytes cover hundreds of rows."""
    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    maps = [rng.integers(0, 4, (h, w), dtype=np.uint8), np.full((h, w), 2, np.uint8),
            np.where(rng.random((h, w)) < 0.01, 5, 1).astype(np.uint8)]
    maps[1][h // 2, w // 2] = 0
    lab = np.stack(maps)
    for expand in (0.05, None, 0.0):
        _check(lab, expand, what="%dx%d expand %s" % (h, w, expand))
    if hw == (1, 7):  # y2 == y1 after the clip: the entry form drops every object
        lab = np.array([[[1, 1, 0, 2, 0, 3, 3]]], np.uint8)
        _, _, counts = _check(lab, 0.05)
        assert counts.tolist() == [0]
        _, _, counts = _check(lab, None)
        assert counts.tolist() == [3]


def test_whole_frame_object_next_to_an_empty_frame():
    lab = np.zeros((3, 40, 70), np.uint8)
    lab[0] = 9
    lab[2, 5:9, 3:60] = 1
    res, objs, counts = _check(lab)
    assert counts.tolist() == [1, 0, 1]
    assert objs[0]["rle"][0].tolist() == [0, 40 * 70]
    assert res["rects"][0, 0].cpu().tolist() == [0, 0, 70, 40]


def test_column_wrap():
    """Full-height columns run on into the next column's first pixel; an object whose last
    column is full to the last pixel of the map ends without a closing run."""
    lab = np.zeros((2, 10, 8), np.uint8)
    lab[0, :, 2:5] = 1          # three full columns: one run of 30
    lab[0, 0:4, 5] = 2          # starts at row 0 of the next column
    lab[0, :, 7] = 1            # full last column
    lab[1, :, 0:2] = 3          # full first columns: the first run is 0
    lab[1, 0, 2] = 3            # ... running on into column 2
    lab[1, 9, 6] = 4
    lab[1, 0:3, 7] = 4          # (9, 6) and (0, 7) are neighbours in column-major order
    _, objs, _ = _check(lab, None)
    assert objs[0]["rle"][0].tolist() == [20, 30, 20, 10]
    assert objs[0]["rle"][1].tolist() == [50, 4, 26]
    assert objs[1]["rle"][0].tolist() == [0, 21, 59]
    assert objs[1]["rle"][1].tolist() == [69, 4, 7]
    # 130 rows: full columns of more than two 64-row chunks
    lab = np.zeros((1, 130, 5), np.uint8)
    lab[0, :, 1:4] = 6
    lab[0, 64, 2] = 0
    lab[0, 128:, 4] = 7
    _check(lab, None)


def test_borders_and_corners():
    h, w = 33, 70
    lab = np.zeros((2, h, w), np.uint8)
    lab[0, 0, 10:20] = 1         # top
    lab[0, h - 1, 30:66] = 2     # bottom
    lab[0, 5:20, 0] = 3          # left
    lab[0, 8:30, w - 1] = 4      # right
    for i, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
        lab[1, y, x] = 10 + i    # a single pixel in each corner
    for expand in (0.05, None):
        _, _, counts = _check(lab, expand)
        assert counts.tolist() == [4, 4]


def test_rle_cap_too_small_for_one_frame():
    """16 x 16 checkerboard of two values, more than 200 runs each.  rle_cap = 100: both objects
    report -n and write no counts; the frames next to it are complete."""
    lab = np.zeros((3, 16, 16), np.uint8)
    lab[0, 2:9, 3:8] = 5
    lab[1] = R.checkerboard(16, 16, 1, 2)
    lab[2, 4:6, :] = 7
    res, objs, _ = _check(lab, None, rle_cap=100)
    assert res["rle_n"][1, :2].cpu().tolist() == [-len(objs[1]["rle"][0]), -len(objs[1]["rle"][1])]
    assert min(len(r) for r in objs[1]["rle"]) > 100
    assert res["rle_n"][0, 0].item() == 11 and res["rle_n"][2, 0].item() > 0
    # the wrapper's retry (one host read) gives the full rows
    from vosdetectron_amd import ops
    full = ops.label_objects(_dev(lab), expand=None)
    _verify(full, lab, None, False, 255, full["rle_counts"].shape[2])
    assert full["rle_counts"].shape[2] == max(len(r) for r in objs[1]["rle"])


def test_255_values_in_one_frame():
    lab = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    _, _, counts = _check(lab, None)
    assert counts.tolist() == [255]
    _, _, counts = _check(lab, None, remap255=True)  # len(vals) - 1 == 255: unchanged
    assert counts.tolist() == [255]
    _check(np.stack([lab[0], lab[0].T]), 0.05)


def test_obj_cap_overflow_fails_that_frame_only():
    from vosdetectron_amd import _lib, ops
    lab = np.zeros((3, 12, 20), np.uint8)
    for v in range(1, 5):
        lab[0, v:v + 3, 4 * v:4 * v + 3] = v
        lab[2, 2 * v:2 * v + 2, 1:6] = 9 - v
    for v in range(1, 6):
        lab[1, 2 * v:2 * v + 2, 3 * v:3 * v + 4] = v * 11
    res, _, counts = _check(lab, 0.05, obj_cap=4)
    assert counts.tolist() == [4, R.FAILED, 4]
    with pytest.raises(_lib.VosdetError):
        ops.raise_on_failed_counts(res["counts"].cpu().tolist())
    _, _, counts = _check(lab, 0.05, obj_cap=5)
    assert counts.tolist() == [4, 5, 4]


def test_remap_255():
    h, w = 9, 14
    a = np.zeros((h, w), np.uint8)
    a[1:3, 1:4], a[4:6, 2:9], a[6:9, 10:14] = 1, 2, 255      # {0, 1, 2, 255}: 255 -> 3
    b = np.array(a)
    b[4:6, 2:9] = 3                                          # {0, 1, 3, 255}: 255 joins 3
    c = np.full((h, w), 1, np.uint8)
    c[2:5, 3:7] = 255                                        # {1, 255}: 255 -> 1, one object
    d = np.full((h, w), 255, np.uint8)                       # {255}: -> 0, no object
    lab = np.stack([a, b, c, d])
    for expand in (None, 0.05):
        res, objs, counts = _check(lab, expand, remap255=True)
        assert counts.tolist() == [3, 2, 1, 0]
        assert objs[0]["ids"].tolist() == [1, 2, 3] and objs[1]["ids"].tolist() == [1, 3]
        assert objs[1]["rects"][1].tolist() == [2, 4, 12, 5]  # the union rect
        assert objs[1]["areas"][1] == 14 + 12
        assert objs[2]["areas"][0] == h * w and objs[2]["rle"][0].tolist() == [0, h * w]
        _, objs, counts = _check(lab, expand, remap255=False)
        assert counts.tolist() == [3, 3, 2, 1]
        assert objs[1]["ids"].tolist() == [1, 3, 255]


def test_wide_rects():
    """The RLE pass stages no column tile.  Its paths change with the rect width at 16
    columns (the 16 waves of a workgroup take a second column) and at 1024 columns (a
    thread of the column scan sums more than one column): rects of 17, 1025 and 1100
    columns, at H = 5."""
    lab = np.zeros((3, 5, 1100), np.uint8)
    rng = np.random.default_rng(11)
    lab[0, 1:4, 40:57] = 1
    lab[0, 2, 45] = 0
    lab[1, :, 30:1055] = np.where(rng.random((5, 1025)) < 0.7, 2, 0)
    lab[1, 0, 30] = lab[1, 4, 1054] = 2
    lab[2] = np.where(rng.random((5, 1100)) < 0.5, 3, 4)
    _, objs, _ = _check(lab, 0.05)
    assert objs[0]["rects"][0].tolist() == [40, 1, 17, 3]
    assert objs[1]["rects"][0].tolist() == [30, 0, 1025, 5]


def test_statistics_over_many_workgroups():
    """160 x 260 takes three workgroups per frame; 4100 x 4100 more chunks than the
    1024-workgroup grid covers in one visit (the strided loop)."""
    from vosdetectron_amd import ops
    lab = np.stack([R.blobs(160, 260, 6, seed=s) for s in (3, 4)])
    _check(lab, 0.05, obj_cap=16, rle_cap=2000)
    big = np.zeros((4100, 4100), np.uint8)
    big[17:4000, 5:90] = 1
    big[4090:4100, 4000:4100] = 2
    big[2000, 2000] = 3
    res = ops.label_objects(_dev(big[None]), want_rle=False)
    assert res["rle_counts"] is None and res["rle_n"] is None
    assert res["counts"].cpu().tolist() == [3]
    assert res["rects"][0, :3].cpu().tolist() == [[5, 17, 85, 3983], [4000, 4090, 100, 10],
                                                  [2000, 2000, 1, 1]]
    assert res["areas"][0, :3].cpu().tolist() == [85 * 3983, 1000, 1]
    want = np.stack([R.entry_box(r, 0.05, 4100, 4100)[0] for r in
                     ((5, 17, 85, 3983), (4000, 4090, 100, 10), (2000, 2000, 1, 1))])
    guarded.rows_equal(res["boxes"][0, :3].cpu().numpy(), want.astype(np.float32), "boxes")


def test_rle_equals_mask_rle_kernel(golden):
    """An independent, already pinned kernel: ops.mask_rle_counts on the planes
    (labels == v) made with torch."""
    from vosdetectron_amd import ops
    lab = np.stack([golden["labels"], R.blobs(37, 83, 9, seed=5)])
    dl = _dev(lab)
    res = ops.label_objects(dl, expand=None)
    counts = res["counts"].cpu().tolist()
    assert min(counts) >= 5
    for f, k in enumerate(counts):
        ids = res["ids"][f, :k]
        planes = (dl[f][None] == ids[:, None, None]).to(torch.uint8)
        c, n = ops.mask_rle_counts(planes)
        assert torch.equal(n, res["rle_n"][f, :k])
        for i in range(k):
            assert torch.equal(c[i, :n[i]], res["rle_counts"][f, i, :n[i]]), (f, i)


def test_graph_capture_and_replay():
    from vosdetectron_amd import ops
    a = np.stack([R.blobs(37, 83, 5, seed=1), R.blobs(37, 83, 3, seed=2)])
    b = np.stack([R.blobs(37, 83, 7, seed=8), np.zeros((37, 83), np.uint8)])
    cap, rle_cap = 16, 4 * 83 + 2
    lab = _dev(a)
    out = _out(2, cap, rle_cap, 0)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.label_objects(lab, obj_cap=cap, rle_cap=rle_cap, out=out)  # warm on the stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        res = ops.label_objects(lab, obj_cap=cap, rle_cap=rle_cap, out=out)
    torch.cuda.synchronize()
    for maps in (b, a):
        lab.copy_(_dev(maps))
        g.replay()
        torch.cuda.synchronize()
        _verify(res, maps, 0.05, False, cap, rle_cap, what="replay")
        eager = ops.label_objects(_dev(maps), obj_cap=cap, rle_cap=rle_cap)
        n = eager["counts"].cpu().tolist()
        assert torch.equal(eager["counts"], res["counts"])
        for f, k in enumerate(n):
            for name in ("ids", "rects", "areas", "boxes", "rle_n"):
                assert torch.equal(eager[name][f, :k], res[name][f, :k]), name


def test_in_guarded_buffers(monkeypatch):
    """Every buffer exact and between canaries, the workspace of exactly the reported size
    pre-filled 0x00 / 0xFF / left over from a larger instance."""
    from vosdetectron_amd import ops
    arena = guarded.Arena(DEV, 8 << 20)
    small = np.stack([R.golden_frame(), np.zeros((37, 83), np.uint8), R.blobs(37, 83, 6, seed=2)])
    small[2, :, 80:] = 200  # full-height columns up to the last pixel of the last frame
    large = np.stack([R.blobs(64, 96, 12, seed=s) for s in range(4)])
    calls = []

    def call(labels, obj_cap, rle_cap, ws_fill, out_fill):
        F, H, W = labels.shape
        lab = arena.carve(labels.shape, torch.uint8, guarded.ZERO, name="labels")
        lab.copy_(torch.from_numpy(labels))
        out = _out(F, obj_cap, rle_cap, out_fill,
                   alloc=lambda name, shape, dt: arena.carve(shape, dt, out_fill, name=name,
                                                             key=("out", name)))
        log = guarded.guarded_ws(monkeypatch, arena, guarded.ONES if ws_fill is guarded.KEEP
                                 else ws_fill, reuse=True, strip=5136 + 32 * obj_cap)
        res = ops.label_objects(lab, obj_cap=obj_cap, rle_cap=rle_cap, out=out)
        assert [n for _, n, _ in log] == [ops.lib().vd_label_objects_workspace_size(F, H, W, obj_cap)]
        calls.append(log[0][1])
        return res, labels, obj_cap, rle_cap

    def verify(r, out_fill, tag):
        res, labels, obj_cap, rle_cap = r
        _verify(res, labels, 0.05, False, obj_cap, rle_cap, out_fill, tag)

    guarded.sweep(arena, lambda ws, of: call(small, 9, 200, ws, of),
                  lambda ws, of: call(large, 12, 400, ws, of), verify)
    assert min(calls) == 3 * (5136 + 32 * 9)


# --------------------------------------------------------------------------- the chain
FRAME_HW = (160, 260)  # the given-boxes configuration of tests/test_given_boxes_gpu.py


@functools.lru_cache(maxsize=None)
def _maps():
    lab = np.stack([R.blobs(*FRAME_HW, 6, seed=21), R.blobs(*FRAME_HW, 4, seed=22)])
    lab[1][lab[1] == 2] = 255
    return lab


@pytest.fixture(scope="module")
def fast_setup():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import FramePipeline
    from vosdetectron_amd.weights import build_model
    cfg = vcfg.e2e_mask_rcnn_R_50_FPN_1x()
    cfg.MODEL.FASTER_RCNN = False
    cfg.TEST.SCALE, cfg.TEST.MAX_SIZE = 256, 416
    vcfg.check_supported(cfg)
    frames = np.stack([np.random.RandomState(70 + r).randint(0, 256, FRAME_HW + (3,), np.uint8)
                       for r in range(2)])
    model, _ = build_model(cfg, seed=0, device=DEV, channels_last=True,
                           calibrate_frame=frames[0])
    pipe = FramePipeline(model, cfg, frame_hw=FRAME_HW, batch=2, device=DEV, channels_last=True)
    return cfg, pipe, torch.from_numpy(frames).to(DEV)


def test_chain_label_map_to_box_proposals(fast_setup):
    """run(frames, box_proposals=the device's (boxes, counts)) equals the same step fed
    host-made boxes from the restatement, tensor for tensor; no host read lies between
    the label maps and the step."""
    from vosdetectron_amd import davis_db, ops
    cfg, pipe, frames = fast_setup
    lab = _maps()
    res = ops.label_objects(_dev(lab), expand=None, remap255=True, want_rle=False)
    out = pipe.run(frames, keep_intermediates=True, box_proposals=(res["boxes"], res["counts"]))
    objs, counts = R.batch(lab, None, True)
    assert counts.tolist() == [len(o["ids"]) for o in objs] and counts.min() >= 3
    host = np.full((2, 255, 4), 7.25, np.float32)
    for f, o in enumerate(objs):
        host[f, :counts[f]] = o["boxes"]
    want = pipe.run(frames, keep_intermediates=True, box_proposals=(_dev(host), _dev(counts)))
    assert want["counts_host"] == out["counts_host"]
    assert torch.equal(out["counts"], want["counts"]) and sum(out["counts_host"]) > 0
    assert torch.equal(out["roi_counts"], want["roi_counts"])
    assert torch.equal(out["masks"], want["masks"])
    for f in range(2):  # rows past a count hold what the caller's padding rows held
        k, u, n = out["counts_host"][f], int(out["roi_counts"][f]), int(counts[f])
        for key, rows in (("dets", k), ("classes", k), ("rois", u), ("box_index", u),
                          ("box_inv_index", n), ("det_rois", n), ("det_cls_prob", n),
                          ("det_bbox_pred", n)):
            assert torch.equal(out[key][f, :rows], want[key][f, :rows]), (key, f)
    b, c = davis_db.get_bboxes(_dev(lab))
    assert torch.equal(c, res["counts"])
    for f in range(2):
        assert torch.equal(b[f, :counts[f]], res["boxes"][f, :counts[f]])


def test_frame_label_objects_of_a_step(fast_setup):
    from vosdetectron_amd import davis_db, engine, ops
    cfg, pipe, frames = fast_setup
    lab = _maps()
    res = ops.label_objects(_dev(lab), expand=None, remap255=True, want_rle=False)
    out = pipe.run(frames, box_proposals=(res["boxes"], res["counts"]))
    assert sum(out["counts_host"]) > 0
    for which in ("gt", "label"):
        got = engine.frame_label_objects(pipe, out, 0.0, 0.0, which=which, obj_cap=100)
        label, gt = engine.frame_label_maps(pipe, out, 0.0, 0.0)
        assert torch.equal(got["label"], label) and torch.equal(got["gt"], gt)
        src = gt if which == "gt" else label
        want = ops.label_objects(src, obj_cap=100)
        assert torch.equal(got["counts"], want["counts"])
        _verify(got, src.cpu().numpy(), 0.05, False, 100, got["rle_counts"].shape[2], what=which)
    # the entry's fields on the host
    label, _ = engine.frame_label_maps(pipe, out, 0.0, 0.0)
    entries = davis_db.add_gt_annotations(label, obj_cap=255)
    objs, counts = R.batch(label.cpu().numpy(), 0.05)
    from tests.label_map_ref import rle_decode
    for f, e in enumerate(entries):
        guarded.rows_equal(e["boxes"], objs[f]["boxes"], "entry boxes")
        assert np.array_equal(e["seg_areas"], objs[f]["areas"].astype(np.float32))
        assert np.array_equal(e["instance_id"], objs[f]["ids"].astype(np.int32))
        assert len(e["segms"]) == counts[f]
        for s, v in zip(e["segms"], objs[f]["ids"]):
            assert s["size"] == list(FRAME_HW) and isinstance(s["counts"], bytes)
            assert np.array_equal(rle_decode(s), (label[f].cpu().numpy() == v).astype(np.uint8))
