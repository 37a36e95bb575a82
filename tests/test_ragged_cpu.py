"""Frames of different sizes in one pipeline step: the host side (no GPU).

ops.frame_geometry must restate get_image_blob's per-frame scale, resized and
padded size exactly (lib/utils/blob.py:37-161: get_target_scale, cv::resize's
dsize, get_max_shape's stride rounding), since the device kernels take the
geometry rows as given; the two new C entries and the wrappers must reject bad
steps before any launch; RaggedFramePipeline is for the FPN configs only."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc

# (H, W) lists with the TEST.SCALE / TEST.MAX_SIZE / stride they are used with
BLOB_SIZES = [(96, 160), (48, 80), (192, 320), (75, 53), (61, 97), (97, 161)]
ENGINE_SIZES = [(256, 416), (416, 256), (200, 300), (128, 200), (250, 410), (128, 208)]
DEMO_SIZES = [(353, 500), (500, 375)]
CASES = [(BLOB_SIZES, 96, 160, 32), (ENGINE_SIZES, 256, 416, 32), (DEMO_SIZES, 800, 1333, 32),
         ([(40, 50), (50, 40), (33, 47)], 600, 1000, 64)]


@pytest.mark.parametrize("sizes,target,max_size,stride", CASES)
def test_frame_geometry_vs_get_image_blob(sizes, target, max_size, stride):
    from vosdetectron_amd import ops
    geo = ops.frame_geometry(sizes, target, max_size, stride)
    assert len(geo) == len(sizes) and geo.sizes == [tuple(s) for s in sizes]
    info = geo.im_info()
    rows = geo.rows()
    pos = 0
    for f, (H, W) in enumerate(sizes):
        blob, scale, im_info = orc.get_image_blob(np.zeros((H, W, 3), np.uint8), target, max_size,
                                                  stride)
        assert geo.scale[f] == scale  # the same double
        assert geo.padded[f] == tuple(blob.shape[2:])
        assert np.array_equal(info[f:f + 1], im_info) and info.dtype == np.float32
        Hr, Wr = geo.resized[f]
        assert geo.padded[f] == (-(-Hr // stride) * stride, -(-Wr // stride) * stride)
        if scale != 1.0:
            assert (Hr, Wr) == orc.cv2_resize_fx(np.zeros((H, W, 1), np.float32), scale).shape[:2]
        else:
            assert (Hr, Wr) == (H, W)
        assert geo.offset[f] == pos
        r = rows[f]
        assert (r["offset"], r["H"], r["W"], r["Hr"], r["Wr"]) == (pos, H, W, Hr, Wr)
        assert r["inv_scale"] == 1.0 / scale
        pos += H * W * 3
    assert geo.nbytes == pos
    assert rows.dtype.itemsize == 32 and rows.view(np.uint8).size == 32 * len(sizes)


def test_geometry_paths_of_the_blob_sizes():
    """The six blob-test frames cover the three paths: scale 1 (inv_scale == 1), x2,
    exactly 0.5 (inv_scale == 2: the 2 x 2 area path), and general scales; (75, 53)
    and (61, 97) have odd byte counts, so frames start at odd byte offsets in
    either order; the bound is 160 x 160."""
    from vosdetectron_amd import ops
    geo = ops.frame_geometry(BLOB_SIZES, 96, 160, 32)
    inv = [float(r["inv_scale"]) for r in geo.rows()]
    assert inv[0] == 1.0 and inv[1] == 0.5 and inv[2] == 2.0
    assert all(v not in (1.0, 2.0) for v in inv[3:])
    assert geo.offset[4] % 2 == 1
    assert any(o % 2 for o in ops.frame_geometry(BLOB_SIZES[::-1], 96, 160, 32).offset)
    assert (max(h for h, _ in geo.padded), max(w for _, w in geo.padded)) == (160, 160)
    assert geo.padded[3] == (160, 96) and geo.padded[0] == (96, 160)


def test_blob_bound():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd import ops
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    assert (cfg.TEST.SCALE, cfg.TEST.MAX_SIZE, cfg.FPN.COARSEST_STRIDE) == (800, 1333, 32)
    assert ops.blob_bound([(800, 1333)], cfg) == (800, 1344)
    assert ops.blob_bound(DEMO_SIZES, cfg) == (1088, 1152)  # 800 x 1133 and 1067 x 800
    with pytest.raises(ValueError):
        ops.blob_bound([], cfg)


def test_new_entries_reject_bad_arguments_on_the_host():
    """VD_ERR_ARG before any launch: F < 1, null pointers, Hp or Wp < 1."""
    from vosdetectron_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails validation
    blob = L.vd_image_resize_to_blob_ragged
    E = _lib.VD_ERR_ARG
    assert blob(p, p, 0, p, 32, 32, 0, p, None) == E
    assert blob(p, p, -1, p, 32, 32, 1, p, None) == E
    assert blob(None, p, 1, p, 32, 32, 0, p, None) == E
    assert blob(p, None, 1, p, 32, 32, 0, p, None) == E
    assert blob(p, p, 1, None, 32, 32, 0, p, None) == E
    assert blob(p, p, 1, p, 32, 32, 0, None, None) == E
    assert blob(p, p, 1, p, 0, 32, 0, p, None) == E
    assert blob(p, p, 1, p, 32, 0, 0, p, None) == E
    rle = L.vd_segm_rle_ragged
    assert rle(p, 0, 28, p, 5, p, 0.5, p, 16, p, None) == _lib.VD_OK  # M == 0: nothing to do
    assert rle(None, 1, 28, p, 5, p, 0.5, p, 16, p, None) == E
    assert rle(p, 1, 28, None, 5, p, 0.5, p, 16, p, None) == E
    assert rle(p, 1, 28, p, 5, None, 0.5, p, 16, p, None) == E
    assert rle(p, 1, 28, p, 5, p, 0.5, None, 16, p, None) == E
    assert rle(p, 1, 28, p, 5, p, 0.5, p, 16, None, None) == E
    assert rle(p, -1, 28, p, 5, p, 0.5, p, 16, p, None) == E
    assert rle(p, 1, 0, p, 5, p, 0.5, p, 16, p, None) == E
    assert rle(p, 1, 28, p, 3, p, 0.5, p, 16, p, None) == E
    assert rle(p, 1, 28, p, 5, p, 0.5, p, 0, p, None) == E
    assert rle(p, 1, 63, p, 5, p, 0.5, p, 16, p, None) == _lib.VD_ERR_SHAPE  # R > 62


def test_geometry_struct_matches_the_header():
    import os
    import re
    from vosdetectron_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "vosdet.h")).read()
    body = re.search(r"typedef struct VdFrameGeom \{(.*?)\} VdFrameGeom;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == ["offset", "H", "W", "Hr", "Wr", "inv_scale"]
    assert [f[0] for f in _lib.VdFrameGeom._fields_] == names == list(ops.GEOM_DTYPE.names)
    for n in names:
        assert getattr(_lib.VdFrameGeom, n).offset == ops.GEOM_DTYPE.fields[n][1], n
    assert ctypes.sizeof(_lib.VdFrameGeom) == ops.GEOM_DTYPE.itemsize == 32


def test_frame_over_the_bound_raises_before_any_launch():
    from vosdetectron_amd import ops
    geo = ops.frame_geometry(BLOB_SIZES, 96, 160, 32)
    ops.check_geometry(geo, 160, 160, geo.nbytes)
    with pytest.raises(ValueError, match="larger than the blob bound"):
        ops.check_geometry(geo, 128, 160)   # the portrait frame is 136 rows
    with pytest.raises(ValueError, match="larger than the blob bound"):
        ops.check_geometry(geo, 160, 128)
    with pytest.raises(ValueError, match="packed buffer"):
        ops.check_geometry(geo, 160, 160, geo.nbytes - 1)
    wide = ops.frame_geometry([(24, 9000)], 24, 9000, 32)
    assert wide.scale == [1.0]
    with pytest.raises(ValueError, match="8192"):
        ops.check_geometry(wide, 32, 9024)
    with pytest.raises(ValueError):
        ops.check_geometry(ops.frame_geometry([], 96, 160, 32), 160, 160)
    with pytest.raises(ValueError):
        ops.frame_geometry([(0, 5)], 96, 160, 32)


@pytest.mark.parametrize("name", ["e2e_mask_rcnn_R-50-C4_1x", "vos_R-101-FPN_3x_gn_dynamic_davis",
                                  "vos_R-101-FPN_3x_gn_static_davis"])
def test_ragged_pipeline_rejects_c4_and_vos(name):
    """NotImplementedError before any device work: no model, and a device this
    host may not have."""
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import RaggedFramePipeline
    cfg = vcfg.get(name)
    with pytest.raises(NotImplementedError):
        RaggedFramePipeline(None, cfg, (512, 896), batch=2, device="cuda")


def test_ragged_pipeline_rejects_a_bad_bound():
    from vosdetectron_amd import config as vcfg
    from vosdetectron_amd.engine import RaggedFramePipeline
    cfg = vcfg.get("e2e_mask_rcnn_R-50-FPN_1x")
    for hw in [(800, 1333), (0, 32), (416, 400)]:
        with pytest.raises(ValueError, match="COARSEST_STRIDE"):
            RaggedFramePipeline(None, cfg, hw, batch=2, device="cuda")
