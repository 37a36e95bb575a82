"""The host side of the label-map PNG files: the strict reader itself (tests/
label_png_ref.py) against PIL-written files and against damaged ones, the palette, the
colour image and overlay, the bound, and the refusals that come before any launch."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import label_png_ref as R


def _pil_png(lab, pal):
    Image = pytest.importorskip("PIL.Image")
    im = Image.frombytes("P", (lab.shape[1], lab.shape[0]), lab.tobytes())
    im.putpalette(pal.tobytes())
    b = io.BytesIO()
    im.save(b, "PNG")
    return b.getvalue()


def _own_png(lab, pal, level=6):
    """A file with exactly the four chunks, written here with zlib."""
    H, W = lab.shape
    raw = b"".join(b"\x00" + lab[y].tobytes() for y in range(H))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)

    return (R.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 3, 0, 0, 0))
            + chunk(b"PLTE", pal.tobytes()) + chunk(b"IDAT", zlib.compress(raw, level))
            + chunk(b"IEND", b""))


def _pal():
    from vosdetectron_amd import vis
    return vis.davis_palette().numpy()


def test_reader_reads_pil_files():
    """Not vacuous: the pixels and the palette of files PIL wrote come back."""
    rng = np.random.default_rng(3)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    for lab in (R.blobs(96, 160), rng.integers(0, 256, (37, 53), dtype=np.uint8),
                np.full((1, 1), 200, np.uint8)):
        H, W, p, px = R.read(_pil_png(lab, pal), critical_only=True)
        assert (H, W) == lab.shape and np.array_equal(px, lab)
        assert np.array_equal(p, pal[:len(p)]) and len(p) > lab.max()


def test_reader_undoes_every_filter_type():
    rng = np.random.default_rng(4)
    lab = rng.integers(0, 256, (6, 11), dtype=np.uint8)
    H, W = lab.shape
    raw = bytearray()
    for y in range(H):
        ft = y % 5
        raw.append(ft)
        for x in range(W):
            a = int(lab[y, x - 1]) if x else 0
            b = int(lab[y - 1, x]) if y else 0
            c = int(lab[y - 1, x - 1]) if x and y else 0
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            raw.append((int(lab[y, x]) - [0, a, b, (a + b) // 2, paeth][ft]) & 255)
    assert np.array_equal(R.unfilter(bytes(raw), H, W), lab)


def test_reader_rejects_damage():
    """One CRC byte of each chunk, one Adler byte, one payload bit, a second IDAT, a
    wrong IHDR field, bytes after IEND."""
    pal = _pal()
    good = _own_png(R.blobs(24, 40), pal)
    assert np.array_equal(R.read(good)[3], R.blobs(24, 40))
    idat_at = good.index(b"IDAT")
    n_idat, = struct.unpack(">I", good[idat_at - 4:idat_at])
    crc_at = {"IHDR": 8 + 8 + 13, "PLTE": 33 + 8 + 768, "IDAT": idat_at + 4 + n_idat,
              "IEND": len(good) - 4}

    def flipped(at, bit=0, fix_idat_crc=False):
        b = bytearray(good)
        b[at] ^= 1 << bit
        if fix_idat_crc:
            b[crc_at["IDAT"]:crc_at["IDAT"] + 4] = struct.pack(
                ">I", zlib.crc32(bytes(b[idat_at:idat_at + 4 + n_idat])) & 0xffffffff)
        return bytes(b)

    for name, at in crc_at.items():
        with pytest.raises(R.PngError, match="CRC"):
            R.read(flipped(at + 1))
    adler_at = idat_at + 4 + n_idat - 4
    with pytest.raises(R.PngError, match="CRC"):  # the chunk CRC catches it first
        R.read(flipped(adler_at))
    with pytest.raises(R.PngError, match="zlib"):  # ... and with that mended, zlib does
        R.read(flipped(adler_at + 2, fix_idat_crc=True))
    with pytest.raises(R.PngError, match="zlib|size"):
        R.read(flipped(idat_at + 4 + 2 + n_idat // 3, bit=5, fix_idat_crc=True))
    two = good[:idat_at - 4] + good[idat_at - 4:crc_at["IDAT"] + 4] * 2 + good[crc_at["IDAT"] + 4:]
    with pytest.raises(R.PngError, match="chunks"):
        R.read(two)
    with pytest.raises(R.PngError, match="IEND"):
        R.read(good + b"\x00")
    b = bytearray(good)
    b[8 + 8 + 9] = 2  # colour type
    b[29:33] = struct.pack(">I", zlib.crc32(bytes(b[12:29])) & 0xffffffff)
    with pytest.raises(R.PngError, match="IHDR"):
        R.read(bytes(b))


def test_davis_palette():
    pal = _pal()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[:5].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128]]
    for i in range(256):
        want = [0, 0, 0]
        for j in range(8):
            for k in range(3):
                want[k] |= (((i >> (3 * j)) >> k) & 1) << (7 - j)
        assert pal[i].tolist() == want, i
    assert len({tuple(r) for r in pal.tolist()}) == 256


def test_label_colors_and_overlay():
    from vosdetectron_amd import vis
    rng = np.random.default_rng(5)
    pal = _pal()
    lab = rng.integers(0, 6, (2, 7, 9), dtype=np.uint8)
    im = rng.integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    lab[0, 0, 0], im[0, 0, 0] = 1, (3, 7, 250)   # RGB (128,0,0): 250 + 51.2 > 255 clips
    lab[0, 0, 1], im[0, 0, 1] = 2, (10, 20, 30)  # 20 + 0.4 * 128 = 71.2 truncates to 71
    clr = vis.label_colors(torch.from_numpy(lab), torch.from_numpy(pal))
    want_clr = pal[lab][..., ::-1]  # what cv2.imread of the file returns: BGR
    assert clr.dtype == torch.uint8 and np.array_equal(clr.numpy(), want_clr)
    got = vis.overlay(torch.from_numpy(im), clr)
    want = np.array(1.0 * im[..., ::-1] + 0.4 * want_clr[..., ::-1]).clip(max=255).astype(np.uint8)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert want[0, 0, 0].tolist() == [255, 7, 3] and want[0, 0, 1].tolist() == [30, 71, 10]
    # one frame, no leading dimension
    assert np.array_equal(vis.overlay(torch.from_numpy(im[0]), clr[0]).numpy(), want[0])


def test_bound():
    from vosdetectron_amd import ops
    for H, W in ((1, 1), (37, 53), (480, 854)):
        assert ops.label_png_bound(H, W) >= R.literal_only_size(H, W), (H, W)
    # what the header derives: 843 fixed bytes, and per strip of r rows
    # floor((9 r (W + 1) + 20) / 8) + 4
    for H, W in ((1, 1), (8, 5), (9, 1), (37, 53), (480, 854), (800, 1333)):
        strips = [8] * (H // 8) + ([H % 8] if H % 8 else [])
        assert ops.label_png_bound(H, W) == 843 + sum((9 * r * (W + 1) + 20) // 8 + 4
                                                      for r in strips)
    for W in (1, 53, 854):
        b = [ops.label_png_bound(H, W) for H in range(1, 70)]
        assert all(x < y for x, y in zip(b, b[1:])), W
    for H in (1, 37, 480):
        b = [ops.label_png_bound(H, W) for W in range(1, 300)]
        assert all(x < y for x, y in zip(b, b[1:])), H
    for H, W in ((0, 5), (5, 0), (16385, 5), (5, 4096)):
        with pytest.raises(ValueError, match="label_png_bound"):
            ops.label_png_bound(H, W)
    assert ops.label_png_bound(16384, 4095) < 2 ** 31


def test_refusals_before_any_launch():
    """A capacity below the bound is refused by the wrapper and by the C entry on the
    host; the pointers are never followed."""
    import ctypes
    from vosdetectron_amd import _lib, ops
    bound = ops.label_png_bound(5, 3)
    with pytest.raises(ValueError, match="cap >= label_png_bound"):  # before any tensor is read
        ops.label_pngs(torch.zeros((2, 5, 3), dtype=torch.uint8),
                       out=torch.zeros((2, bound - 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match="device"):
        ops.label_pngs(torch.zeros((2, 5, 3), dtype=torch.uint8))
    L = _lib.lib()
    F, H, W = 2, 5, 3
    size = L.vd_label_pngs_workspace(F, H, W)
    assert size == F * 1 * 16 and L.vd_label_pngs_workspace(F, 9, W) == F * 2 * 16
    assert L.vd_label_pngs_workspace(F, H, 4096) == 0 and L.vd_label_png_bound(H, 4096) == 0
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(labels=p, F=F, H=H, W=W, palette=p, out=p, cap=bound, lengths=p, ws=p, wsb=size):
        return L.vd_label_pngs(labels, F, H, W, palette, out, cap, lengths, ws, wsb, None)

    assert call(cap=bound - 1) == _lib.VD_ERR_ARG
    for name in ("labels", "palette", "out", "lengths", "ws"):
        assert call(**{name: None}) == _lib.VD_ERR_ARG, name
    for kw in ({"H": 0}, {"W": 0}, {"W": 4096}, {"H": 16385}, {"F": 65536}):
        assert call(**kw) == _lib.VD_ERR_SHAPE, kw
    assert call(wsb=size - 1) == _lib.VD_ERR_WORKSPACE
    assert call(F=0) == _lib.VD_OK


def test_ragged_outputs_are_refused():
    from vosdetectron_amd import engine
    for out in ({"frame_hw": [(30, 40)]}, {"im_hw": None}):
        with pytest.raises(NotImplementedError, match="RaggedFramePipeline"):
            engine.frame_label_pngs(None, out)
