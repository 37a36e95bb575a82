"""A strict reader of 8-bit indexed PNG files, written with struct and zlib only, for
the tests of vd_label_pngs.  Unlike PIL it checks every chunk's CRC-32 (PIL accepts a
wrong IDAT CRC), and zlib.decompress raises on a wrong Adler-32 or a broken bit stream.

read(data) -> (H, W, palette [256,3] uint8, pixels [H,W] uint8); PngError otherwise.
Also the sizes the tests compare against (literal_only_size) and the label maps they
encode (blobs)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


class PngError(ValueError):
    pass


def chunks(data: bytes):
    """[(type, payload)] of a PNG file image; every length and CRC-32 checked, and
    nothing may follow IEND."""
    if data[:8] != SIGNATURE:
        raise PngError("signature")
    res, at = [], 8
    while at < len(data):
        if at + 12 > len(data):
            raise PngError("truncated chunk header at %d" % at)
        n, typ = struct.unpack(">I4s", data[at:at + 8])
        if at + 12 + n > len(data):
            raise PngError("chunk %r runs past the end" % typ)
        payload = data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        if crc != (zlib.crc32(typ + payload) & 0xffffffff):
            raise PngError("CRC of %r" % typ)
        res.append((typ, payload))
        at += 12 + n
        if typ == b"IEND":
            break
    if at != len(data):
        raise PngError("bytes after IEND")
    return res


def unfilter(raw: bytes, H: int, W: int) -> np.ndarray:
    """Undo PNG filter types 0-4 of an 8-bit one-channel image (bpp = 1)."""
    if len(raw) != H * (W + 1):
        raise PngError("decoded size %d, want %d" % (len(raw), H * (W + 1)))
    out = np.zeros((H, W), np.uint8)
    prev = np.zeros(W, np.int64)
    for y in range(H):
        ft = raw[y * (W + 1)]
        line = np.frombuffer(raw, np.uint8, W, y * (W + 1) + 1).astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(W, np.int64)
            for x in range(W):
                a = cur[x - 1] if x else 0
                b = prev[x]
                c = prev[x - 1] if x else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + p) & 255
        else:
            raise PngError("filter type %d" % ft)
        out[y] = cur
        prev = cur
    return out


def read(data: bytes, critical_only: bool = False):
    """(H, W, palette, pixels) of an 8-bit indexed, non-interlaced PNG whose chunks are
    exactly IHDR, PLTE, IDAT, IEND (critical_only: ancillary chunks are skipped and
    consecutive IDATs joined, as a general reader does)."""
    cs = chunks(bytes(data))
    if critical_only:
        cs = [c for c in cs if c[0] in (b"IHDR", b"PLTE", b"IDAT", b"IEND")]
        idat = b"".join(p for t, p in cs if t == b"IDAT")
        first = [t for t, _ in cs].index(b"IDAT")
        cs = [c for c in cs if c[0] != b"IDAT"]
        cs.insert(first, (b"IDAT", idat))
    if [t for t, _ in cs] != [b"IHDR", b"PLTE", b"IDAT", b"IEND"]:
        raise PngError("chunks %r" % [t for t, _ in cs])
    ihdr, plte, idat, iend = (p for _, p in cs)
    if len(ihdr) != 13 or len(iend) != 0:
        raise PngError("IHDR / IEND length")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", ihdr)
    if (depth, colour, comp, filt, interlace) != (8, 3, 0, 0, 0) or W < 1 or H < 1:
        raise PngError("IHDR fields %r" % ((W, H, depth, colour, comp, filt, interlace),))
    if len(plte) % 3 or not 3 <= len(plte) <= 768:
        raise PngError("PLTE length %d" % len(plte))
    try:
        raw = zlib.decompress(idat)
    except zlib.error as e:
        raise PngError("zlib: %s" % e)
    palette = np.frombuffer(plte, np.uint8).reshape(-1, 3).copy()
    return H, W, palette, unfilter(raw, H, W)


def idat_payload(data: bytes) -> bytes:
    return b"".join(p for t, p in chunks(bytes(data)) if t == b"IDAT")


def literal_only_size(H: int, W: int) -> int:
    """The file size of a fixed-Huffman stream that codes every filtered byte as a 9-bit
    literal in one block: signature 8, IHDR 25, PLTE 780, IDAT 12 + zlib 2 + 4, IEND 12."""
    bits = 3 + 9 * H * (W + 1) + 7
    return 8 + 25 + 780 + 12 + 2 + (bits + 7) // 8 + 4 + 12


def blobs(H: int, W: int, n: int = 5, seed: int = 0) -> np.ndarray:
    """n elliptic objects with ids 1..n on background 0."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    for k in range(1, n + 1):
        cy, cx = rng.integers(H // 8, H - H // 8), rng.integers(W // 8, W - W // 8)
        r = rng.integers(max(H // 16, 2), max(H // 4, 3))
        lab[(yy - cy) ** 2 + ((xx - cx) * 0.7) ** 2 < r * r] = k
    return lab
