"""Middlebury .flo optical-flow files, written from the published format:

    bytes 0-3    little-endian float32 tag 202021.25 (the bytes spell "PIEH")
    bytes 4-7    little-endian int32 width
    bytes 8-11   little-endian int32 height
    bytes 12-    height * width * 2 little-endian float32, row-major, u then v
                 per pixel

read_flo returns the H x W x 2 array VOSPipeline.run(raw_flow=...) and
ops.flow_to_levels take (stacked over the frames of a step and uploaded).
"""
from __future__ import annotations

import numpy as np

FLO_TAG = np.float32(202021.25)
_MAX_SIDE = 1 << 20  # a sanity bound on the header, far above any frame


def read_flo(path) -> np.ndarray:
    """The flow of a .flo file as an H x W x 2 float32 array (u, v).  A bad tag, an
    implausible size or a truncated file raises ValueError."""
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12:
            raise ValueError("%s: truncated .flo header (%d of 12 bytes)" % (path, len(head)))
        tag = np.frombuffer(head, "<f4", 1, 0)[0]
        if tag != FLO_TAG:
            raise ValueError("%s: bad .flo tag %r (expected %r)" % (path, float(tag),
                                                                   float(FLO_TAG)))
        w, h = (int(v) for v in np.frombuffer(head, "<i4", 2, 4))
        if not (0 < w <= _MAX_SIDE and 0 < h <= _MAX_SIDE):
            raise ValueError("%s: implausible .flo size %d x %d" % (path, w, h))
        want = h * w * 2 * 4
        data = fh.read(want)
    if len(data) < want:
        raise ValueError("%s: truncated .flo data (%d of %d bytes for %d x %d)"
                         % (path, len(data), want, w, h))
    return np.frombuffer(data, "<f4").astype(np.float32).reshape(h, w, 2)


def write_flo(path, flow) -> None:
    """Write an H x W x 2 flow (u, v) as a .flo file."""
    flow = np.asarray(flow)
    if flow.ndim != 3 or flow.shape[2] != 2 or flow.shape[0] < 1 or flow.shape[1] < 1:
        raise ValueError("write_flo: flow must be H x W x 2, got %s" % (flow.shape,))
    h, w = flow.shape[:2]
    with open(path, "wb") as fh:
        fh.write(np.asarray([FLO_TAG], "<f4").tobytes())
        fh.write(np.asarray([w, h], "<i4").tobytes())
        fh.write(np.ascontiguousarray(flow, "<f4").tobytes())
