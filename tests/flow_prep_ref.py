"""numpy restatement of vd_flow_to_levels (shared by the CPU and GPU tests).

flo_to_blob (lib/utils/blob.py:63-75): the flow is resized like the image
(oracle.cv2_resize_fx, the restated cv2.resize(fx=fy=s, INTER_LINEAR)), its
values multiplied by the scale in float64 (`flo[0] * flo_scale`, a float32 array
times a Python list) and rounded once to float32 by the blob assignment, then
zero-padded and transposed.  At scale 1 the blob is the input itself.
FlowAlign.conv_flow_downsample: level k = (1/k)^3 * the k x k block sum of that
float32 blob -- here in float64, the reference the kernel's float32 tree and
torch's float32 conv are both measured against."""
import numpy as np

from oracle import oracle as orc

STRIDES = (4, 8, 16, 32, 64)


def resized_hw(h, w, s):
    return int(round(h * s)), int(round(w * s))


def flow_blob(raw, s, Hp, Wp):
    """raw: F x H x W x 2 float32 -> F x 2 x Hp x Wp float32 (data_flow)."""
    raw = np.asarray(raw, np.float32)
    out = np.zeros((raw.shape[0], 2, Hp, Wp), np.float32)
    for f, flo in enumerate(raw):
        if s == 1:
            r = flo
        else:
            r = (orc.cv2_resize_fx(flo, s).astype(np.float64) * s).astype(np.float32)
        assert r.shape[:2] == resized_hw(flo.shape[0], flo.shape[1], s)
        out[f, :, :r.shape[0], :r.shape[1]] = r.transpose(2, 0, 1)
    return out


def block_sum(x, k):
    """float64 sum over k x k blocks of the last two axes."""
    x = np.asarray(x, np.float64)
    h, w = x.shape[-2:]
    return x.reshape(x.shape[:-2] + (h // k, k, w // k, k)).sum(axis=(-3, -1))


def level(blob, k):
    """float64 level flow: (1/k)^3 * block sum of the float32 blob."""
    return block_sum(blob, k) * (1.0 / k) ** 3


def level_bound(blob, k):
    """A-priori bound on |float32 level - float64 level|: a float32 sum of k^2
    terms in any order is within (k^2 - 1) u * sum|x| (u = 2^-24) to first order,
    plus one rounding of the scaled result: 1.001 * k^2 * 2^-24 * (1/k)^3 * sum|blob|."""
    return 1.001 * k * k * 2.0 ** -24 * (1.0 / k) ** 3 * block_sum(np.abs(blob), k)
