"""Torch-facing wrappers over the C ABI (libvosdet.so).

Every function takes device tensors, launches on torch's current HIP stream and
returns device tensors; shapes and dtypes are checked here, and any kernel
status other than VD_OK raises.  PyTorch is used for allocation and streams
only -- all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import collections
import ctypes
import os
import sys
import weakref
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import VD_ERR_SHAPE, check, lib


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must be a device (HIP) tensor; there is no CPU path" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t.contiguous()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# --------------------------------------------------------------------------- #
# RoIAlign (Caffe2)                                                            #
# --------------------------------------------------------------------------- #
def roi_align_forward(features, rois, aligned_height, aligned_width, spatial_scale,
                      sampling_ratio):
    """RoIAlignFunction.forward (roi_xfrom/roi_align/functions/roi_align.py:16-32) on
    NCHW features; returns R x C x ah x aw."""
    f = _need(features, "features")
    r = _need(rois, "rois")
    if f.dim() != 4 or r.dim() != 2:
        raise ValueError("features must be 4-D NCHW and rois 2-D")
    B, C, H, W = f.shape
    R = r.shape[0]
    out = torch.empty((R, C, aligned_height, aligned_width), dtype=torch.float32, device=f.device)
    if R == 0:
        return out
    check(lib().vd_roi_align_forward(int(aligned_height), int(aligned_width),
                                     float(spatial_scale), int(sampling_ratio), f.data_ptr(),
                                     B, C, H, W, r.data_ptr(), R, r.shape[1], out.data_ptr(),
                                     _stream()), "vd_roi_align_forward")
    return out


def roi_align_backward(top_grad, rois, feat_shape, spatial_scale, sampling_ratio):
    g = _need(top_grad, "top_grad")
    r = _need(rois, "rois")
    B, C, H, W = feat_shape
    R, _, ah, aw = g.shape
    out = torch.zeros((B, C, H, W), dtype=torch.float32, device=g.device)
    if R == 0:
        return out
    check(lib().vd_roi_align_backward(ah, aw, float(spatial_scale), int(sampling_ratio),
                                      g.data_ptr(), B, C, H, W, r.data_ptr(), R, r.shape[1],
                                      out.data_ptr(), _stream()), "vd_roi_align_backward")
    return out


class _RoIAlignAutograd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, ah, aw, scale, sr):
        ctx.save_for_backward(rois)
        ctx.meta = (tuple(features.shape), scale, sr)
        return roi_align_forward(features, rois, ah, aw, scale, sr)

    @staticmethod
    def backward(ctx, grad_out):
        (rois,) = ctx.saved_tensors
        shape, scale, sr = ctx.meta
        g = roi_align_backward(grad_out, rois, shape, scale, sr)
        return g, None, None, None, None, None


class RoIAlignFunction:
    """Drop-in for the reference's old-style ``RoIAlignFunction(aligned_height,
    aligned_width, spatial_scale, sampling_ratio)(features, rois)``
    (lib/modeling/roi_xfrom/roi_align/functions/roi_align.py:7-48).  The
    reference raises NotImplementedError for CPU tensors (:29-30); so does this
    one (there is no CPU path)."""

    def __init__(self, aligned_height, aligned_width, spatial_scale, sampling_ratio):
        self.aligned_width = int(aligned_width)
        self.aligned_height = int(aligned_height)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)

    def __call__(self, features, rois):
        if not features.is_cuda:
            raise NotImplementedError("RoIAlign has no CPU implementation")
        return _RoIAlignAutograd.apply(features, rois, self.aligned_height, self.aligned_width,
                                       self.spatial_scale, self.sampling_ratio)

    forward = __call__


class RoIAlign(torch.nn.Module):
    """modules/roi_align.py:6-17 counterpart."""

    def __init__(self, aligned_height, aligned_width, spatial_scale, sampling_ratio):
        super().__init__()
        self.fn = RoIAlignFunction(aligned_height, aligned_width, spatial_scale, sampling_ratio)

    def forward(self, features, rois):
        return self.fn(features, rois)


def roi_align_fpn(levels: Sequence[torch.Tensor], spatial_scales: Sequence[float],
                  rois: torch.Tensor, roi_level: Optional[torch.Tensor], resolution: int,
                  sampling_ratio: int, layout: str = "nhwc",
                  roi_order: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, out_layout: str = "nchw") -> torch.Tensor:
    """One-launch multi-level RoIAlign (replaces the per-level loop + cat + restore
    of model_builder.py:252-303).  levels: finest first, each B x H x W x C
    (layout 'nhwc') or B x C x H x W ('nchw', single level only).  roi_level[r]
    is the index into ``levels``.  Output row r belongs to rois[r]; out_layout
    'nchw' -> R x C x P x P (the reference's), 'nhwc' -> R x P x P x C."""
    if len(levels) < 1 or len(levels) > _lib.VD_MAX_LEVELS:
        raise ValueError("1..%d levels" % _lib.VD_MAX_LEVELS)
    r = _need(rois, "rois")
    nhwc = layout == "nhwc"
    if r.dim() != 2 or r.shape[1] != 5:
        raise ValueError("rois must be R x 5, got %s" % (tuple(r.shape),))
    descs = (_lib.VdFeatLevel * len(levels))()
    keep = []
    BC = None
    for i, (t, sc) in enumerate(zip(levels, spatial_scales)):
        t = _need(t, "levels[%d]" % i)
        if t.dim() != 4:
            raise ValueError("levels[%d] must be 4-D" % i)
        keep.append(t)
        if nhwc:
            B, H, W, C = t.shape
        else:
            B, C, H, W = t.shape
        if BC is not None and (B, C) != BC:
            raise ValueError("levels[%d] has B, C = %s; levels[0] has %s" % (i, (B, C), BC))
        BC = (B, C)
        descs[i] = _lib.VdFeatLevel(t.data_ptr(), H, W, float(sc))
    R = r.shape[0]
    onhwc = out_layout == "nhwc"
    shape = (R, resolution, resolution, C) if onhwc else (R, C, resolution, resolution)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=r.device)
    elif (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != r.device):
        raise ValueError("out must be a contiguous float32 %s tensor on %s, got %s %s"
                         % (shape, r.device, tuple(out.shape), out.dtype))
    if R == 0:
        return out
    if roi_level is not None and tuple(roi_level.shape) != (R,):
        raise ValueError("roi_level must have R = %d entries" % R)
    if roi_order is not None and tuple(roi_order.shape) != (R,):
        raise ValueError("roi_order must have R = %d entries" % R)
    lv = _need(roi_level, "roi_level", torch.int32) if roi_level is not None else None
    od = _need(roi_order, "roi_order", torch.int32) if roi_order is not None else None
    if nhwc and onhwc and int(sampling_ratio) == 2 and roi_align_variant() == "30" \
            and (len(levels) == 1 or lv is not None):
        # tile-binned LDS-staged kernel (csrc/roi_align_tile.hip): bit-identical to the
        # reference's per-sample arithmetic; roi_order does not apply (tiles set the order)
        L = len(levels)
        nws = lib().vd_roi_align_fpn_tiled_workspace_size(descs, L, B, C, R, resolution)
        if nws:
            ws = _ws(nws, r.device)
            st = lib().vd_roi_align_fpn_tiled_forward(
                descs, L, B, C, r.data_ptr(), lv.data_ptr() if lv is not None else None, R,
                resolution, 2, out.data_ptr(), ws.data_ptr(), nws, _stream())
            if st != _lib.VD_ERR_SHAPE:
                check(st, "vd_roi_align_fpn_tiled_forward")
                return out
    check(lib().vd_roi_align_fpn_forward(
        descs, len(levels), B, C, _lib.VD_LAYOUT_NHWC if nhwc else _lib.VD_LAYOUT_NCHW,
        r.data_ptr(), lv.data_ptr() if lv is not None else None,
        od.data_ptr() if od is not None else None, R, resolution, resolution,
        int(sampling_ratio), _lib.VD_LAYOUT_NHWC if onhwc else _lib.VD_LAYOUT_NCHW,
        out.data_ptr(), _stream()), "vd_roi_align_fpn_forward")
    return out


_ORDER_CACHE = {}

# FPN RoIAlign kernel for NHWC in/out (VOSDET_ROIALIGN_VARIANT overrides):
# "30" tile-binned LDS-staged (roi_align_tile.hip), "10" register-gather separable
# (roi_align.hip), "3" reference-order rows.
ROI_ALIGN_DEFAULT_VARIANT = "10"


def roi_align_variant() -> str:
    return os.environ.get("VOSDET_ROIALIGN_VARIANT", ROI_ALIGN_DEFAULT_VARIANT)


def _spread16(v: torch.Tensor) -> torch.Tensor:
    """Bits 0..15 of v to the even bit positions 0..30."""
    v = (v | (v << 8)) & 0x00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F
    v = (v | (v << 2)) & 0x33333333
    return (v | (v << 1)) & 0x55555555


def _morton16(y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Z-order index of 16-bit (y, x): x on the even bits, y on the odd bits."""
    return _spread16(x) | (_spread16(y) << 1)


def _deal(n: int, n_xcd: int, window: Optional[int]) -> np.ndarray:
    """Block b -> position in the sorted order: inside each window of `window`
    consecutive positions (the whole order by default), XCD k (b % n_xcd == k)
    takes the k-th contiguous slice."""
    p = np.empty(n, np.int64)
    w = n if not window else int(window)
    for start in range(0, n, w):
        m = min(w, n - start)
        per = -(-m // n_xcd)
        b = np.arange(m)
        slot = (b % n_xcd) * per + b // n_xcd
        ok = slot < m
        q = np.empty(m, np.int64)
        q[ok] = slot[ok]
        q[~ok] = np.setdiff1d(np.arange(m), slot[ok])
        p[start:start + m] = q + start
    return p


def xcd_roi_order(rois: torch.Tensor, roi_level: torch.Tensor, n_xcd: Optional[int] = None,
                  band: int = 8, window: Optional[int] = None,
                  curve: Optional[str] = None) -> torch.Tensor:
    """Scheduling permutation for roi_align_fpn (never changes results): RoIs
    sorted by (image, level, position) and dealt so that the blocks of one XCD
    (b % 8 equal) walk one contiguous slice of that order -- spatial
    neighbours, whose footprints overlap, run on the same L2.  `curve` orders
    the positions: 'band' (y-band of `band` level pixels, then x) or 'morton'
    (Z-order of the level-pixel centre: consecutive RoIs stay inside a square,
    so the RoIs resident on an XCD at one time share more of their footprint;
    tools/research/ra_l2_sim.py models the L2 misses of both).  The default is
    VOSDET_RA_CURVE or 'morton'.  With `window` the dealing restarts every
    `window` positions (e.g. one frame's RoIs), so all XCDs work on the same
    frame at a time; n_xcd=1 is the plain spatial sort."""
    curve = curve or os.environ.get("VOSDET_RA_CURVE", "morton")
    n_xcd = 8 if n_xcd is None else n_xcd
    r = rois
    lv = roi_level.to(torch.int64)
    scale = torch.pow(2.0, -(lv + 2).to(torch.float32))
    cy = (r[:, 2] + r[:, 4]) * 0.5 * scale
    cx = (r[:, 1] + r[:, 3]) * 0.5 * scale
    head = r[:, 0].to(torch.int64) * 8 + lv
    if curve == "band":
        key = (head * 4096 + (cy / band).to(torch.int64)) * 65536 \
            + cx.clamp(0, 65535).to(torch.int64)
    elif curve == "morton":
        key = head * (1 << 32) + _morton16(cy.clamp(0, 65535).to(torch.int64),
                                           cx.clamp(0, 65535).to(torch.int64))
    else:
        raise ValueError("curve must be 'band' or 'morton', got %r" % (curve,))
    srt = torch.argsort(key)
    n = r.shape[0]
    if n_xcd <= 1:
        return srt.to(torch.int32).contiguous()
    perm = _ORDER_CACHE.get((n, n_xcd, window, r.device))
    if perm is None:
        perm = torch.from_numpy(_deal(n, n_xcd, window)).to(r.device)
        _ORDER_CACHE[(n, n_xcd, window, r.device)] = perm
    return srt[perm].to(torch.int32).contiguous()


# --------------------------------------------------------------------------- #
# lib/model ops: legacy RoIAlign, RoIPool, RoICrop                             #
# --------------------------------------------------------------------------- #
def roi_align_legacy(features, rois, aligned_height, aligned_width, spatial_scale):
    """jwyang RoIAlignFunction (lib/model/roi_align/functions/roi_align.py)."""
    f = _need(features, "features")
    r = _need(rois, "rois")
    B, C, H, W = f.shape
    R = r.shape[0]
    out = torch.zeros((R, C, aligned_height, aligned_width), dtype=torch.float32, device=f.device)
    if R:
        check(lib().vd_roi_align_legacy_forward(aligned_height, aligned_width,
                                                float(spatial_scale), f.data_ptr(), B, C, H, W,
                                                r.data_ptr(), R, out.data_ptr(), _stream()),
              "vd_roi_align_legacy_forward")
    return out


class _RoIPoolAutograd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, ph, pw, scale):
        f = _need(features, "features")
        r = _need(rois, "rois")
        B, C, H, W = f.shape
        R = r.shape[0]
        out = torch.zeros((R, C, ph, pw), dtype=torch.float32, device=f.device)
        arg = torch.full((R, C, ph, pw), -1, dtype=torch.int32, device=f.device)
        if R:
            check(lib().vd_roi_pool_forward(ph, pw, float(scale), f.data_ptr(), B, C, H, W,
                                            r.data_ptr(), R, out.data_ptr(), arg.data_ptr(),
                                            _stream()), "vd_roi_pool_forward")
        ctx.save_for_backward(arg)
        ctx.shape = (B, C, H, W)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        (arg,) = ctx.saved_tensors
        g = _need(grad_out, "grad_out")
        bottom = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        check(lib().vd_roi_pool_backward(g.data_ptr(), arg.data_ptr(), g.numel(),
                                         bottom.data_ptr(), _stream()), "vd_roi_pool_backward")
        return bottom, None, None, None, None


class RoIPoolFunction:
    """``RoIPoolFunction(pooled_height, pooled_width, spatial_scale)(features, rois)``
    (lib/model/roi_pooling/functions/roi_pool.py:6-38), CUDA-kernel semantics."""

    def __init__(self, pooled_height, pooled_width, spatial_scale):
        self.pooled_height = int(pooled_height)
        self.pooled_width = int(pooled_width)
        self.spatial_scale = float(spatial_scale)
        self.argmax = None

    def __call__(self, features, rois):
        out, self.argmax = _RoIPoolAutograd.apply(features, rois, self.pooled_height,
                                                  self.pooled_width, self.spatial_scale)
        return out


class RoICropFunction:
    """``RoICropFunction()(input_BCHW, grid_yx)`` (lib/model/roi_crop/functions/roi_crop.py:7-15)."""

    def __call__(self, input1, input2):
        f = _need(input1, "input")
        g = _need(input2, "grid")
        B, C, H, W = f.shape
        R, GH, GW, two = g.shape
        if two != 2:
            raise ValueError("grid must be R x GH x GW x 2 (y, x)")
        out = torch.zeros((R, C, GH, GW), dtype=torch.float32, device=f.device)
        if R:
            check(lib().vd_roi_crop_forward(f.data_ptr(), B, C, H, W, g.data_ptr(), R, GH, GW,
                                            out.data_ptr(), _stream()), "vd_roi_crop_forward")
        return out


# --------------------------------------------------------------------------- #
# NMS / levels                                                                 #
# --------------------------------------------------------------------------- #
def nms(dets: torch.Tensor, thresh: float) -> torch.Tensor:
    """cython_nms.nms semantics on device: dets N x (>=5) fp32 -> kept indices
    (int64, ascending)."""
    d = _need(dets, "dets")
    n = d.shape[0]
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=d.device)
    num = torch.zeros((1,), dtype=torch.int32, device=d.device)
    wsb = lib().vd_nms_workspace_size(n)
    ws = _ws(wsb, d.device)
    check(lib().vd_nms(d.data_ptr() if n else None, n, d.shape[1] if d.dim() == 2 else 5,
                       float(np.float32(thresh)), keep.data_ptr(), num.data_ptr(),
                       ws.data_ptr(), ws.numel(), _stream()), "vd_nms")
    return keep[: int(num.item())]


def soft_nms(dets: torch.Tensor, sigma: float = 0.5, overlap_thresh: float = 0.3,
             score_thresh: float = 0.001, method: str = "linear"):
    """utils.boxes.soft_nms on the device (vd_soft_nms): dets N x (>=5) fp32 ->
    (rows [N',5] with decayed scores in the reference's order, keep int64 [N'])."""
    d = _need(dets, "dets")
    n = d.shape[0]
    if method not in SOFT_NMS_METHODS:
        raise ValueError("Unknown soft_nms method: {}".format(method))  # boxes.py:344
    out = torch.empty((max(n, 1), 5), dtype=torch.float32, device=d.device)
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=d.device)
    num = torch.zeros((1,), dtype=torch.int32, device=d.device)
    check(lib().vd_soft_nms(d.data_ptr() if n else None, n, d.shape[1] if d.dim() == 2 else 5,
                            float(np.float32(sigma)), float(np.float32(overlap_thresh)),
                            float(np.float32(score_thresh)), SOFT_NMS_METHODS[method],
                            out.data_ptr(), keep.data_ptr(), num.data_ptr(), _stream()),
          "vd_soft_nms")
    k = int(num.item())
    return out[:k], keep[:k]


def box_voting(top_dets: torch.Tensor, all_dets: torch.Tensor, thresh: float,
               scoring_method: str = "ID", beta: float = 1.0) -> torch.Tensor:
    """utils.boxes.box_voting on the device (vd_box_voting): top [n,>=5], all
    [m,>=5] fp32 -> [n,5]."""
    t, a = _need(top_dets, "top_dets"), _need(all_dets, "all_dets")
    out = torch.empty((t.shape[0], 5), dtype=torch.float32, device=t.device)
    if t.shape[0]:
        check(lib().vd_box_voting(t.data_ptr(), t.shape[0], t.shape[1], a.data_ptr(),
                                  a.shape[0], a.shape[1], float(np.float32(thresh)),
                                  bbox_vote_method(scoring_method, beta), float(beta),
                                  out.data_ptr(), _stream()), "vd_box_voting")
    return out


def map_rois_to_fpn_levels(rois: torch.Tensor, k_min: int, k_max: int, col0: int = 1,
                           canonical_scale: float = 224., canonical_level: float = 4.):
    """utils/fpn.py:11-28 on device; returns int32 levels (k_min..k_max)."""
    r = _need(rois, "rois")
    R = r.shape[0]
    out = torch.empty((R,), dtype=torch.int32, device=r.device)
    if R:
        check(lib().vd_map_rois_to_fpn_levels(r.data_ptr(), r.shape[1], col0, R, k_min, k_max,
                                              float(canonical_scale), float(canonical_level),
                                              out.data_ptr(), _stream()),
              "vd_map_rois_to_fpn_levels")
    return out


def mask_rois(dets: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor,
              im_scale: torch.Tensor, rows: int, k_min: int, k_max: int, row0: int = 0,
              canonical_scale: float = 224., canonical_level: float = 4.):
    """The mask-head batch of all frames without a host read (vd_mask_rois):
    dets [F, D, 5], classes [F, D] int32, counts [F] int32, im_scale [F] float64
    -> rois [rows, 5], levels [rows] (level - k_min), classes [rows] int32 and the
    device total [1] int32; global rows [row0, row0 + rows), frame-major, padding
    past the total."""
    d, c, n = _need(dets, "dets"), _need(classes, "classes", torch.int32), \
        _need(counts, "counts", torch.int32)
    sc = _need(im_scale, "im_scale", torch.float64)
    F, D = d.shape[0], d.shape[1]
    if tuple(c.shape) != (F, D) or n.numel() != F or sc.numel() != F:
        raise ValueError("mask_rois: dets %s classes %s counts %s im_scale %s"
                         % (tuple(d.shape), tuple(c.shape), tuple(n.shape), tuple(sc.shape)))
    rois = torch.empty((rows, 5), dtype=torch.float32, device=d.device)
    lvl = torch.empty((rows,), dtype=torch.int32, device=d.device)
    cls = torch.empty((rows,), dtype=torch.int32, device=d.device)
    total = torch.empty((1,), dtype=torch.int32, device=d.device)
    check(lib().vd_mask_rois(d.data_ptr(), c.data_ptr(), n.data_ptr(), F, D, sc.data_ptr(),
                             int(row0), int(rows), k_min, k_max, float(canonical_scale),
                             float(canonical_level), rois.data_ptr(), lvl.data_ptr(),
                             cls.data_ptr(), total.data_ptr(), _stream()), "vd_mask_rois")
    return rois, lvl, cls, total


def nchw_to_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    t = _need(x, "x")
    B, C, H, W = t.shape
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=t.device)
    check(lib().vd_nchw_to_nhwc(t.data_ptr(), B, C, H, W, out.data_ptr(), _stream()),
          "vd_nchw_to_nhwc")
    return out


def bias_act_(x: torch.Tensor, bias: Optional[torch.Tensor], residual=None, residual_bias=None,
              relu: bool = True, upsample_residual: bool = False) -> torch.Tensor:
    """In-place conv epilogue x = act((x + bias) + residual[+residual_bias]) (vd_bias_act).
    x: N x C x H x W, contiguous or channels_last; residual in the same memory format."""
    N, C, H, W = x.shape
    if x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        nhwc = 1
    elif x.is_contiguous():
        nhwc = 0
    else:
        raise ValueError("x must be contiguous (NCHW or channels_last)")
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("x must be a float32 device tensor")
    for v in (bias, residual_bias):
        if v is not None and (v.numel() != C or not v.is_contiguous() or v.dtype != torch.float32):
            raise ValueError("bias vectors must be contiguous float32 of length C")
    mode = 0
    if residual is not None:
        mode = 2 if upsample_residual else 1
        want_shape = (N, C, H // 2, W // 2) if upsample_residual else (N, C, H, W)
        if tuple(residual.shape) != want_shape or residual.dtype != torch.float32:
            raise ValueError("residual shape %s, expected %s" % (tuple(residual.shape),
                                                                 want_shape))
        want = torch.channels_last if nhwc else torch.contiguous_format
        if not residual.is_contiguous(memory_format=want):
            residual = residual.contiguous(memory_format=want)
    check(lib().vd_bias_act(x.data_ptr(), bias.data_ptr() if bias is not None else None,
                            residual.data_ptr() if residual is not None else None,
                            residual_bias.data_ptr() if residual_bias is not None else None,
                            N, C, H, W, nhwc, mode, int(relu), _stream()), "vd_bias_act")
    return x


_GEMM_WS = {}


def gemm_workspace(device) -> torch.Tensor:
    """The hipBLASLt workspace for one vd_gemm_bias_act launch.  Algorithms with
    a workspace keep inter-workgroup state in it (split-K partials, stream-K
    fix-up flags; vd_gemm_plan_list shows which plans use one), so two GEMMs
    that can run at the same time must not share it.  A captured step bakes the
    pointer into its graph: the two captured steps of bench.capture_graphs,
    replayed concurrently on two streams, shared the one per-device workspace of
    round 4 and stopped making progress.  So:
      * while the current stream is capturing, every call takes its workspace
        from the graph's private memory pool (freed after the call, the caching
        allocator hands the same block to the next GEMM of the same capture:
        one workspace per graph, stream-ordered inside it);
      * eager launches use one workspace per (device, stream)."""
    device = torch.device(device)
    if torch.cuda.is_current_stream_capturing():
        return _ws(lib().vd_gemm_workspace_size(), device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _GEMM_WS.get(key)
    if ws is None:
        ws = _GEMM_WS[key] = _ws(lib().vd_gemm_workspace_size(), device)
    return ws


def gemm_plan_list() -> list:
    """(M, N, K, relu, has_res, 'own' | 'blas', workspace_bytes) for every GEMM
    shape this process has planned (vd_gemm_plan_list)."""
    n = 1 << 16
    while True:
        buf = ctypes.create_string_buffer(n)
        st = lib().vd_gemm_plan_list(buf, n)
        if st != _lib.VD_ERR_WORKSPACE:
            break
        n *= 4
    check(st, "vd_gemm_plan_list")
    rows = []
    for line in buf.value.decode().splitlines():
        M, N, K, relu, res, what, ws = line.split()
        rows.append((int(M), int(N), int(K), int(relu), int(res), what, int(ws)))
    return rows


# K from which a GEMM with a split-bf16 route runs it there (gemm_split3_bias_act):
# below it the GEMMs are HBM-bound and the fp32 kernels are as fast
# (profiles/r06/gemm_split3/)
SPLIT3_MIN_K = 128
# (transform, id(weight tensor)) -> (weakref to it, key, transformed weight); an entry
# leaves with its tensor
_weight_cache = {}


def split3_enabled() -> bool:
    """VOSDET_GEMM_SPLIT3=0 keeps every GEMM on the fp32-MFMA kernels (A/B runs)."""
    return os.environ.get("VOSDET_GEMM_SPLIT3", "1") != "0"


def _weight_cached(w: torch.Tensor, transform, trace: Optional[str] = None):
    """transform(w), made once per weight tensor object (callers such as gemm_bias_act
    hold a bare weight, no module to keep it on) and remade when the tensor changes (its
    storage, version counter or shape: an in-place update, load_state_dict)."""
    key = (w.data_ptr(), w._version, tuple(w.shape))
    slot = (transform, id(w))
    ent = _weight_cache.get(slot)
    if ent is not None and ent[0]() is w and ent[1] == key:
        return ent[2]
    def _drop(r, slot=slot):
        if _weight_cache.get(slot, (None,))[0] is r:
            del _weight_cache[slot]
    ref = weakref.ref(w, _drop)
    if trace is not None and os.environ.get(trace) == "1":  # research: report every remake
        import traceback
        sys.stderr.write("%s %s (cache %s)\n%s" % (
            transform.__name__, tuple(w.shape), "stale" if ent is not None else "miss",
            "".join(traceback.format_stack(limit=7)[:-2])))
    wp = transform(w)
    _weight_cache[slot] = (ref, key, wp)
    return wp


def split3_weight_cached(w: torch.Tensor) -> Optional[torch.Tensor]:
    """gemm_split3_weight(w) through _weight_cached (VOSDET_SPLIT3_TRACE=1 reports each)."""
    return _weight_cached(w, gemm_split3_weight, "VOSDET_SPLIT3_TRACE")


def h2_enabled() -> bool:
    """VOSDET_GEMM_H2=0 keeps the split GEMMs on the six-product bf16 kernel (A/B runs);
    VOSDET_GEMM_SPLIT3=0 switches both schemes off."""
    return split3_enabled() and os.environ.get("VOSDET_GEMM_H2", "1") != "0"


def h2_route(M: int, N: int, K: int) -> bool:
    """A split GEMM whose caller asks for the two-piece fp16 scheme (gemm_h2_bias_act)
    runs there: a function of the shape alone, so a captured graph replays what it
    captured.  From K = SPLIT3_MIN_K (below it the fp16 pieces' representation error
    shows, and those GEMMs are HBM-bound).  Every shape class of the 64-frame step is
    faster there, the HBM-bound K = 256 -> 64 res2 conv1 by 1.1x
    (profiles/gemm_h2/README.md), so no class is held back."""
    return h2_enabled() and K >= SPLIT3_MIN_K and K % 16 == 0 and N % 64 == 0 and M > 0


def h2_weight_cached(w: torch.Tensor) -> Optional[torch.Tensor]:
    """gemm_h2_weight(w) through _weight_cached (VOSDET_SPLIT3_TRACE=1 reports each)."""
    return _weight_cached(w, gemm_h2_weight, "VOSDET_SPLIT3_TRACE")


def split_gemm_bias_act(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, h2: bool = False,
                        **kw) -> Optional[torch.Tensor]:
    """gemm_split3_bias_act of the weight tensor w [N, K] (its image cached per tensor),
    or with h2 and h2_route(M, N, K) gemm_h2_bias_act.  M is the output row count (a
    quarter of a's rows with sub_hw).  None when the shape is not served."""
    N, K = w.shape[0], w[0].numel()
    M = a.shape[0]
    if kw.get("sub_hw") is not None:
        sh, sw = kw["sub_hw"]
        M = M // (sh * sw) * ((sh + 1) // 2) * ((sw + 1) // 2)
    if h2 and h2_route(M, N, K):
        wp = h2_weight_cached(w)
        return None if wp is None else gemm_h2_bias_act(a, wp, bias, **kw)
    wp = split3_weight_cached(w)
    return None if wp is None else gemm_split3_bias_act(a, wp, bias, **kw)


def gemm_bias_act(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor,
                  residual: Optional[torch.Tensor] = None, relu: bool = True,
                  out: Optional[torch.Tensor] = None,
                  a_bias: Optional[torch.Tensor] = None, h2: bool = False) -> torch.Tensor:
    """act(a @ w.T + bias (+ residual)) in one GEMM launch: a [M,K], w [N,K], bias [N],
    residual / out [M,N], all fp32 contiguous.  From K = SPLIT3_MIN_K (N a multiple
    of 64) on the bf16 matrix cores at fp32 accuracy (gemm_split3_bias_act, the
    weight's split image cached per tensor); otherwise vd_gemm_bias_act (hipBLASLt
    with the epilogue fused, or the hand-written fp32 MFMA kernel where it is
    faster).  h2: the split GEMM on the two-piece fp16 scheme where h2_route serves the
    shape (the engine's layers ask for it; activations within gemm_h2_bias_act's input
    contract).  a_bias [K]: a enters as relu(a + a_bias) (fused into the split GEMM's A
    load; a separate pass before the other kernels).  Returns None when nothing serves
    the shape (the caller falls back, a_bias not applied)."""
    a_ = _need(a, "a")
    w_ = _need(w, "w")
    b_ = _need(bias, "bias")
    M, K = a_.shape
    N = w_.shape[0]
    if w_.shape[1] != K or b_.numel() != N:
        raise ValueError("gemm_bias_act: a %s, w %s, bias %s" % (tuple(a_.shape), tuple(w_.shape),
                                                                 tuple(b_.shape)))
    r_ = None
    if residual is not None:
        r_ = _need(residual, "residual")
        if tuple(r_.shape) != (M, N):
            raise ValueError("residual must be %s, got %s" % ((M, N), tuple(r_.shape)))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a_.device)
    elif tuple(out.shape) != (M, N) or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor" % ((M, N),))
    if K >= SPLIT3_MIN_K and N % 64 == 0 and K % 16 == 0 and M > 0 and split3_enabled():
        y = split_gemm_bias_act(a_, w if w.is_contiguous() else w_, b_, h2=h2, residual=r_,
                                relu=relu, out=out, a_bias=a_bias)
        if y is not None:
            return y
    if a_bias is not None:
        a_ = torch.relu(a_ + _need(a_bias, "a_bias"))
    if os.environ.get("VOSDET_GEMM_TRACE") == "1":  # research: the fp32-kernel GEMMs
        sys.stderr.write("fp32 gemm M=%d N=%d K=%d res=%d\n" % (M, N, K, r_ is not None))
    ws = gemm_workspace(a_.device)
    st = lib().vd_gemm_bias_act(a_.data_ptr(), M, K, w_.data_ptr(), N, b_.data_ptr(),
                                r_.data_ptr() if r_ is not None else None, int(relu),
                                out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    if st == VD_ERR_SHAPE:  # no hipBLASLt algorithm and no MFMA kernel for the shape
        return None
    check(st, "vd_gemm_bias_act")
    return out


def gemm_split3_weight(w: torch.Tensor) -> Optional[torch.Tensor]:
    """W [N, K] fp32 (a 1x1 conv / Linear weight) -> the three-piece bf16 split image
    vd_gemm_split3_bias_act reads (once per model; N * K * 6 bytes).  None when the
    shape is not served (K a multiple of 32, N of 64)."""
    w_ = _need(w.reshape(w.shape[0], -1), "w")
    N, K = w_.shape
    nbytes = lib().vd_gemm_split3_weight_size(N, K)
    if not nbytes:
        return None
    wp = torch.empty(nbytes, dtype=torch.uint8, device=w_.device)
    check(lib().vd_gemm_split3_weight(w_.data_ptr(), N, K, wp.data_ptr(), _stream()),
          "vd_gemm_split3_weight")
    wp.split3_shape = (N, K)
    return wp


def gemm_split3_bias_act(a: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor,
                         residual: Optional[torch.Tensor] = None, relu: bool = True,
                         out: Optional[torch.Tensor] = None, cfg: int = 0,
                         up_hw: Optional[Sequence[int]] = None,
                         sub_hw: Optional[Sequence[int]] = None,
                         a2: Optional[torch.Tensor] = None,
                         a_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(a @ w.T + bias (+ residual)) with the fp32 operands split into three bf16
    pieces on the bf16 matrix cores (vd_gemm_split3_bias_act, fp32 accuracy):
    a [M,K], wp from gemm_split3_weight(w [N,K]), bias [N], out [M,N]; residual
    [M,N], or with up_hw = (H, W) the top-down map [M / (H W), H/2, W/2, N] of an
    FPN level added at the nearest-2x row of each pixel (FPN.py:292-300).  With
    sub_hw = (H, W): a is an images x H x W map's rows [images H W, K] read at
    stride 2, M = images x ceil(H/2) x ceil(W/2) output rows (a stride-2 1x1 conv).
    With a2 [M, K2]: w's last K2 input channels multiply a2 (a is [M, K - K2]): two
    1x1 convs of two inputs summed in one GEMM.  With a_bias [K - K2]: a enters as
    relu(a + a_bias) (the producing layer's bias + ReLU, fused into the A load)."""
    return _split_gemm("vd_gemm_split3_bias_act", wp.split3_shape, a, wp, bias, residual, relu,
                       out, cfg, up_hw, sub_hw, a2, a_bias)


def gemm_h2_weight(w: torch.Tensor) -> Optional[torch.Tensor]:
    """W [N, K] fp32 -> the image vd_gemm_h2_bias_act reads (once per weight): the three
    fp16 images Wm, Wr, W0 of the row-scaled weight in the kernel's fragment order
    (N * K * 6 bytes), then the N fp32 row scales 1 / (2^11 r_n).  None when the shape is
    not served (K a multiple of 16, N of 64)."""
    w_ = _need(w.reshape(w.shape[0], -1), "w")
    N, K = w_.shape
    nbytes = lib().vd_gemm_h2_weight_size(N, K)
    if not nbytes:
        return None
    wp = torch.empty(nbytes, dtype=torch.uint8, device=w_.device)
    check(lib().vd_gemm_h2_weight(w_.data_ptr(), N, K, wp.data_ptr(), _stream()),
          "vd_gemm_h2_weight")
    wp.h2_shape = (N, K)
    return wp


def gemm_h2_bias_act(a: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor,
                     residual: Optional[torch.Tensor] = None, relu: bool = True,
                     out: Optional[torch.Tensor] = None, cfg: int = 0,
                     up_hw: Optional[Sequence[int]] = None,
                     sub_hw: Optional[Sequence[int]] = None,
                     a2: Optional[torch.Tensor] = None,
                     a_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gemm_split3_bias_act with three fp16 products per fp32 product instead of six
    bf16 ones (vd_gemm_h2_bias_act; wp from gemm_h2_weight): a = a0 + a1 / 2^11 in two
    fp16 pieces, the row-scaled weight in three fp16 images, one accumulator.  Same
    arguments.  At fp32's error level for activations whose largest magnitude lies in
    [2^-10, 65504]; a larger activation gives a non-finite output row (include/vosdet.h)."""
    return _split_gemm("vd_gemm_h2_bias_act", wp.h2_shape, a, wp, bias, residual, relu, out,
                       cfg, up_hw, sub_hw, a2, a_bias)


def _split_gemm(entry, shape, a, wp, bias, residual, relu, out, cfg, up_hw, sub_hw, a2, a_bias):
    """The argument checks and the launch of gemm_split3_bias_act / gemm_h2_bias_act."""
    a_ = _need(a, "a")
    N, K = shape
    M = a_.shape[0]
    K2, a2_ = 0, None
    if a2 is not None:
        a2_ = _need(a2, "a2")
        K2 = a2_.shape[1]
        if a2_.shape[0] != M or a_.shape[1] + K2 != K or K2 % 16 or sub_hw is not None:
            raise ValueError("%s: a %s + a2 %s vs w (%d, %d)"
                             % (entry[3:], tuple(a_.shape), tuple(a2_.shape), N, K))
    sh = sw = 0
    if sub_hw is not None:
        sh, sw = int(sub_hw[0]), int(sub_hw[1])
        if sh < 1 or sw < 1 or M % (sh * sw):
            raise ValueError("a %s is not a stack of %s maps" % (tuple(a_.shape), (sh, sw)))
        M = M // (sh * sw) * ((sh + 1) // 2) * ((sw + 1) // 2)
    b_ = _need(bias, "bias")
    if a_.dim() != 2 or a_.shape[1] + K2 != K or b_.numel() != N:
        raise ValueError("%s: a %s, w (%d, %d), bias %s"
                         % (entry[3:], tuple(a_.shape), N, K, tuple(b_.shape)))
    ab_ = None
    if a_bias is not None:
        ab_ = _need(a_bias, "a_bias")
        if ab_.numel() != K - K2:
            raise ValueError("a_bias must have %d entries, got %d" % (K - K2, ab_.numel()))
    r_ = None
    uh = uw = 0
    if residual is not None:
        r_ = _need(residual, "residual")
        if up_hw is not None:
            uh, uw = int(up_hw[0]), int(up_hw[1])
            if uh % 2 or uw % 2 or uh < 2 or uw < 2 or M % (uh * uw) or \
                    r_.numel() != (M // 4) * N:
                raise ValueError("top-down map %s does not match %d pixels of %s maps"
                                 % (tuple(r_.shape), M, (uh, uw)))
        elif tuple(r_.shape) != (M, N):
            raise ValueError("residual must be %s, got %s" % ((M, N), tuple(r_.shape)))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a_.device)
    elif tuple(out.shape) != (M, N) or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor" % ((M, N),))
    check(getattr(lib(), entry)(a_.data_ptr(), M, K,
                                a2_.data_ptr() if a2_ is not None else None, K2,
                                ab_.data_ptr() if ab_ is not None else None,
                                wp.data_ptr(), N, b_.data_ptr(),
                                r_.data_ptr() if r_ is not None else None, uh, uw,
                                sh, sw, int(relu), out.data_ptr(), int(cfg), _stream()),
          entry)
    return out


def mask_head_upconv_logits(x: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor,
                            cls_w: torch.Tensor, cls_b: torch.Tensor, roi_ch: torch.Tensor,
                            P: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mask head's upconv5 + ReLU and the class-selected mask logits + sigmoid in one
    split-bf16 launch (vd_mask_head_upconv_logits): x [R P P, 256] NHWC RoI map rows,
    wp = gemm_split3_weight of the upconv weight as [(i, j, co), 256], bias [1024],
    cls_w [classes, 256], cls_b [classes], roi_ch [R] (int32 class channels).  Returns
    [R, 2P, 2P] mask probabilities.  A wp from gemm_h2_weight runs the two-piece fp16
    scheme (vd_mask_head_upconv_logits_h2)."""
    x_ = _need(x, "x")
    R = int(roi_ch.numel())
    h2 = hasattr(wp, "h2_shape")
    shape = wp.h2_shape if h2 else wp.split3_shape
    entry = "vd_mask_head_upconv_logits_h2" if h2 else "vd_mask_head_upconv_logits"
    if x_.dim() != 2 or x_.shape[0] != R * P * P or tuple(shape) != (1024, x_.shape[1]):
        raise ValueError("mask_head_upconv_logits: x %s, %d RoIs of %d x %d, w %s"
                         % (tuple(x_.shape), R, P, P, shape))
    cw = _need(cls_w, "cls_w")
    if cw.dim() != 2 or cw.shape[1] != 256:
        raise ValueError("cls_w must be [classes, 256], got %s" % (tuple(cw.shape),))
    ch = _need(roi_ch, "roi_ch", torch.int32)
    if out is None:
        out = torch.empty((R, 2 * P, 2 * P), dtype=torch.float32, device=x_.device)
    check(getattr(lib(), entry)(x_.data_ptr(), x_.shape[0], x_.shape[1], wp.data_ptr(),
                                _need(bias, "bias").data_ptr(), cw.data_ptr(),
                                _need(cls_b, "cls_b").data_ptr(), ch.data_ptr(), P,
                                out.data_ptr(), _stream()),
          entry)
    return out


def conv3x3_weight(w: torch.Tensor) -> torch.Tensor:
    """PyTorch conv weight [Cout][Cin][3][3] -> the [Cout][3][3][Cin] layout
    vd_conv3x3_bias_act reads (once per model, at prepare time)."""
    return w.permute(0, 2, 3, 1).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _conv3x3_x(x: torch.Tensor):
    """The conv3x3_*_bias_act entries' check of x; its (N, C, H, W)."""
    if x.dim() != 4 or not x.is_cuda or x.dtype != torch.float32 \
            or not x.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("x must be a channels_last fp32 device tensor")
    return x.shape


def _conv3x3_bias_out(x: torch.Tensor, bias, Cout: int, out):
    """The rest of those entries' preamble, once the weight operand has given Cout:
    (the bias as _need gives it or None, `out` -- allocated, or checked where given)."""
    b_ = _need(bias, "bias") if bias is not None else None
    if b_ is not None and b_.numel() != Cout:
        raise ValueError("bias must have %d elements" % Cout)
    shape = (x.shape[0], Cout, x.shape[2], x.shape[3])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device,
                          memory_format=torch.channels_last)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device \
            or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("out must be a channels_last fp32 %s tensor on x's device" % (shape,))
    return b_, out


def _conv3x3_done(st: int, out: torch.Tensor, what: str):
    """Those entries' tail: None for a shape the kernel does not serve (the caller falls
    back), any other failure raises."""
    if st == VD_ERR_SHAPE:
        return None
    check(st, what)
    return out


def conv3x3_bias_act(x: torch.Tensor, w2: torch.Tensor, bias: Optional[torch.Tensor],
                     relu: bool = False, out: Optional[torch.Tensor] = None):
    """act(conv3x3(x, pad 1) + bias) on a channels_last fp32 tensor in one MFMA
    implicit-GEMM kernel (vd_conv3x3_bias_act); w2 from conv3x3_weight.  Returns
    None for a shape the kernel does not serve (the caller falls back)."""
    N, C, H, W = _conv3x3_x(x)
    w_ = _need(w2, "w2")
    Cout = w_.shape[0]
    if tuple(w_.shape) != (Cout, 3, 3, C):
        raise ValueError("w2 must be [Cout][3][3][Cin], got %s" % (tuple(w_.shape),))
    b, out = _conv3x3_bias_out(x, bias, Cout, out)
    return _conv3x3_done(lib().vd_conv3x3_bias_act(
        x.data_ptr(), N, H, W, C, w_.data_ptr(), Cout, _ptr(b), int(relu), out.data_ptr(),
        _stream()), out, "vd_conv3x3_bias_act")


WINO_MAX_CIN = 4096  # csrc/conv3x3_wino.hip: the zero lanes' DMA source holds 4096 floats


def wino_serves(Cin: int, Cout: int) -> bool:
    """The channel counts both Winograd kernels serve: Cout in 64-channel blocks, Cin in
    8-channel MFMA steps up to WINO_MAX_CIN.  One rule for the weight transforms below
    and for modeling's route functions."""
    return Cout > 0 and Cin > 0 and Cout % 64 == 0 and Cin % 8 == 0 and Cin <= WINO_MAX_CIN


def conv3x3_wino_weight(w: torch.Tensor) -> Optional[torch.Tensor]:
    """PyTorch conv weight [Cout][Cin][3][3] -> the Winograd F(2x2,3x3) operand
    U = G g G^T in the kernel's register-fragment order [Cout/64][Cin/8][2][16][64][4]
    (32-channel group, fragment, lane, 2 positions x 2 channels;
    vd_conv3x3_wino_weight; once per model).  None for
    a shape the kernel does not serve (Cout % 64, Cin % 8, Cin > WINO_MAX_CIN)."""
    w_ = _need(w, "w")
    if w_.dim() != 4 or tuple(w_.shape[2:]) != (3, 3):
        raise ValueError("conv3x3_wino_weight: weight %s" % (tuple(w_.shape),))
    Cout, C = w_.shape[:2]
    if not wino_serves(C, Cout):
        return None
    u = torch.empty((Cout // 64, C // 8, 2, 16, 64, 4), dtype=torch.float32, device=w_.device)
    check(lib().vd_conv3x3_wino_weight(w_.data_ptr(), Cout, C, u.data_ptr(), _stream()),
          "vd_conv3x3_wino_weight")
    return u


def conv3x3_wino_bias_act(x: torch.Tensor, u: torch.Tensor, bias: Optional[torch.Tensor],
                          relu: bool = False, out: Optional[torch.Tensor] = None,
                          mosaic: bool = False):
    """act(conv3x3(x, pad 1) + bias) on a channels_last fp32 tensor by Winograd
    F(2x2,3x3) on the MFMA pipes (vd_conv3x3_wino_bias_act); u from
    conv3x3_wino_weight.  mosaic=True runs the N images as one N*H-row image with
    per-image zero padding (vd_conv3x3_wino_seg_bias_act; H even): bit-identical,
    fewer idle block rows on small maps.  mosaic="2d" also packs maps side by side
    (vd_conv3x3_wino_mosaic_bias_act; an odd side padded by a phantom row / column
    per map): no idle block columns either.
    Returns None for a shape the kernel does not serve."""
    N, C, H, W = _conv3x3_x(x)
    if u is None:
        return None
    u_ = _need(u, "u")
    if u_.dim() != 6 or tuple(u_.shape[1:]) != (C // 8, 2, 16, 64, 4) or C % 8:
        raise ValueError("u must be [Cout/64][%d][2][16][64][4], got %s" % (C // 8, tuple(u_.shape)))
    Cout = u_.shape[0] * 64
    b, out = _conv3x3_bias_out(x, bias, Cout, out)
    if mosaic == "2d" and N > 0:
        st = lib().vd_conv3x3_wino_mosaic_bias_act(x.data_ptr(), N, H, W, C, u_.data_ptr(), Cout,
                                                   _ptr(b), int(relu), out.data_ptr(), _stream())
    elif mosaic and N > 0:
        st = lib().vd_conv3x3_wino_seg_bias_act(x.data_ptr(), N * H, W, C, u_.data_ptr(), Cout,
                                                _ptr(b), int(relu), H, out.data_ptr(), _stream())
    else:
        st = lib().vd_conv3x3_wino_bias_act(x.data_ptr(), N, H, W, C, u_.data_ptr(), Cout,
                                            _ptr(b), int(relu), out.data_ptr(), _stream())
    return _conv3x3_done(st, out, "vd_conv3x3_wino_bias_act")


def conv3x3_wino4_weight(w: torch.Tensor) -> Optional[torch.Tensor]:
    """PyTorch conv weight [Cout][Cin][3][3] -> the Winograd F(4x4,3x3) operand
    U = G g G^T (6 x 6 positions) in the kernel's fragment order
    [Cout/64][Cin/8][4][18][64][4] (vd_conv3x3_wino4_weight; once per model).  None
    for a shape the kernel does not serve."""
    w_ = _need(w, "w")
    if w_.dim() != 4 or tuple(w_.shape[2:]) != (3, 3):
        raise ValueError("conv3x3_wino4_weight: weight %s" % (tuple(w_.shape),))
    Cout, C = w_.shape[:2]
    if not wino_serves(C, Cout):
        return None
    u = torch.empty((Cout // 64, C // 8, 4, 18, 64, 4), dtype=torch.float32, device=w_.device)
    check(lib().vd_conv3x3_wino4_weight(w_.data_ptr(), Cout, C, u.data_ptr(), _stream()),
          "vd_conv3x3_wino4_weight")
    return u


def conv3x3_wino4_grouped_weight(w: torch.Tensor, groups: int) -> Optional[torch.Tensor]:
    """A grouped conv's weight [C][C / groups][3][3] (C / groups dividing 64) -> U for
    vd_conv3x3_wino4_grouped_bias_act: the block-diagonal expansion to [C][64][3][3]
    (each output channel's 64-channel input block, zeros outside its group) through
    conv3x3_wino4_weight (once per model).  None for a shape the kernel does not serve."""
    w_ = _need(w, "w")
    C, cpg = int(w_.shape[0]), int(w_.shape[1])
    if groups < 2 or cpg * groups != C or C % 64 or 64 % cpg or tuple(w_.shape[2:]) != (3, 3):
        return None
    G = 64 // cpg  # groups per 64-channel block
    wd = torch.zeros((C // 64, G, cpg, G, cpg, 3, 3), dtype=w_.dtype, device=w_.device)
    wg = w_.view(C // 64, G, cpg, cpg, 3, 3)
    for i in range(G):
        wd[:, i, :, i] = wg[:, i]
    return conv3x3_wino4_weight(wd.view(C, 64, 3, 3))


def conv3x3_wino4_bias_act(x: torch.Tensor, u: torch.Tensor, bias: Optional[torch.Tensor],
                           relu: bool = False, out: Optional[torch.Tensor] = None,
                           mosaic=False, groups: int = 1):
    """act(conv3x3(x, pad 1) + bias) on a channels_last fp32 tensor by Winograd
    F(4x4,3x3) (vd_conv3x3_wino4_bias_act); u from conv3x3_wino4_weight.  mosaic
    True / "pair": maps of at most 15 x 15 two per output block
    (vd_conv3x3_wino4_mosaic_bias_act); "rows": the maps stacked at tile-aligned
    pitches, block shape and maps per stack row from the block plan
    (vd_conv3x3_wino4_rows_bias_act, conv3x3_wino4_plan); both bit-identical.  "grid": the
    maps as a 2-D grid at an (H + 1) x (W + 1) pitch (vd_conv3x3_wino4_grid_bias_act;
    equal within Winograd rounding).  groups > 1: a grouped conv (u from
    conv3x3_wino4_grouped_weight; mosaic False or "rows").  None for a shape the kernel
    does not serve."""
    N, C, H, W = _conv3x3_x(x)
    if u is None:
        return None
    u_ = _need(u, "u")
    if groups > 1:
        if u_.dim() != 6 or tuple(u_.shape) != (C // 64, 8, 4, 18, 64, 4) or C % 64:
            raise ValueError("grouped u must be [%d][8][4][18][64][4], got %s"
                             % (C // 64, tuple(u_.shape)))
        if mosaic not in (False, None, "rows"):
            return None
        b, out = _conv3x3_bias_out(x, bias, C, out)
        return _conv3x3_done(lib().vd_conv3x3_wino4_grouped_bias_act(
            x.data_ptr(), N, H, W, C, u_.data_ptr(), int(groups), _ptr(b), int(relu),
            out.data_ptr(), int(mosaic == "rows"), _stream()), out,
            "vd_conv3x3_wino4_grouped_bias_act")
    if u_.dim() != 6 or tuple(u_.shape[1:]) != (C // 8, 4, 18, 64, 4) or C % 8:
        raise ValueError("u must be [Cout/64][%d][4][18][64][4], got %s" % (C // 8, tuple(u_.shape)))
    Cout = u_.shape[0] * 64
    b, out = _conv3x3_bias_out(x, bias, Cout, out)
    fn = {False: lib().vd_conv3x3_wino4_bias_act, True: lib().vd_conv3x3_wino4_mosaic_bias_act,
          "pair": lib().vd_conv3x3_wino4_mosaic_bias_act,
          "rows": lib().vd_conv3x3_wino4_rows_bias_act,
          "grid": lib().vd_conv3x3_wino4_grid_bias_act}[mosaic]
    return _conv3x3_done(fn(x.data_ptr(), N, H, W, C, u_.data_ptr(), Cout, _ptr(b), int(relu),
                            out.data_ptr(), _stream()), out,
                         "vd_conv3x3_wino4_bias_act (mosaic %r)" % (mosaic,))


def conv3x3_wino4_plan(N: int, H: int, W: int, C: int, Cout: int, stacked: bool, n_cu: int):
    """The block plan of a conv3x3_wino4_bias_act launch (vd_conv3x3_wino4_plan; no GPU
    needed): (shape "wide" 16 x 32 / "tall" 32 x 16, maps per stack row, spatial blocks,
    rounds of workgroups over n_cu compute units).  stacked: the "rows" entries (dense
    or grouped), else the plain entry.  Honours VOSDET_WINO4_PLAN like the launch."""
    out = (ctypes.c_int * 4)()
    check(lib().vd_conv3x3_wino4_plan(int(N), int(H), int(W), int(C), int(Cout), int(bool(stacked)),
                                      int(n_cu), out), "vd_conv3x3_wino4_plan")
    return ("tall" if out[0] else "wide", int(out[1]), int(out[2]), int(out[3]))


def conv3x3_wino4_dilated2_bias_act(x: torch.Tensor, u: torch.Tensor,
                                    bias: Optional[torch.Tensor], relu: bool = False,
                                    out: Optional[torch.Tensor] = None, layout=False):
    """act(conv3x3(x, dilation 2, pad 2) + bias) of channels_last fp32 maps (H, W even)
    on the F(4x4) kernel as the plain conv of the polyphase sub-maps, read and written in
    place (vd_conv3x3_wino4_dilated2_bias_act); u from conv3x3_wino4_weight.  None for a
    shape the kernel does not serve.  layout: the sub-maps' block layout, False (one
    per block), "pair" (pairs / octets) or "grid"."""
    N, C, H, W = _conv3x3_x(x)
    lay = {False: 0, None: 0, "pair": 1, True: 1, "grid": 2}.get(layout)
    if lay is None:
        return None
    u_ = _need(u, "u")
    if u_.dim() != 6 or tuple(u_.shape[1:]) != (C // 8, 4, 18, 64, 4) or C % 8 or H % 2 or W % 2:
        return None
    if lay == 1 and (H > 30 or W > 30):  # pairs / octets hold sub-maps of at most 15 x 15
        return None
    Cout = u_.shape[0] * 64
    b, out = _conv3x3_bias_out(x, bias, Cout, out)
    return _conv3x3_done(lib().vd_conv3x3_wino4_dilated2_bias_act(
        x.data_ptr(), N, H, W, C, u_.data_ptr(), Cout, _ptr(b), int(relu), out.data_ptr(), lay,
        _stream()), out, "vd_conv3x3_wino4_dilated2_bias_act")


def gemm_dual_bias_act(a1: torch.Tensor, a2: torch.Tensor, w: torch.Tensor, bias: torch.Tensor,
                       relu: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(a1 @ w[:, :K1].T + a2 @ w[:, K1:].T + bias) in one MFMA kernel
    (vd_gemm_dual_bias_act): a1 [M,K1], a2 [M,K2], w [N,K1+K2], bias [N].
    Returns None for a shape the kernel does not serve (the caller falls back)."""
    a1_, a2_ = _need(a1, "a1"), _need(a2, "a2")
    w_, b_ = _need(w, "w"), _need(bias, "bias")
    M, K1 = a1_.shape
    K2 = a2_.shape[1]
    N = w_.shape[0]
    if a2_.shape[0] != M or w_.shape[1] != K1 + K2 or b_.numel() != N:
        raise ValueError("gemm_dual_bias_act: a1 %s, a2 %s, w %s, bias %s"
                         % (tuple(a1_.shape), tuple(a2_.shape), tuple(w_.shape), tuple(b_.shape)))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a1_.device)
    elif tuple(out.shape) != (M, N) or not out.is_contiguous():
        raise ValueError("out must be a contiguous %s tensor" % ((M, N),))
    st = lib().vd_gemm_dual_bias_act(a1_.data_ptr(), K1, a2_.data_ptr(), K2, M, w_.data_ptr(), N,
                                     b_.data_ptr(), int(relu), out.data_ptr(), _stream())
    if st == VD_ERR_SHAPE:
        return None
    check(st, "vd_gemm_dual_bias_act")
    return out


FPN_LATERAL_K = (256, 512, 1024)  # csrc/gemm_lateral.hip (N = 256)


def fpn_lateral_weight(w: torch.Tensor) -> Optional[torch.Tensor]:
    """The lateral 1x1 conv weight [256][K] (or [256][K][1][1]) -> the fragment order
    vd_fpn_lateral_topdown reads (vd_fpn_lateral_weight; once per model).  None for a
    shape the kernel does not serve (N != 256 or K not in FPN_LATERAL_K)."""
    w_ = _need(w, "w").reshape(w.shape[0], -1).contiguous()
    N, K = w_.shape
    if N != 256 or K not in FPN_LATERAL_K:
        return None
    wf = torch.empty((K // 32, 16, 2, 64, 4), dtype=torch.float32, device=w_.device)
    check(lib().vd_fpn_lateral_weight(w_.data_ptr(), N, K, wf.data_ptr(), _stream()),
          "vd_fpn_lateral_weight")
    return wf


def fpn_lateral_topdown(lateral: torch.Tensor, wf: torch.Tensor, bias: torch.Tensor,
                        top: Optional[torch.Tensor],
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FPN.py topdown_lateral_module.forward (:292-300) in one MFMA launch
    (vd_fpn_lateral_topdown): conv_lateral(lateral) + nearest-2x(top), the sum in the
    reference's order ((conv + bias) + top).  lateral: channels_last N x K x H x W fp32;
    top: channels_last N x 256 x H/2 x W/2 (None: the lateral conv alone); wf from
    fpn_lateral_weight.  Returns a channels_last N x 256 x H x W tensor (`out` when given)."""
    if not lateral.is_cuda or lateral.dtype != torch.float32 or lateral.dim() != 4 \
            or not lateral.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("lateral must be a channels_last fp32 device tensor")
    N, K, H, W = lateral.shape
    wf_ = _need(wf, "wf")
    b_ = _need(bias, "bias")
    if tuple(wf_.shape) != (K // 32, 16, 2, 64, 4) or b_.numel() != 256:
        raise ValueError("fpn_lateral_topdown: wf %s / bias %s for K = %d"
                         % (tuple(wf_.shape), tuple(b_.shape), K))
    t_ = None
    if top is not None:
        if tuple(top.shape) != (N, 256, H // 2, W // 2) or H % 2 or W % 2:
            raise ValueError("top must be %s, got %s" % ((N, 256, H // 2, W // 2),
                                                         tuple(top.shape)))
        if not top.is_cuda or top.dtype != torch.float32:
            raise ValueError("top must be a float32 device tensor")
        # (not _need: its .contiguous() would copy a channels_last tensor to NCHW)
        t_ = top if top.is_contiguous(memory_format=torch.channels_last) else \
            top.contiguous(memory_format=torch.channels_last)
    if out is None:
        out = torch.empty((N, 256, H, W), dtype=torch.float32, device=lateral.device,
                          memory_format=torch.channels_last)
    elif tuple(out.shape) != (N, 256, H, W) or out.dtype != torch.float32 or not out.is_cuda \
            or not out.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("out must be a channels_last fp32 %s device tensor" % ((N, 256, H, W),))
    check(lib().vd_fpn_lateral_topdown(lateral.data_ptr(), N * H * W, K, wf_.data_ptr(), 256,
                                       b_.data_ptr(), t_.data_ptr() if t_ is not None else None,
                                       H, W, out.data_ptr(), _stream()),
          "vd_fpn_lateral_topdown")
    return out


def pixel_lut(pixel_means=(102.9801, 115.9465, 122.7717)) -> np.ndarray:
    """float32(u - mean_c) for u in 0..255 exactly as numpy computes
    ``im.astype(float32); im -= PIXEL_MEANS`` (float64 subtraction, float32 store,
    lib/utils/blob.py:126-127)."""
    u = np.arange(256, dtype=np.float32).astype(np.float64)
    return np.stack([(u - m).astype(np.float32) for m in pixel_means]).reshape(-1)


def image_to_blob(frames: torch.Tensor, lut: torch.Tensor, Hp: int, Wp: int, nhwc: bool = False,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    fr = _need(frames, "frames", torch.uint8)
    F, H, W, three = fr.shape
    lt = _need(lut, "lut")
    if out is None:
        shape = (F, Hp, Wp, 3) if nhwc else (F, 3, Hp, Wp)
        out = torch.empty(shape, dtype=torch.float32, device=fr.device)
    check(lib().vd_image_to_blob(fr.data_ptr(), F, H, W, lt.data_ptr(), Hp, Wp, int(nhwc),
                                 out.data_ptr(), _stream()), "vd_image_to_blob")
    return out


def target_scale(im_h: int, im_w: int, target_size: float, max_size: float) -> float:
    """lib/utils/blob.py:153-160 get_target_scale (Python floats = doubles)."""
    smin, smax = min(im_h, im_w), max(im_h, im_w)
    s = float(target_size) / float(smin)
    if np.round(s * smax) > max_size:
        s = float(max_size) / float(smax)
    return s


def resized_hw(im_h: int, im_w: int, im_scale: float):
    """cv::resize's dsize for fx = fy = im_scale: saturate_cast<int> rounds half
    to even, as Python's round does."""
    return int(round(im_h * im_scale)), int(round(im_w * im_scale))


def image_resize_to_blob(frames: torch.Tensor, lut: torch.Tensor, im_scale: float, Hp: int,
                         Wp: int, nhwc: bool = False, out: Optional[torch.Tensor] = None):
    """prep_im_for_blob + im_list_to_blob at any scale (vd_image_resize_to_blob)."""
    fr = _need(frames, "frames", torch.uint8)
    F, H, W, three = fr.shape
    Hr, Wr = resized_hw(H, W, im_scale)
    if Hp < Hr or Wp < Wr:
        raise ValueError("blob %dx%d smaller than the resized frame %dx%d" % (Hp, Wp, Hr, Wr))
    lt = _need(lut, "lut")
    if out is None:
        shape = (F, Hp, Wp, 3) if nhwc else (F, 3, Hp, Wp)
        out = torch.empty(shape, dtype=torch.float32, device=fr.device)
    check(lib().vd_image_resize_to_blob(fr.data_ptr(), F, H, W, lt.data_ptr(), float(im_scale),
                                        Hr, Wr, Hp, Wp, int(nhwc), out.data_ptr(), _stream()),
          "vd_image_resize_to_blob")
    return out


def aspect_width(im_w: int, ar: float) -> int:
    """lib/utils/image.py:30: int(round(aspect_ratio * im_w)), Python's round of the
    float64 product (half to even)."""
    return int(round(float(ar) * im_w))


def image_aspect_resize_to_blob(frames: torch.Tensor, lut: torch.Tensor, ar: float,
                                im_scale: float, Hp: int, Wp: int, hflip: bool = False,
                                nhwc: bool = False, out: Optional[torch.Tensor] = None):
    """The blob of an aspect-ratio view in one launch (vd_image_aspect_resize_to_blob):
    aspect_ratio_rel's u8 width resize to War = aspect_width(W, ar), the horizontal
    flip of that image when hflip (pass the UNFLIPPED frames), then prep_im_for_blob +
    im_list_to_blob at im_scale.  The u8 image is never written."""
    fr = _need(frames, "frames", torch.uint8)
    F, H, W, three = fr.shape
    War = aspect_width(W, ar)
    if War < 1:
        raise ValueError("aspect ratio %r of width %d leaves no column" % (ar, W))
    Hr, Wr = resized_hw(H, War, im_scale)
    if Hp < Hr or Wp < Wr:
        raise ValueError("blob %dx%d smaller than the resized frame %dx%d" % (Hp, Wp, Hr, Wr))
    lt = _need(lut, "lut")
    if out is None:
        shape = (F, Hp, Wp, 3) if nhwc else (F, 3, Hp, Wp)
        out = torch.empty(shape, dtype=torch.float32, device=fr.device)
    check(lib().vd_image_aspect_resize_to_blob(
        fr.data_ptr(), F, H, W, War, int(bool(hflip)), lt.data_ptr(), float(im_scale), Hr, Wr,
        Hp, Wp, int(nhwc), out.data_ptr(), _stream()), "vd_image_aspect_resize_to_blob")
    return out


# ---- frames of different sizes in one blob (vd_image_resize_to_blob_ragged)
GEOM_DTYPE = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("Hr", "<i4"),
                       ("Wr", "<i4"), ("inv_scale", "<f8")])  # struct VdFrameGeom
assert GEOM_DTYPE.itemsize == ctypes.sizeof(_lib.VdFrameGeom) == 32
RAGGED_MAX_WIDTH = 8192  # vd_segm_rle_ragged's column table (kSegmMaxW)


class FrameGeometry:
    """Per-frame geometry of one ragged step, as lists over frames: sizes (H, W),
    scale (get_target_scale), resized (Hr, Wr), padded (Hp, Wp), offset (bytes into
    the packed buffer) and nbytes (the packed frames' total)."""

    def __init__(self, sizes, scale, resized, padded, offset, nbytes):
        self.sizes, self.scale, self.resized, self.padded = sizes, scale, resized, padded
        self.offset, self.nbytes = offset, nbytes

    def __len__(self):
        return len(self.sizes)

    def fill_rows(self, rows: np.ndarray) -> np.ndarray:
        """The VdFrameGeom rows into a GEOM_DTYPE array (inv_scale = 1 / s in double)."""
        for f, ((H, W), s, (Hr, Wr)) in enumerate(zip(self.sizes, self.scale, self.resized)):
            rows[f] = (self.offset[f], H, W, Hr, Wr, 1.0 / s)
        return rows

    def rows(self) -> np.ndarray:
        return self.fill_rows(np.zeros(len(self), GEOM_DTYPE))

    def im_info(self) -> np.ndarray:
        """[F, 3] float32 (Hp_f, Wp_f, s_f): each frame's own get_image_blob row."""
        return np.array([[hp, wp, s] for (hp, wp), s in zip(self.padded, self.scale)],
                        np.float32).reshape(-1, 3)


def frame_geometry(sizes, target_size: float, max_size: float, stride: int) -> FrameGeometry:
    """get_image_blob's geometry of every (H, W) in `sizes`, in Python doubles exactly
    as target_scale and resized_hw compute it, with the frames packed back to back."""
    st = int(stride)
    sz, scale, resized, padded, offset = [], [], [], [], []
    pos = 0
    for H, W in sizes:
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError("frame size must be positive, got %dx%d" % (H, W))
        s = target_scale(H, W, target_size, max_size)
        Hr, Wr = resized_hw(H, W, s)
        sz.append((H, W))
        scale.append(s)
        resized.append((Hr, Wr))
        padded.append((-(-Hr // st) * st, -(-Wr // st) * st))
        offset.append(pos)
        pos += H * W * 3
    return FrameGeometry(sz, scale, resized, padded, offset, pos)


def blob_bound(sizes, cfg):
    """The smallest blob (Hb, Wb) that holds every frame of `sizes` under cfg's
    TEST.SCALE / TEST.MAX_SIZE / FPN.COARSEST_STRIDE: the maximum of the frames' own
    padded sizes, as im_list_to_blob's get_max_shape takes it."""
    geo = frame_geometry(sizes, cfg.TEST.SCALE, cfg.TEST.MAX_SIZE, cfg.FPN.COARSEST_STRIDE)
    if not len(geo):
        raise ValueError("blob_bound needs at least one frame size")
    return max(hp for hp, _ in geo.padded), max(wp for _, wp in geo.padded)


def check_geometry(geo: FrameGeometry, Hp: int, Wp: int, capacity: Optional[int] = None):
    """Host-side validation of a ragged step (the sizes are known here, the kernel
    only clamps): every resized frame inside the Hp x Wp bound, no frame wider than
    the ragged RLE kernel takes, the packed frames inside `capacity` bytes."""
    if len(geo) < 1:
        raise ValueError("a ragged step needs at least one frame")
    for f, ((H, W), (Hr, Wr)) in enumerate(zip(geo.sizes, geo.resized)):
        if Hr > Hp or Wr > Wp:
            raise ValueError("frame %d (%dx%d, resized %dx%d) is larger than the blob bound "
                             "%dx%d" % (f, H, W, Hr, Wr, Hp, Wp))
        if Hr < 1 or Wr < 1:
            raise ValueError("frame %d (%dx%d) resizes to nothing (%dx%d)" % (f, H, W, Hr, Wr))
        if W > RAGGED_MAX_WIDTH:
            raise ValueError("frame %d is %d wide; the ragged path takes widths up to %d"
                             % (f, W, RAGGED_MAX_WIDTH))
    if capacity is not None and geo.nbytes > capacity:
        raise ValueError("the step's frames take %d bytes, the packed buffer holds %d"
                         % (geo.nbytes, capacity))


def image_resize_to_blob_ragged(packed: torch.Tensor, geom, lut: torch.Tensor, Hp: int, Wp: int,
                                nhwc: bool = False, out: Optional[torch.Tensor] = None):
    """get_image_blob of F frames of different sizes into one F x 3 x Hp x Wp (nhwc:
    F x Hp x Wp x 3) blob, each frame top-left and zero elsewhere
    (vd_image_resize_to_blob_ragged).  packed: 1-D uint8 device tensor, the frames
    back to back.  geom: a FrameGeometry (validated here against the bound and
    packed's size, its rows uploaded), or a device uint8 tensor of F VdFrameGeom
    rows whose owner validated them (engine.RaggedBatch.load) -- then nothing here
    reads or writes host memory, so the call can be captured."""
    pk = _need(packed, "packed", torch.uint8)
    lt = _need(lut, "lut")
    Hp, Wp = int(Hp), int(Wp)
    if Hp < 1 or Wp < 1:
        raise ValueError("blob bound must be positive, got %dx%d" % (Hp, Wp))
    if isinstance(geom, FrameGeometry):
        check_geometry(geom, Hp, Wp, pk.numel())
        rows = torch.from_numpy(geom.rows().view(np.uint8)).to(pk.device)
    else:
        rows = _need(geom, "geom", torch.uint8)
        if rows.numel() < GEOM_DTYPE.itemsize or rows.numel() % GEOM_DTYPE.itemsize:
            raise ValueError("geom must hold whole VdFrameGeom rows (%d bytes each), got %d "
                             "bytes" % (GEOM_DTYPE.itemsize, rows.numel()))
    F = rows.numel() // GEOM_DTYPE.itemsize
    shape = (F, Hp, Wp, 3) if nhwc else (F, 3, Hp, Wp)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pk.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda \
            or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 device tensor of shape %s" % (shape,))
    check(lib().vd_image_resize_to_blob_ragged(pk.data_ptr(), rows.data_ptr(), F, lt.data_ptr(),
                                               Hp, Wp, int(nhwc), out.data_ptr(), _stream()),
          "vd_image_resize_to_blob_ragged")
    return out


# --------------------------------------------------------------------------- #
# Proposals, collect/distribute, detections                                    #
# --------------------------------------------------------------------------- #
def generate_proposals(cls_probs: Sequence[torch.Tensor], bbox_preds: Sequence[torch.Tensor],
                       anchors: Sequence[torch.Tensor], spatial_scales: Sequence[float],
                       im_info: torch.Tensor, pre_nms_topN: int, post_nms_topN: int,
                       nms_thresh: float, min_size: float, out=None):
    """GenerateProposalsOp over all levels / images.  Returns (rois [N,L,post,5],
    probs [N,L,post], counts int32 [N,L])."""
    L = len(cls_probs)
    descs = (_lib.VdRpnLevel * L)()
    keep = []
    N = cls_probs[0].shape[0]
    for i in range(L):
        p = _need(cls_probs[i], "cls_prob")
        d = _need(bbox_preds[i], "bbox_pred")
        a = _need(anchors[i], "anchors", torch.float64)
        keep += [p, d, a]
        _, A, H, W = p.shape
        descs[i] = _lib.VdRpnLevel(p.data_ptr(), d.data_ptr(), a.data_ptr(), A, H, W,
                                   float(spatial_scales[i]))
    info = _need(im_info, "im_info")
    dev = info.device
    if out is None:
        rois = torch.zeros((N, L, post_nms_topN, 5), dtype=torch.float32, device=dev)
        probs = torch.zeros((N, L, post_nms_topN), dtype=torch.float32, device=dev)
        counts = torch.zeros((N, L), dtype=torch.int32, device=dev)
    else:
        rois, probs, counts = out
    wsb = lib().vd_generate_proposals_workspace_size(descs, L, N, pre_nms_topN)
    ws = _ws(wsb, dev)
    check(lib().vd_generate_proposals(descs, L, N, info.data_ptr(), int(pre_nms_topN),
                                      int(post_nms_topN), float(np.float32(nms_thresh)),
                                      float(min_size), rois.data_ptr(), probs.data_ptr(),
                                      counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "vd_generate_proposals")
    return rois, probs, counts


COUNT_SELECT_FAILED, COUNT_PREV_BOXES = -1, -2  # include/vosdet.h VD_COUNT_*


def raise_on_failed_counts(counts, what: str = "frame"):
    """-1 in a per-image count means a device kernel could not complete that
    image (generate_proposals' top-k threshold search could not bracket
    pre_nms_topN within its candidate capacity; collect_distribute and
    box_detections pass the -1 on).  Raise instead of dropping proposals."""
    prev = [i for i, c in enumerate(counts) if c == COUNT_PREV_BOXES]
    if prev:
        raise _lib.VosdetError(
            "TEST.NMS_SMALL_BOX_IOU: the previous result of %s(s) %s holds more than one box "
            "of a class (lib_vos/tools/vos_test.py:848 asserts < 2; set "
            "TEST.NUM_DET_PER_CLASS_POST = 1 or TEST.NMS_WITH_MASK_IOU)" % (what, prev))
    bad = [i for i, c in enumerate(counts) if c < 0]
    if bad:
        raise _lib.VosdetError(
            "proposal selection failed for %s(s) %s: the pre_nms_topN threshold search "
            "could not bracket its candidates (count -1)" % (what, bad))


def collect_distribute(level_rois, level_probs, level_counts, post_nms_topN: int, k_min: int = 2,
                       k_max: int = 5, out=None):
    """collect + distribute per image: returns (rois [N,post,5], lvl idx int32
    [N,post] (level - k_min), counts int32 [N])."""
    lr = _need(level_rois, "level_rois")
    lp = _need(level_probs, "level_probs")
    lc = _need(level_counts, "level_counts", torch.int32)
    N, L, cap, _ = lr.shape
    if out is None:
        rois = torch.zeros((N, post_nms_topN, 5), dtype=torch.float32, device=lr.device)
        lvl = torch.zeros((N, post_nms_topN), dtype=torch.int32, device=lr.device)
        cnt = torch.zeros((N,), dtype=torch.int32, device=lr.device)
    else:
        rois, lvl, cnt = out
    check(lib().vd_collect_distribute(lr.data_ptr(), lp.data_ptr(), lc.data_ptr(), L, cap, N,
                                      int(post_nms_topN), k_min, k_max, rois.data_ptr(),
                                      lvl.data_ptr(), cnt.data_ptr(), _stream()),
          "vd_collect_distribute")
    return rois, lvl, cnt


GIVEN_BOXES_CAP = 4096  # csrc/vosdet_internal.hpp kGivenBoxesCap


def rois_from_boxes_workspace(F: int, cap: int) -> int:
    """Bytes of workspace vd_rois_from_boxes takes (0: its keys live in LDS)."""
    return int(lib().vd_rois_from_boxes_workspace(int(F), int(cap)))


def rois_from_boxes(boxes: torch.Tensor, counts: torch.Tensor, im_scale: torch.Tensor,
                    dedup: float = 0.0625, out=None):
    """The front of im_detect_bbox for caller-given boxes (lib/core/test.py:128-139 with
    MODEL.FASTER_RCNN False): _get_rois_blob and the DEDUP_BOXES hash + np.unique, for
    every frame of a step in one call (vd_rois_from_boxes).  boxes [F,cap,4] fp32 in image
    coordinates, counts [F] int32, im_scale [F] float64, all on the device; dedup is
    cfg.DEDUP_BOXES (0: no de-dup).  Nothing is read on the host, so the call can be
    captured.  -> (rois [F,cap,5], ucounts [F] int32, index [F,cap] int32, inv_index
    [F,cap] int32): rois[f, :ucounts[f]] are frame f's distinct RoIs in ascending hash
    order (column 0 = f), index their first rows, inv_index[f, :counts[f]] each row's RoI.
    Rows past the counts keep what `out` held (zeros when allocated here).  A count above
    cap leaves ucounts[f] = -1 (raise_on_failed_counts)."""
    b = _need(boxes, "boxes")
    n = _need(counts, "counts", torch.int32)
    sc = _need(im_scale, "im_scale", torch.float64)
    if b.dim() != 3 or b.shape[2] != 4:
        raise ValueError("boxes must be F x cap x 4, got %s" % (tuple(b.shape),))
    F, cap = b.shape[0], b.shape[1]
    if n.numel() != F or sc.numel() != F:
        raise ValueError("rois_from_boxes: boxes %s counts %s im_scale %s"
                         % (tuple(b.shape), tuple(n.shape), tuple(sc.shape)))
    if not 1 <= cap <= GIVEN_BOXES_CAP:
        raise ValueError("rois_from_boxes: cap = %d is outside 1..%d rows per frame"
                         % (cap, GIVEN_BOXES_CAP))
    if not float(dedup) >= 0:
        raise ValueError("rois_from_boxes: DEDUP_BOXES = %r is negative" % (dedup,))
    if out is None:
        rois = torch.zeros((F, cap, 5), dtype=torch.float32, device=b.device)
        ucounts = torch.zeros((F,), dtype=torch.int32, device=b.device)
        index = torch.zeros((F, cap), dtype=torch.int32, device=b.device)
        inv_index = torch.zeros((F, cap), dtype=torch.int32, device=b.device)
    else:
        rois, ucounts, index, inv_index = out
    if F:  # no workspace: rois_from_boxes_workspace is 0, the C entry takes NULL
        check(lib().vd_rois_from_boxes(b.data_ptr(), n.data_ptr(), sc.data_ptr(),
                                       float(np.float32(dedup)), F, cap, rois.data_ptr(),
                                       ucounts.data_ptr(), index.data_ptr(),
                                       inv_index.data_ptr(), None, 0, _stream()),
              "vd_rois_from_boxes")
    return rois, ucounts, index, inv_index


def get_rois_blob(im_rois, im_scale, frame: int = 0) -> np.ndarray:
    """_get_rois_blob (lib/core/test.py:877-890), an ndarray drop-in: R x 4 boxes in image
    coordinates -> R x 5 float32 (frame, box * im_scale), through vd_rois_from_boxes
    without the de-dup."""
    b = np.ascontiguousarray(im_rois, dtype=np.float32).reshape(-1, 4)
    R = b.shape[0]
    if R == 0:
        return np.zeros((0, 5), np.float32)
    if R > GIVEN_BOXES_CAP:
        raise ValueError("get_rois_blob: %d boxes exceed %d per call" % (R, GIVEN_BOXES_CAP))
    dev = torch.device("cuda")
    F = int(frame) + 1  # the kernel writes its frame number into column 0
    boxes = torch.zeros((F, R, 4), dtype=torch.float32, device=dev)
    boxes[frame] = torch.from_numpy(b).to(dev)
    counts = torch.zeros((F,), dtype=torch.int32, device=dev)
    counts[frame] = R
    scale = torch.full((F,), float(np.asarray(im_scale, np.float64).reshape(-1)[0]),
                       dtype=torch.float64, device=dev)
    rois, _, _, _ = rois_from_boxes(boxes, counts, scale, 0.)
    return rois[frame].cpu().numpy()


def gather_rows(boxes: torch.Tensor, scores: torch.Tensor, deltas: torch.Tensor,
                index: torch.Tensor, inv_index: torch.Tensor, counts: torch.Tensor,
                ucounts: torch.Tensor, out=None):
    """scores[inv_index], pred_boxes[inv_index] of im_detect_bbox (lib/core/test.py:186-189)
    in front of the decode (vd_gather_rows): scores [F,cap,K] and deltas [F,cap,D] of the
    distinct RoIs and the caller's boxes [F,cap,4] -> for the caller's rows r < counts[f]
    the scores and deltas of row inv_index[f, r] and the box rows (f, boxes[f,
    index[f, inv_index[f, r]]]) [F,cap,5] the reference decodes from (boxes[index],
    test.py:139): box_detections takes them as its rois with an im_scale of 1.  The fourth
    result is its roi_count: counts, or the failure code of ucounts.  Rows past counts
    keep what `out` held (zeros here)."""
    b, s, d = _need(boxes, "boxes"), _need(scores, "scores"), _need(deltas, "deltas")
    i, v = _need(index, "index", torch.int32), _need(inv_index, "inv_index", torch.int32)
    n, u = _need(counts, "counts", torch.int32), _need(ucounts, "ucounts", torch.int32)
    if b.dim() != 3 or b.shape[2] != 4:
        raise ValueError("boxes must be F x cap x 4, got %s" % (tuple(b.shape),))
    F, cap = b.shape[0], b.shape[1]
    if s.dim() != 3 or d.dim() != 3 or tuple(s.shape[:2]) != (F, cap) or \
            tuple(d.shape[:2]) != (F, cap) or tuple(i.shape) != (F, cap) or \
            tuple(v.shape) != (F, cap) or n.numel() != F or u.numel() != F:
        raise ValueError("gather_rows: boxes %s scores %s deltas %s index %s inv_index %s "
                         "counts %s ucounts %s"
                         % (tuple(b.shape), tuple(s.shape), tuple(d.shape), tuple(i.shape),
                            tuple(v.shape), tuple(n.shape), tuple(u.shape)))
    if out is None:
        ro = torch.zeros((F, cap, 5), dtype=torch.float32, device=b.device)
        so, do = torch.zeros_like(s), torch.zeros_like(d)
        co = torch.zeros((F,), dtype=torch.int32, device=b.device)
    else:
        ro, so, do, co = out
    if F:
        check(lib().vd_gather_rows(b.data_ptr(), s.data_ptr(), d.data_ptr(), i.data_ptr(),
                                   v.data_ptr(), n.data_ptr(), u.data_ptr(), F, cap, s.shape[2],
                                   d.shape[2], ro.data_ptr(), so.data_ptr(), do.data_ptr(),
                                   co.data_ptr(), _stream()), "vd_gather_rows")
    return ro, so, do, co


SOFT_NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}  # utils/boxes.py:344
BBOX_VOTE_METHODS = {"ID": 0, "AVG": 1, "IOU_AVG": 2, "QUASI_SUM": 3}


def bbox_vote_method(scoring_method: str, beta: float = 1.0) -> int:
    """TEST.BBOX_VOTE.SCORING_METHOD -> vd_box_detections_ex's code; GENERALIZED_AVG
    at beta 1 is AVG (mean(ws**1)**1).  TEMP_AVG (numpy's float32 log / exp) and
    GENERALIZED_AVG at other betas raise NotImplementedError."""
    if scoring_method == "GENERALIZED_AVG" and float(beta) == 1.0:
        return BBOX_VOTE_METHODS["AVG"]
    if scoring_method not in BBOX_VOTE_METHODS:
        raise NotImplementedError("TEST.BBOX_VOTE.SCORING_METHOD=%r (beta %r) is not implemented"
                                  % (scoring_method, beta))
    return BBOX_VOTE_METHODS[scoring_method]


def box_detections(rois, cls_prob, bbox_pred, roi_count, im_scale, im_hw, score_thresh=0.05,
                   nms_thresh=0.5, dets_per_im=100, bbox_reg_weights=(10., 10., 5., 5.),
                   det_cap=256, out=None, nms_cross_class=0., num_det_per_class_pre=0,
                   soft_nms=None, soft_nms_sigma=0.5, bbox_vote=None, bbox_vote_thresh=0.8,
                   bbox_vote_beta=1.0):
    """Decode + clip + per-class NMS + detections limit.  rois [N,R,5],
    cls_prob [N,R,K], bbox_pred [N,R,4K] -> (dets [N,cap,5], cls int32 [N,cap],
    counts int32 [N]).  soft_nms: TEST.SOFT_NMS.METHOD ('hard' / 'linear' /
    'gaussian') instead of the NMS; bbox_vote: TEST.BBOX_VOTE.SCORING_METHOD
    (lib/core/test.py:756-776, vd_box_detections_ex)."""
    r = _need(rois, "rois")
    p = _need(cls_prob, "cls_prob")
    d = _need(bbox_pred, "bbox_pred")
    c = _need(roi_count, "roi_count", torch.int32)
    s = _need(im_scale, "im_scale")
    hw = _need(im_hw, "im_hw", torch.int32)
    N, R, K = p.shape
    if out is None:
        dets = torch.zeros((N, det_cap, 5), dtype=torch.float32, device=r.device)
        cls = torch.zeros((N, det_cap), dtype=torch.int32, device=r.device)
        cnt = torch.zeros((N,), dtype=torch.int32, device=r.device)
    else:
        dets, cls, cnt = out
    wsb = lib().vd_box_detections_workspace_size(R, N, K)
    ws = _ws(wsb, r.device)
    w = (ctypes.c_float * 4)(*[float(np.float32(x)) for x in bbox_reg_weights])
    if soft_nms is None and bbox_vote is None:
        check(lib().vd_box_detections(r.data_ptr(), p.data_ptr(), d.data_ptr(), c.data_ptr(), R,
                                      N, K, s.data_ptr(), hw.data_ptr(),
                                      float(np.float32(score_thresh)),
                                      float(np.float32(nms_thresh)), int(dets_per_im),
                                      ctypes.cast(w, ctypes.c_void_p), det_cap, dets.data_ptr(),
                                      cls.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream()), "vd_box_detections")
    else:
        sm = -1 if soft_nms is None else SOFT_NMS_METHODS[soft_nms]
        vm = -1 if bbox_vote is None else bbox_vote_method(bbox_vote, bbox_vote_beta)
        check(lib().vd_box_detections_ex(
            r.data_ptr(), p.data_ptr(), d.data_ptr(), c.data_ptr(), R, N, K, s.data_ptr(),
            hw.data_ptr(), float(np.float32(score_thresh)), float(np.float32(nms_thresh)),
            int(dets_per_im), ctypes.cast(w, ctypes.c_void_p), sm,
            float(np.float32(soft_nms_sigma)), float(np.float32(0.0001)), vm,
            float(np.float32(bbox_vote_thresh)), float(bbox_vote_beta), det_cap, dets.data_ptr(),
            cls.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "vd_box_detections_ex")
    if nms_cross_class > 0 or num_det_per_class_pre > 0:  # the fork's vos_test.py:805-833
        check(lib().vd_detections_postfilter(dets.data_ptr(), cls.data_ptr(), cnt.data_ptr(), N,
                                             det_cap, float(np.float32(nms_cross_class)),
                                             int(num_det_per_class_pre), _stream()),
              "vd_detections_postfilter")
    return dets, cls, cnt


UNION_MAX_CAND = 16384  # csrc/box_union.hip kUnionCandMax


class BoxUnion:
    """im_detect_bbox_aug with the UNION heuristics followed by
    box_results_with_nms_and_limit (lib/core/test.py:193-311, 733-797) on the device:
    add_view() once per box view in np.vstack order (config.aug_views' box order, the
    identity view last), then detections().  The per-class candidate lists live in one
    workspace of vd_box_union_workspace_size(cand_cap, F, K) bytes, allocated here once
    (no allocation per step)."""

    def __init__(self, cand_cap: int, num_images: int, num_classes: int, device="cuda"):
        if not 1 <= int(cand_cap) <= UNION_MAX_CAND:
            raise ValueError("BoxUnion: cand_cap = %r outside [1, %d]" % (cand_cap, UNION_MAX_CAND))
        self.cand_cap, self.F, self.K = int(cand_cap), int(num_images), int(num_classes)
        self.ws = _ws(lib().vd_box_union_workspace_size(self.cand_cap, self.F, self.K), device)
        self.views = 0

    def add_view(self, rois, cls_prob, bbox_pred, roi_count, im_scale, im_hw, hflip: bool,
                 score_thresh=0.05, bbox_reg_weights=(10., 10., 5., 5.), first=None,
                 x_inv=None):
        """One view's rois [F,R,5], cls_prob [F,R,K], bbox_pred [F,R,4K], roi_count [F],
        its im_scale [F] fp32 and the ORIGINAL frames' im_hw [F,2] int32.  first (default:
        the first call after construction or detections()) empties the lists.  x_inv: an
        aspect-ratio view's float32(1.0 / ar) (vd_box_union_add_view_ar: im_hw is then
        the view's (H, War), and x1, x2 are multiplied by x_inv after the flip-back)."""
        r = _need(rois, "rois")
        p = _need(cls_prob, "cls_prob")
        d = _need(bbox_pred, "bbox_pred")
        c = _need(roi_count, "roi_count", torch.int32)
        s = _need(im_scale, "im_scale")
        hw = _need(im_hw, "im_hw", torch.int32)
        N, R, K = p.shape
        if (N, K) != (self.F, self.K) or tuple(d.shape) != (N, R, 4 * K) or \
                tuple(r.shape) != (N, R, 5) or c.numel() != N or s.numel() != N or \
                hw.numel() != 2 * N:
            raise ValueError("BoxUnion.add_view: rois %s cls_prob %s bbox_pred %s for F = %d, "
                             "K = %d" % (tuple(r.shape), tuple(p.shape), tuple(d.shape), self.F,
                                         self.K))
        first = self.views == 0 if first is None else bool(first)
        w = (ctypes.c_float * 4)(*[float(np.float32(x)) for x in bbox_reg_weights])
        if x_inv is None:
            check(lib().vd_box_union_add_view(
                r.data_ptr(), p.data_ptr(), d.data_ptr(), c.data_ptr(), R, N, K, s.data_ptr(),
                hw.data_ptr(), int(bool(hflip)), int(first), float(np.float32(score_thresh)),
                ctypes.cast(w, ctypes.c_void_p), self.cand_cap, self.ws.data_ptr(),
                self.ws.numel(), _stream()), "vd_box_union_add_view")
        else:
            check(lib().vd_box_union_add_view_ar(
                r.data_ptr(), p.data_ptr(), d.data_ptr(), c.data_ptr(), R, N, K, s.data_ptr(),
                hw.data_ptr(), int(bool(hflip)), float(np.float32(x_inv)), int(first),
                float(np.float32(score_thresh)), ctypes.cast(w, ctypes.c_void_p), self.cand_cap,
                self.ws.data_ptr(), self.ws.numel(), _stream()), "vd_box_union_add_view_ar")
        self.views = 1 if first else self.views + 1

    def detections(self, nms_thresh=0.5, dets_per_im=100, det_cap=256, out=None,
                   nms_cross_class=0., num_det_per_class_pre=0, soft_nms=None,
                   soft_nms_sigma=0.5, bbox_vote=None, bbox_vote_thresh=0.8, bbox_vote_beta=1.0,
                   cand_counts=None):
        """-> (dets [F,cap,5], cls int32 [F,cap], counts int32 [F]) as box_detections
        returns them; a failed image (a list past cand_cap, a failed view) has count -1.
        cand_counts: optional int32 [F,K] tensor that receives the lists' lengths."""
        dev = self.ws.device
        if out is None:
            dets = torch.zeros((self.F, det_cap, 5), dtype=torch.float32, device=dev)
            cls = torch.zeros((self.F, det_cap), dtype=torch.int32, device=dev)
            cnt = torch.zeros((self.F,), dtype=torch.int32, device=dev)
        else:
            dets, cls, cnt = out
        sm = -1 if soft_nms is None else SOFT_NMS_METHODS[soft_nms]
        vm = -1 if bbox_vote is None else bbox_vote_method(bbox_vote, bbox_vote_beta)
        cc = None
        if cand_counts is not None:
            cc = _need(cand_counts, "cand_counts", torch.int32)
            if cc.numel() != self.F * self.K or cc.data_ptr() != cand_counts.data_ptr():
                raise ValueError("cand_counts must be a contiguous int32 [F, K] tensor")
        check(lib().vd_box_union_detections(
            self.cand_cap, self.F, self.K, float(np.float32(nms_thresh)), int(dets_per_im), sm,
            float(np.float32(soft_nms_sigma)), float(np.float32(0.0001)), vm,
            float(np.float32(bbox_vote_thresh)), float(bbox_vote_beta), det_cap, dets.data_ptr(),
            cls.data_ptr(), cnt.data_ptr(), None if cc is None else cc.data_ptr(),
            self.ws.data_ptr(), self.ws.numel(), _stream()), "vd_box_union_detections")
        if nms_cross_class > 0 or num_det_per_class_pre > 0:  # the fork's vos_test.py:805-833
            check(lib().vd_detections_postfilter(dets.data_ptr(), cls.data_ptr(), cnt.data_ptr(),
                                                 self.F, det_cap,
                                                 float(np.float32(nms_cross_class)),
                                                 int(num_det_per_class_pre), _stream()),
                  "vd_detections_postfilter")
        self.views = 0
        return dets, cls, cnt


MASK_AUG_HEURS = {"SOFT_AVG": 0, "SOFT_MAX": 1, "LOGIT_AVG": 2}  # include/vosdet.h VD_MASK_AUG_*


def mask_aug_accumulate(acc: torch.Tensor, masks: torch.Tensor, hflip: bool, heur: str,
                        first: bool) -> torch.Tensor:
    """One view of im_detect_mask_aug's masks_ts (lib/core/test.py:405-476) folded into
    acc in place (vd_mask_aug_accumulate): masks [M,R,R] class-selected sigmoid outputs,
    a flipped view read with its last axis reversed; first: the identity view."""
    a, m = _need(acc, "acc"), _need(masks, "masks")
    if a.data_ptr() != acc.data_ptr() or a.shape != m.shape or m.dim() != 3 or \
            m.shape[1] != m.shape[2]:
        raise ValueError("mask_aug_accumulate: acc %s (contiguous) and masks %s must both be "
                         "[M, R, R]" % (tuple(acc.shape), tuple(masks.shape)))
    M, R = m.shape[0], m.shape[2]
    check(lib().vd_mask_aug_accumulate(a.data_ptr() if M else None, m.data_ptr() if M else None,
                                       M, R, int(bool(hflip)), MASK_AUG_HEURS[heur],
                                       int(bool(first)), _stream()), "vd_mask_aug_accumulate")
    return acc


def mask_aug_finish(acc: torch.Tensor, num_views: int, heur: str) -> torch.Tensor:
    """np.mean / the logistic of the mean logit over the num_views accumulated views, in
    place (vd_mask_aug_finish); SOFT_MAX needs nothing."""
    a = _need(acc, "acc")
    if a.data_ptr() != acc.data_ptr() or a.dim() != 3:
        raise ValueError("mask_aug_finish: acc must be a contiguous [M, R, R] tensor")
    M, R = a.shape[0], a.shape[2]
    check(lib().vd_mask_aug_finish(a.data_ptr() if M else None, M, R, int(num_views),
                                   MASK_AUG_HEURS[heur], _stream()), "vd_mask_aug_finish")
    return acc


def detections_prev_box_filter(dets: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor,
                               prev_dets: torch.Tensor, prev_classes: torch.Tensor,
                               prev_counts: torch.Tensor, iou_thresh: float,
                               score_thresh: float) -> None:
    """TEST.NMS_SMALL_BOX_IOU (lib_vos/tools/vos_test.py:845-860) in place on the
    device detections (vd_detections_prev_box_filter): dets [F,cap,5], classes /
    counts as box_detections writes them; prev_* the previous frame's final result
    of each row ([F,pcap,5], [F,pcap], [F]).  A row whose previous result holds
    two boxes of one class gets count -1 (the reference asserts)."""
    d, c, n = _need(dets, "dets"), _need(classes, "classes", torch.int32), \
        _need(counts, "counts", torch.int32)
    pd, pc, pn = _need(prev_dets, "prev_dets"), _need(prev_classes, "prev_classes", torch.int32), \
        _need(prev_counts, "prev_counts", torch.int32)
    F, cap = d.shape[0], d.shape[1]
    if tuple(pd.shape[:1]) != (F,) or pd.shape[2] != 5 or tuple(pc.shape) != tuple(pd.shape[:2]) \
            or pn.numel() != F:
        raise ValueError("prev_* must be [F,pcap,5], [F,pcap], [F] for F = %d" % F)
    check(lib().vd_detections_prev_box_filter(
        d.data_ptr(), c.data_ptr(), n.data_ptr(), F, cap, pd.data_ptr(), pc.data_ptr(),
        pn.data_ptr(), pd.shape[1], float(np.float32(iou_thresh)),
        float(np.float32(score_thresh)), _stream()), "vd_detections_prev_box_filter")


def mask_iou_nms(planes: torch.Tensor, dets: torch.Tensor, classes: torch.Tensor,
                 iou_th: float, max_per_class: int) -> torch.Tensor:
    """nms_with_mask_iou (lib_vos/tools/vos_test.py:985-1029) on one frame
    (vd_mask_iou_nms): planes [n,H,W] uint8 binary masks, dets [n,>=5], classes
    [n] int32, in cls_boxes order.  Returns the kept indices (int64) in the
    reference's output order (class ascending, then score order)."""
    pl = _need(planes, "planes", torch.uint8)
    d, c = _need(dets, "dets"), _need(classes, "classes", torch.int32)
    n = d.shape[0]
    if pl.shape[0] != n or c.numel() != n:
        raise ValueError("planes, dets and classes must have the same n")
    H, W = (pl.shape[1], pl.shape[2]) if pl.dim() == 3 else (1, 1)
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=d.device)
    num = torch.zeros((1,), dtype=torch.int32, device=d.device)
    ws = _ws(lib().vd_mask_iou_nms_workspace_size(n, H, W), d.device)
    check(lib().vd_mask_iou_nms(pl.data_ptr() if n else None, n, H, W,
                                d.data_ptr() if n else None, d.shape[1] if d.dim() == 2 else 5,
                                c.data_ptr() if n else None, float(iou_th), int(max_per_class),
                                keep.data_ptr(), num.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream()), "vd_mask_iou_nms")
    return keep[: int(num.item())]


def mask_iou_nms_frames_workspace(F: int, cap: int, rows: int, im_h: int, im_w: int) -> int:
    """Bytes of workspace vd_mask_iou_nms_frames takes for this shape (0: refused)."""
    return int(lib().vd_mask_iou_nms_frames_workspace_size(int(F), int(cap), int(rows),
                                                           int(im_h), int(im_w)))


def mask_iou_nms_frames(masks: torch.Tensor, dets: torch.Tensor, classes: torch.Tensor,
                        counts: torch.Tensor, im_h: int, im_w: int, iou_th: float,
                        max_per_class: int, bin_thresh: float = 0.5, prev=None,
                        want_valid: bool = True, rows_fit: bool = False,
                        workspace_budget: int = 1 << 30):
    """nms_with_mask_iou (lib_vos/tools/vos_test.py:985-1029) of every frame of a step
    in one call (vd_mask_iou_nms_frames), from the R x R mask probabilities: masks
    [M,R,R] fp32 class-selected, rows in (frame, detection) order; dets [F,cap,5],
    classes [F,cap] int32, counts [F] int32 on the device, as label_maps takes them.
    Nothing is read on the host and no allocation depends on a device value, so counts
    still being computed on the stream are a valid input and the call can be captured.
    -> (keep [F,cap] int32, keep_counts [F] int32, valid [F,cap] uint8 or None):
    keep[f, :keep_counts[f]] are frame f's kept rows in the reference's output order
    (class ascending, then score order), exactly what paste_masks + mask_iou_nms give
    on that frame; valid marks them.  A negative count stays in keep_counts.
    prev = (prev_dets [F,pcap,5], prev_classes [F,pcap] int32, prev_counts [F] int32),
    pcap >= cap, contiguous: receives the kept rows and their number in place (the
    previous-frame result detections_prev_box_filter reads).  Detections whose mask row
    is past M are cut on the device; rows_fit (the caller knows they fit) changes
    nothing here and is accepted for symmetry with label_maps.  ValueError when the
    workspace exceeds workspace_budget bytes."""
    m = _need(masks, "masks")
    d, c, n = _need(dets, "dets"), _need(classes, "classes", torch.int32), \
        _need(counts, "counts", torch.int32)
    if d.dim() != 3 or d.shape[2] != 5:
        raise ValueError("dets must be F x cap x 5, got %s" % (tuple(d.shape),))
    F, cap = d.shape[0], d.shape[1]
    if tuple(c.shape) != (F, cap) or n.numel() != F:
        raise ValueError("mask_iou_nms_frames: dets %s classes %s counts %s"
                         % (tuple(d.shape), tuple(c.shape), tuple(n.shape)))
    if m.dim() != 3 or m.shape[1] != m.shape[2]:
        raise ValueError("masks must be M x R x R, got %s" % (tuple(m.shape),))
    M, R = m.shape[0], m.shape[2]
    pd = pc = pn = None
    pcap = 0
    if prev is not None:
        pd, pc, pn = prev
        for t, name, dt in ((pd, "prev_dets", torch.float32), (pc, "prev_classes", torch.int32),
                            (pn, "prev_counts", torch.int32)):
            if _need(t, name, dt) is not t:
                raise ValueError("%s must be contiguous: it is written in place" % name)
        pcap = pd.shape[1] if pd.dim() == 3 else 0
        if pd.dim() != 3 or pd.shape[0] != F or pd.shape[2] != 5 or pcap < cap or \
                tuple(pc.shape) != (F, pcap) or pn.numel() != F:
            raise ValueError("prev must be ([F,pcap,5], [F,pcap], [F]) with F = %d and "
                             "pcap >= cap = %d" % (F, cap))
    keep = torch.zeros((F, cap), dtype=torch.int32, device=d.device)
    keep_counts = torch.zeros((F,), dtype=torch.int32, device=d.device)
    valid = torch.zeros((F, cap), dtype=torch.uint8, device=d.device) if want_valid else None
    if F == 0:
        return keep, keep_counts, valid
    size = mask_iou_nms_frames_workspace(F, cap, M, im_h, im_w)
    if size > int(workspace_budget):
        raise ValueError("mask_iou_nms_frames: the workspace for F = %d, cap = %d, %d mask rows "
                         "at %d x %d is %d bytes, above workspace_budget = %d"
                         % (F, cap, M, im_h, im_w, size, int(workspace_budget)))
    ws = _ws(size, d.device)
    check(lib().vd_mask_iou_nms_frames(
        m.data_ptr() if M else d.data_ptr(), M, R, d.data_ptr(), c.data_ptr(), n.data_ptr(), F,
        cap, int(im_h), int(im_w), float(np.float32(bin_thresh)), float(iou_th),
        int(max_per_class), keep.data_ptr(), keep_counts.data_ptr(),
        valid.data_ptr() if valid is not None else None,
        pd.data_ptr() if pd is not None else None, pc.data_ptr() if pc is not None else None,
        pn.data_ptr() if pn is not None else None, pcap, ws.data_ptr(), ws.numel(), _stream()),
        "vd_mask_iou_nms_frames")
    return keep, keep_counts, valid


# --------------------------------------------------------------------------- #
# segm_results: paste + binarize + RLE counts      #
# --------------------------------------------------------------------------- #
def paste_masks(masks: torch.Tensor, boxes: torch.Tensor, im_h: int, im_w: int,
                thresh: float = 0.5, out=None) -> torch.Tensor:
    """masks [M,R,R] fp32 (class-selected probabilities), boxes [M,>=4] fp32 image
    coordinates -> [M,im_h,im_w] uint8 binary masks (segm_results' expand_boxes +
    cv2.resize + `> THRESH_BINARIZE` + paste, lib/core/test.py:801-835)."""
    m = _need(masks, "masks")
    b = _need(boxes, "boxes")
    M, R = m.shape[0], m.shape[-1]
    if b.shape[0] != M or b.dim() != 2 or b.shape[1] < 4:
        raise ValueError("boxes must be M x >=4, got %s" % (tuple(b.shape),))
    if out is None:
        out = torch.empty((M, im_h, im_w), dtype=torch.uint8, device=m.device)
    check(lib().vd_paste_masks(m.data_ptr(), M, R, b.data_ptr(), b.shape[1], int(im_h),
                               int(im_w), float(np.float32(thresh)), out.data_ptr(), _stream()),
          "vd_paste_masks")
    return out


def mask_rle_counts(planes: torch.Tensor, cap: Optional[int] = None):
    """pycocotools mask.encode run lengths (column-major, zeros first) of each
    [H,W] uint8 plane: returns (counts int32 [M,cap'], n int32 [M]); runs are
    < H*W <= 2^31, so int32 holds the kernel's uint32 counts."""
    p = _need(planes, "planes", torch.uint8)
    M, H, W = p.shape
    cap = int(cap or (8 * W + 2))
    while True:
        counts = torch.empty((M, cap), dtype=torch.int32, device=p.device)
        n = torch.empty((M,), dtype=torch.int32, device=p.device)
        check(lib().vd_mask_rle(p.data_ptr(), M, H, W, counts.data_ptr(), cap, n.data_ptr(),
                                _stream()), "vd_mask_rle")
        need = int((-n).max().item()) if M else 0
        if need <= cap:
            return counts, n
        cap = need


def bias_relu_maxpool(x_raw: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """ResNet stem tail (vd_bias_relu_maxpool): MaxPool2d(3, 2, 1)(relu(x + b)) of
    a channels_last N x C x H x W tensor; returns channels_last N x C x Ho x Wo."""
    N, C, H, W = x_raw.shape
    if not (x_raw.is_cuda and x_raw.dtype == torch.float32
            and x_raw.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("x_raw must be a channels_last float32 device tensor")
    b = _need(bias, "bias")
    if b.numel() != C:
        raise ValueError("bias must have C = %d entries" % C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((N, C, Ho, Wo), dtype=torch.float32, device=x_raw.device,
                      memory_format=torch.channels_last)
    check(lib().vd_bias_relu_maxpool(x_raw.data_ptr(), b.data_ptr(), N, C, H, W,
                                     out.data_ptr(), _stream()), "vd_bias_relu_maxpool")
    return out


def stem_pack(weight: torch.Tensor, split: bool = False) -> torch.Tensor:
    """conv1's weight [64, 3, 7, 7] in vd_stem_conv_pool's register order (once), or
    (split) its three-piece bf16 image for vd_stem_split_conv_pool (a uint8 tensor)."""
    w = _need(weight, "weight")
    if tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError("stem weight must be 64 x 3 x 7 x 7, got %s" % (tuple(w.shape),))
    if split:
        out = torch.empty((lib().vd_stem_split_weight_size(),), dtype=torch.uint8,
                          device=w.device)
        check(lib().vd_stem_split_weight_pack(w.data_ptr(), out.data_ptr(), _stream()),
              "vd_stem_split_weight_pack")
        return out
    out = torch.empty((lib().vd_stem_weight_size() // 4,), dtype=torch.float32, device=w.device)
    check(lib().vd_stem_weight_pack(w.data_ptr(), out.data_ptr(), _stream()),
          "vd_stem_weight_pack")
    return out


def stem_conv_pool(x: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """ResNet stem in one kernel (vd_stem_conv_pool, or vd_stem_split_conv_pool for a
    split image from stem_pack(w, split=True)): MaxPool2d(3, 2, 1)(relu(conv1 7x7/2
    pad 3 (x) + bias)) for a channels_last N x 3 x H x W blob; returns channels_last
    N x 64 x Ho x Wo (the conv output never leaves LDS)."""
    N, C, H, W = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and C == 3
            and x.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("x must be a channels_last float32 N x 3 x H x W device tensor")
    b = _need(bias, "bias")
    if b.numel() != 64:
        raise ValueError("bias must have 64 entries")
    split = packed.dtype == torch.uint8
    need = lib().vd_stem_split_weight_size() if split else lib().vd_stem_weight_size()
    if not packed.is_cuda or packed.numel() * packed.element_size() != need:
        raise ValueError("packed must be stem_pack's device image (%d bytes)" % need)
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Ho, Wo = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.empty((N, 64, Ho, Wo), dtype=torch.float32, device=x.device,
                      memory_format=torch.channels_last)
    fn = lib().vd_stem_split_conv_pool if split else lib().vd_stem_conv_pool
    check(fn(x.data_ptr(), N, H, W, packed.data_ptr(), b.data_ptr(), out.data_ptr(), _stream()),
          "vd_stem_split_conv_pool" if split else "vd_stem_conv_pool")
    return out


def rpn_head(x_raw: torch.Tensor, conv_bias: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
             num_anchors: int):
    """FPN RPN head of one level (vd_rpn_head): x_raw = the shared 3x3 conv's
    output without bias, N x C x H x W in channels_last memory; w [5A, C] (cls
    then bbox 1x1 weights), b [5A].  Returns (cls_prob N x A x H x W after the
    sigmoid, bbox_pred N x 4A x H x W), both contiguous NCHW."""
    N, C, H, W = x_raw.shape
    if not (x_raw.is_cuda and x_raw.dtype == torch.float32
            and x_raw.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("x_raw must be a channels_last float32 device tensor")
    A = int(num_anchors)
    cb = _need(conv_bias, "conv_bias")
    wt = _need(w, "w")
    bt = _need(b, "b")
    if tuple(wt.shape) != (5 * A, C) or bt.numel() != 5 * A or cb.numel() != C:
        raise ValueError("w must be [5A, C] = [%d, %d], b [5A], conv_bias [C]" % (5 * A, C))
    cls = torch.empty((N, A, H, W), dtype=torch.float32, device=x_raw.device)
    box = torch.empty((N, 4 * A, H, W), dtype=torch.float32, device=x_raw.device)
    check(lib().vd_rpn_head(x_raw.data_ptr(), cb.data_ptr(), wt.data_ptr(), bt.data_ptr(), N, H,
                            W, C, A, cls.data_ptr(), box.data_ptr(), _stream()), "vd_rpn_head")
    return cls, box


def segm_rle_counts(masks: torch.Tensor, boxes: torch.Tensor, im_h: int, im_w: int,
                    thresh: float = 0.5, cap: Optional[int] = None):
    """paste_masks + mask_rle_counts fused (vd_segm_rle): the same counts and n
    without materialising the M x im_h x im_w planes.  Frames wider than the
    fused kernel's LDS column table (VD_ERR_SHAPE) take the two-pass planes path
    (paste_masks, then mask_rle_counts), which has no width limit."""
    m = _need(masks, "masks")
    b = _need(boxes, "boxes")
    M, R = m.shape[0], m.shape[-1]
    if b.shape[0] != M or b.dim() != 2 or b.shape[1] < 4:
        raise ValueError("boxes must be M x >=4, got %s" % (tuple(b.shape),))
    cap = int(cap or (4 * im_w + 2))
    while True:
        counts = torch.empty((M, cap), dtype=torch.int32, device=m.device)
        n = torch.empty((M,), dtype=torch.int32, device=m.device)
        st = lib().vd_segm_rle(m.data_ptr(), M, R, b.data_ptr(), b.shape[1], int(im_h),
                               int(im_w), float(np.float32(thresh)), counts.data_ptr(), cap,
                               n.data_ptr(), _stream())
        if st == VD_ERR_SHAPE:
            return mask_rle_counts(paste_masks(m, b, im_h, im_w, thresh))
        check(st, "vd_segm_rle")
        need = int((-n).max().item()) if M else 0
        if need <= cap:
            return counts, n
        cap = need


def segm_rle_counts_ragged(masks: torch.Tensor, boxes: torch.Tensor, det_hw, thresh: float = 0.5,
                           cap: Optional[int] = None):
    """segm_rle_counts for detections of frames of different sizes in one launch
    (vd_segm_rle_ragged): det_hw [M, 2] = (im_h, im_w) of each detection's own
    frame, as a host array or a tensor (its values are read on the host: they are
    validated here, the kernel has no planes fallback for wide frames).  Returns
    the same (counts, n) as segm_rle_counts called per frame, rows in order."""
    m = _need(masks, "masks")
    b = _need(boxes, "boxes")
    M, R = m.shape[0], m.shape[-1]
    if b.shape[0] != M or b.dim() != 2 or b.shape[1] < 4:
        raise ValueError("boxes must be M x >=4, got %s" % (tuple(b.shape),))
    hw = det_hw.detach().cpu().numpy() if isinstance(det_hw, torch.Tensor) else det_hw
    hw = np.ascontiguousarray(np.asarray(hw).reshape(-1, 2), dtype=np.int32)
    if hw.shape[0] != M:
        raise ValueError("det_hw must be M x 2 = %d x 2, got %s" % (M, hw.shape))
    if M and (hw.min() < 1 or hw[:, 1].max() > RAGGED_MAX_WIDTH):
        raise ValueError("det_hw rows must be positive with widths up to %d, got heights "
                         "%d..%d, widths %d..%d" % (RAGGED_MAX_WIDTH, hw[:, 0].min(),
                                                    hw[:, 0].max(), hw[:, 1].min(),
                                                    hw[:, 1].max()))
    hw_t = torch.from_numpy(hw).to(m.device)
    cap = int(cap or (4 * (int(hw[:, 1].max()) if M else 1) + 2))
    while True:
        counts = torch.empty((M, cap), dtype=torch.int32, device=m.device)
        n = torch.empty((M,), dtype=torch.int32, device=m.device)
        check(lib().vd_segm_rle_ragged(m.data_ptr(), M, R, b.data_ptr(), b.shape[1],
                                       hw_t.data_ptr(), float(np.float32(thresh)),
                                       counts.data_ptr(), cap, n.data_ptr(), _stream()),
              "vd_segm_rle_ragged")
        need = int((-n).max().item()) if M else 0
        if need <= cap:
            return counts, n
        cap = need


def rle_strings(counts: torch.Tensor, n: torch.Tensor) -> list:
    """pycocotools rleToString of each row's counts[:n] on the device
    (vd_rle_strings): list of M ASCII strings, as segm_results stores them."""
    c = _need(counts, "counts", torch.int32)
    nn = _need(n, "n", torch.int32)
    M, cap = c.shape
    if M == 0:
        return []
    lens = torch.empty((M,), dtype=torch.int32, device=c.device)
    check(lib().vd_rle_strings(c.data_ptr(), nn.data_ptr(), M, cap, lens.data_ptr(), None,
                               _stream()), "vd_rle_strings")
    offs = np.zeros(M + 1, np.int64)
    np.cumsum(lens.cpu().numpy(), out=offs[1:])
    total = int(offs[-1])
    if total >= 2 ** 31:
        raise ValueError("RLE strings of %d detections exceed 2 GiB" % M)
    chars = torch.empty((max(total, 1),), dtype=torch.uint8, device=c.device)
    check(lib().vd_rle_strings(c.data_ptr(), nn.data_ptr(), M, cap, lens.data_ptr(),
                               chars.data_ptr(), _stream()), "vd_rle_strings")
    buf = chars[:total].cpu().numpy().tobytes()
    return [buf[offs[i]:offs[i + 1]].decode("ascii") for i in range(M)]


# --------------------------------------------------------------------------- #
# viz_mask_result: per-frame object-ID maps                                    #
# --------------------------------------------------------------------------- #
LABEL_MAX_CAP = 1024  # csrc/label_map.hip kLabelMaxCap


def label_lut(lut) -> np.ndarray:
    """A class -> written id table as the uint8 array vd_label_maps takes: 1-D, at
    least one entry, integers in [0, 255].  ValueError otherwise.  Needs no device."""
    a = lut.detach().cpu().numpy() if isinstance(lut, torch.Tensor) else np.asarray(lut)
    if a.ndim != 1 or a.size < 1:
        raise ValueError("lut must be 1-D with at least one entry, got shape %s"
                         % (tuple(a.shape),))
    if a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 255:
        raise ValueError("lut must hold integers in [0, 255]")
    return np.ascontiguousarray(a.astype(np.uint8))


def label_maps(masks: torch.Tensor, dets: torch.Tensor, classes: torch.Tensor,
               counts: torch.Tensor, im_h: int, im_w: int, score_thresh: float,
               gt_thresh: Optional[float] = None, bin_thresh: float = 0.5, lut=None, valid=None,
               rows_fit: bool = False):
    """viz_mask_result's maps of every frame in one call (vd_label_maps): masks [M,R,R]
    fp32 class-selected probabilities, rows in (frame, detection) order; dets [F,cap,5],
    classes [F,cap] int32, counts [F] int32 on the device (read there: no host read, so a
    run(sync=False) output is a valid input); valid [F,cap] uint8 / bool or None; lut a
    class -> id table (label_lut; a uint8 device tensor is used as it is) or None for the
    class itself.  -> (label, gt) uint8
    [F,im_h,im_w]: the id of the highest-scoring detection with score >= float32(
    score_thresh) whose pasted mask covers the pixel (equal scores: the higher row), and
    the same where that score > float32(gt_thresh); gt is None without gt_thresh.
    Rows past M are not painted: the counts are cut to the rows masks holds, on the device
    (a few small torch kernels), unless M >= F * cap or the caller knows that they fit
    (rows_fit: masks holds sum(clamp(counts, 0, cap)) rows, e.g. a completed step)."""
    lut_t = None
    if isinstance(lut, torch.Tensor) and lut.is_cuda and lut.dtype == torch.uint8 and \
            lut.dim() == 1 and lut.numel() >= 1:
        lut_t = lut.contiguous()  # already on the device: no copy, capturable
    elif lut is not None:
        lut_t = label_lut(lut)
    m = _need(masks, "masks")
    d, c, n = _need(dets, "dets"), _need(classes, "classes", torch.int32), \
        _need(counts, "counts", torch.int32)
    if d.dim() != 3 or d.shape[2] != 5:
        raise ValueError("dets must be F x cap x 5, got %s" % (tuple(d.shape),))
    F, cap = d.shape[0], d.shape[1]
    if tuple(c.shape) != (F, cap) or n.numel() != F:
        raise ValueError("label_maps: dets %s classes %s counts %s"
                         % (tuple(d.shape), tuple(c.shape), tuple(n.shape)))
    if m.dim() != 3 or m.shape[1] != m.shape[2]:
        raise ValueError("masks must be M x R x R, got %s" % (tuple(m.shape),))
    M, R = m.shape[0], m.shape[2]
    v = None
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or tuple(valid.shape) != (F, cap):
            raise ValueError("valid must be an F x cap tensor")
        v = _need(valid.to(torch.uint8), "valid", torch.uint8)
    label = torch.empty((F, int(im_h), int(im_w)), dtype=torch.uint8, device=d.device)
    gt = torch.empty_like(label) if gt_thresh is not None else None
    if F == 0:
        return label, gt
    if M < F * cap and not rows_fit:  # the counts may sum past the mask rows: cut them at M
        end = n.clamp(0, cap).cumsum(0)
        n = (end.clamp(max=M) - (end - n.clamp(0, cap)).clamp(max=M)).to(torch.int32)
    if isinstance(lut_t, np.ndarray):
        lut_t = torch.from_numpy(lut_t).to(d.device)
    ws = _ws(lib().vd_label_maps_workspace_size(F, cap), d.device)
    check(lib().vd_label_maps(
        m.data_ptr() if M else d.data_ptr(), R, d.data_ptr(), c.data_ptr(), n.data_ptr(),
        v.data_ptr() if v is not None else None, F, cap, int(im_h), int(im_w),
        float(np.float32(bin_thresh)), float(np.float32(score_thresh)),
        float(np.float32(gt_thresh if gt_thresh is not None else 0.0)),
        lut_t.data_ptr() if lut_t is not None else None,
        lut_t.numel() if lut_t is not None else 0,
        label.data_ptr(), gt.data_ptr() if gt is not None else None, ws.data_ptr(), ws.numel(),
        _stream()), "vd_label_maps")
    return label, gt


# --------------------------------------------------------------------------- #
# label maps as indexed PNG file images                                        #
# --------------------------------------------------------------------------- #
def label_png_bound(im_h: int, im_w: int) -> int:
    """vd_label_png_bound: the bytes no H x W label map's PNG can exceed, which is the
    per-frame capacity label_pngs allocates.  ValueError for a size the kernel does
    not serve (W in 1..4095, H in 1..16384).  Needs no device."""
    n = int(lib().vd_label_png_bound(int(im_h), int(im_w)))
    if n == 0:
        raise ValueError("label_png_bound: %d x %d is outside 1..16384 x 1..4095"
                         % (int(im_h), int(im_w)))
    return n


def label_pngs(labels: torch.Tensor, palette: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None):
    """Every frame's label map as a complete 8-bit indexed PNG file image, encoded on
    the device (vd_label_pngs): labels [F,H,W] uint8 on the device (label_maps' label
    or gt), palette [256,3] uint8 RGB (default: vis.davis_palette()), out an optional
    [F,cap] uint8 device buffer with cap >= label_png_bound(H, W).  -> (streams [F,cap]
    uint8, lengths [F] int32), both on the device: streams[f, :lengths[f]] is the file.
    No host read, so the call follows a run(sync=False) step and can be graph-captured
    (give `palette` as a device tensor then).  vis.png_bytes / vis.write_pngs bring
    the files to the host."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3:
        raise ValueError("labels must be an F x H x W tensor")
    F, H, W = (int(v) for v in labels.shape)
    cap = label_png_bound(H, W)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape[0] != F or \
                out.shape[1] < cap:
            raise ValueError("out must be F x cap uint8 with cap >= label_png_bound(%d, %d) = "
                             "%d, got %s" % (H, W, cap, tuple(getattr(out, "shape", ()))))
    lab = _need(labels, "labels", torch.uint8)
    if palette is None:
        from . import vis
        palette = vis.davis_palette().to(lab.device)
    if not isinstance(palette, torch.Tensor) or tuple(palette.shape) != (256, 3):
        raise ValueError("palette must be a 256 x 3 uint8 tensor")
    pal = _need(palette.to(lab.device), "palette", torch.uint8)
    if out is None:
        out = torch.empty((F, cap), dtype=torch.uint8, device=lab.device)
    elif not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 device tensor")
    lengths = torch.empty((F,), dtype=torch.int32, device=lab.device)
    if F == 0:
        return out, lengths
    ws = _ws(lib().vd_label_pngs_workspace(F, H, W), lab.device)
    check(lib().vd_label_pngs(lab.data_ptr(), F, H, W, pal.data_ptr(), out.data_ptr(),
                              out.shape[1], lengths.data_ptr(), ws.data_ptr(), ws.numel(),
                              _stream()), "vd_label_pngs")
    return out, lengths


# --------------------------------------------------------------------------- #
# the objects of a label map: boxes, areas, RLE                                #
# --------------------------------------------------------------------------- #
LABEL_OBJECTS_MAX_CAP = 255    # csrc/label_objects.hip kObjMaxCap
LABEL_OBJECTS_MAX_WIDTH = 8192  # kObjMaxW

_LABEL_OBJECT_FIELDS = (("ids", torch.uint8, ()), ("rects", torch.int32, (4,)),
                        ("areas", torch.int32, ()), ("boxes", torch.float32, (4,)))


def label_objects(labels: torch.Tensor, expand: Optional[float] = 0.05, remap255: bool = False,
                  obj_cap: int = 255, rle_cap: Optional[int] = None, want_rle: bool = True,
                  out: Optional[dict] = None) -> dict:
    """The objects of every frame's label map in one call (vd_label_objects): labels
    [F,H,W] uint8 on the device (label_maps' gt or label, or DAVIS annotations).  Per
    distinct non-zero value, ascending: ids [F,obj_cap] uint8, rects [F,obj_cap,4] int32
    (cv2.boundingRect), areas [F,obj_cap] int32, boxes [F,obj_cap,4] fp32 and counts [F]
    int32 -- (boxes, counts) is what FramePipeline.run takes as box_proposals --, and with
    want_rle rle_counts [F,obj_cap,rle_cap] int32 / rle_n [F,obj_cap] int32, the
    pycocotools mask.encode counts of (map == value) (rle_strings gives the strings);
    both None without want_rle.  expand=None: boxes (x, y, x + w, y + h) of get_bboxes /
    get_cls_mapper, every object kept; expand >= 0: add_gt_annotations_to_entry's
    expanded, clipped boxes in float64 and its validity filter (rows compacted).
    remap255: get_gt's rule for value 255 first.  A frame with more than obj_cap kept
    objects has counts[f] = -1 (raise_on_failed_counts).  Rows past a count are not
    written.
    Without `out` and `rle_cap` the call retries with a larger rle_cap when an object has
    more runs (one host read; first try 4 * W + 2).  With `out` (a dict of the output
    tensors, as a previous call returned them; reused, so the call can be captured) or an
    explicit rle_cap there is no host read: an object with more than rle_cap runs has
    rle_n = -n and no counts.
    Device footprint: rle_counts is F * obj_cap * rle_cap * 4 bytes -- 348 MB for 64 maps
    of 800 x 1333 at the defaults (obj_cap 255, rle_cap 4 * W + 2), five times the maps;
    only the rows below the counts are ever copied to the host.  Give the obj_cap the maps
    need (DAVIS: <= 10 objects; davis_db uses 32), and want_rle=False where only boxes are
    wanted: the RLE pass launches obj_cap x F workgroups, those past a count return at
    once."""
    lab = _need(labels, "labels", torch.uint8)
    if lab.dim() != 3:
        raise ValueError("labels must be F x H x W, got %s" % (tuple(lab.shape),))
    F, H, W = (int(v) for v in lab.shape)
    obj_cap = int(obj_cap)
    if not 1 <= obj_cap <= LABEL_OBJECTS_MAX_CAP:
        raise ValueError("label_objects: obj_cap = %d is outside 1..%d"
                         % (obj_cap, LABEL_OBJECTS_MAX_CAP))
    if H < 1 or W < 1 or W > LABEL_OBJECTS_MAX_WIDTH or H * W >= 2 ** 31 or F > 65535:
        raise ValueError("label_objects: %d maps of %d x %d are outside 1..65535 maps, width "
                         "1..%d, H * W < 2^31" % (F, H, W, LABEL_OBJECTS_MAX_WIDTH))
    if expand is not None and not float(expand) >= 0.0:
        raise ValueError("label_objects: expand = %r is neither None nor >= 0" % (expand,))
    ex = -1.0 if expand is None else float(expand)
    retry = out is None and rle_cap is None and want_rle
    dev = lab.device
    if out is not None:
        for name, dt, tail in _LABEL_OBJECT_FIELDS + (("counts", torch.int32, None),):
            t = out.get(name)
            want = (F,) if tail is None else (F, obj_cap) + tail
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
                raise ValueError("out[%r] must be %s" % (name, want))
            _need(t, "out[%r]" % name, dt)
        if want_rle:
            rc, rn = out.get("rle_counts"), out.get("rle_n")
            if not isinstance(rc, torch.Tensor) or rc.dim() != 3 or \
                    tuple(rc.shape[:2]) != (F, obj_cap) or rc.shape[2] < 1 or \
                    not isinstance(rn, torch.Tensor) or tuple(rn.shape) != (F, obj_cap):
                raise ValueError("out['rle_counts'] must be F x obj_cap x rle_cap and "
                                 "out['rle_n'] F x obj_cap")
            _need(rc, "out['rle_counts']", torch.int32)
            _need(rn, "out['rle_n']", torch.int32)
            if rle_cap is not None and int(rle_cap) != rc.shape[2]:
                raise ValueError("rle_cap = %d but out['rle_counts'] holds %d per object"
                                 % (int(rle_cap), rc.shape[2]))
            rle_cap = int(rc.shape[2])
        res = dict(out)
    else:
        res = {name: torch.empty((F, obj_cap) + tail, dtype=dt, device=dev)
               for name, dt, tail in _LABEL_OBJECT_FIELDS}
        res["counts"] = torch.empty((F,), dtype=torch.int32, device=dev)
    if not want_rle:
        res["rle_counts"] = res["rle_n"] = None
        cap = 0
    else:
        cap = int(rle_cap) if rle_cap is not None else 4 * W + 2
        if cap < 1:
            raise ValueError("label_objects: rle_cap = %d must be positive" % cap)
    if F == 0:
        if want_rle and out is None:
            res["rle_counts"] = torch.empty((0, obj_cap, cap), dtype=torch.int32, device=dev)
            res["rle_n"] = torch.empty((0, obj_cap), dtype=torch.int32, device=dev)
        return res
    ws = _ws(lib().vd_label_objects_workspace_size(F, H, W, obj_cap), dev)
    while True:
        if want_rle and out is None:
            res["rle_counts"] = torch.empty((F, obj_cap, cap), dtype=torch.int32, device=dev)
            res["rle_n"] = torch.empty((F, obj_cap), dtype=torch.int32, device=dev)
        check(lib().vd_label_objects(
            lab.data_ptr(), F, H, W, 1 if remap255 else 0, ex, obj_cap, cap,
            res["ids"].data_ptr(), res["rects"].data_ptr(), res["areas"].data_ptr(),
            res["boxes"].data_ptr(), res["counts"].data_ptr(),
            res["rle_counts"].data_ptr() if want_rle else None,
            res["rle_n"].data_ptr() if want_rle else None, ws.data_ptr(), ws.numel(),
            _stream()), "vd_label_objects")
        if not retry:
            return res
        # rows past a count hold no defined value: look at the written rows only
        live = torch.arange(obj_cap, device=dev)[None, :] < res["counts"][:, None]
        need = int(torch.where(live, -res["rle_n"], 0).max().item())
        if need <= cap:
            return res
        cap = need


# --------------------------------------------------------------------------- #
# keypoint_results: heatmap decode                                             #
# --------------------------------------------------------------------------- #
KEYPOINT_MAX_HEATMAP = 64  # csrc/keypoints.hip kKpMaxM
KEYPOINT_MAX_K = 32


def heatmaps_to_keypoints(maps: torch.Tensor, boxes: torch.Tensor,
                          min_size: int = 0) -> torch.Tensor:
    """heatmaps_to_keypoints (lib/utils/keypoints.py:103-157) on the device
    (vd_heatmaps_to_keypoints): maps [R,K,M,M] fp32 logits, boxes [R,>=4] fp32
    (x1, y1, x2, y2 first; a column view such as dets[:, 1:5] is read in place by
    its row stride) -> [R,4,K] fp32 rows (x, y, logit, prob).  No host read."""
    m = _need(maps, "maps")
    if m.dim() != 4 or m.shape[2] != m.shape[3]:
        raise ValueError("maps must be R x K x M x M, got %s" % (tuple(maps.shape),))
    R, K, M = m.shape[0], m.shape[1], m.shape[2]
    if M < 1 or M > KEYPOINT_MAX_HEATMAP or K < 1 or K > KEYPOINT_MAX_K:
        raise ValueError("heatmaps_to_keypoints: M = %d (<= %d), K = %d (<= %d)"
                         % (M, KEYPOINT_MAX_HEATMAP, K, KEYPOINT_MAX_K))
    if not isinstance(boxes, torch.Tensor) or not boxes.is_cuda or boxes.dtype != torch.float32:
        raise TypeError("boxes must be a float32 device tensor")
    if boxes.dim() != 2 or boxes.shape[0] != R or boxes.shape[1] < 4:
        raise ValueError("boxes must be R x >=4, got %s" % (tuple(boxes.shape),))
    b = boxes
    if b.stride(1) != 1 or (R > 1 and b.stride(0) < 4):
        b = b.contiguous()
    stride = b.stride(0) if R > 1 else 4  # one row: the stride is never applied
    out = torch.empty((R, 4, K), dtype=torch.float32, device=m.device)
    if R == 0:
        return out
    check(lib().vd_heatmaps_to_keypoints(m.data_ptr(), R, K, M, b.data_ptr(), int(stride),
                                         int(min_size), out.data_ptr(), _stream()),
          "vd_heatmaps_to_keypoints")
    return out


KPS_AUG_HEURS = {"HM_AVG": 0, "HM_MAX": 1}  # include/vosdet.h VD_KPS_AUG_*
KPS_AUG_MAX_VIEWS = 32


def _bits(flags, name, V):
    flags = [bool(f) for f in flags]
    if len(flags) != V:
        raise ValueError("%s: %d flags for %d views" % (name, len(flags), V))
    return sum(1 << i for i, f in enumerate(flags) if f)


def heatmaps_to_keypoints_aug(views, hflips, ds, us, boxes: torch.Tensor, min_size: int = 0,
                              heur: str = "HM_AVG", area_th=None, flip_perm=None,
                              want_combined: bool = False):
    """im_detect_keypoints_aug's combination (lib/core/test.py:630-651, 705-730) and
    keypoint_results' decode in one launch (vd_heatmaps_to_keypoints_aug).  views: the
    V <= 32 views' [R,K,M,M] fp32 logits as the network returned them, in heatmaps_ts
    order (the identity view first); hflips / ds / us: per view, whether it saw the
    flipped image (read as flip_heatmaps inverts it) and whether its scale is below /
    above TEST.SCALE; boxes [R,>=4]: the unflipped detection boxes; heur HM_AVG /
    HM_MAX; area_th: None, or KPS_AUG.AREA_TH for SCALE_SIZE_DEP (a box with
    area < area_th drops the ds views, any other the us views).  flip_perm: K channel
    indices, by default keypoints.get_keypoints()'s left/right swap when K == 17.
    -> [R,4,K] rows (x, y, logit, prob), or (that, the combined [R,K,M,M] maps) with
    want_combined.  No host read."""
    views = list(views)
    V = len(views)
    if V < 1 or V > KPS_AUG_MAX_VIEWS:
        raise ValueError("heatmaps_to_keypoints_aug: %d views (1..%d)" % (V, KPS_AUG_MAX_VIEWS))
    ms = [_need(v, "views[%d]" % i) for i, v in enumerate(views)]
    m = ms[0]
    if m.dim() != 4 or m.shape[2] != m.shape[3]:
        raise ValueError("views must be R x K x M x M, got %s" % (tuple(m.shape),))
    for i, v in enumerate(ms):
        if v.shape != m.shape or v.device != m.device:
            raise ValueError("views[%d] is %s on %s, views[0] %s on %s"
                             % (i, tuple(v.shape), v.device, tuple(m.shape), m.device))
    R, K, M = m.shape[0], m.shape[1], m.shape[2]
    if M < 1 or M > KEYPOINT_MAX_HEATMAP or K < 1 or K > KEYPOINT_MAX_K:
        raise ValueError("heatmaps_to_keypoints_aug: M = %d (<= %d), K = %d (<= %d)"
                         % (M, KEYPOINT_MAX_HEATMAP, K, KEYPOINT_MAX_K))
    if heur not in KPS_AUG_HEURS:
        raise ValueError("heatmaps_to_keypoints_aug: heur %r not in %s"
                         % (heur, sorted(KPS_AUG_HEURS)))
    hf, dsb, usb = _bits(hflips, "hflips", V), _bits(ds, "ds", V), _bits(us, "us", V)
    if (dsb | usb) & 1 or dsb & usb:
        raise ValueError("heatmaps_to_keypoints_aug: the identity view carries no ds / us tag "
                         "and no view carries both (ds %s, us %s)" % (list(ds), list(us)))
    if flip_perm is None:
        if K != 17:
            raise ValueError("heatmaps_to_keypoints_aug: K = %d needs an explicit flip_perm "
                             "(the default is the 17 COCO keypoints' left/right swap)" % K)
        from .keypoints import flip_permutation
        flip_perm = flip_permutation()
    perm = [int(p) for p in flip_perm]
    if len(perm) != K or any(p < 0 or p >= K for p in perm):
        raise ValueError("flip_perm must hold K = %d indices in [0, %d), got %s" % (K, K, perm))
    th = -1.0
    if area_th is not None:
        th = float(area_th)
        if not th >= 0 or float(np.float32(th)) != th:
            raise ValueError("area_th = %r must be a non-negative number that float32 holds "
                             "exactly" % (area_th,))
    if not isinstance(boxes, torch.Tensor) or not boxes.is_cuda or boxes.dtype != torch.float32:
        raise TypeError("boxes must be a float32 device tensor")
    if boxes.dim() != 2 or boxes.shape[0] != R or boxes.shape[1] < 4:
        raise ValueError("boxes must be R x >=4, got %s" % (tuple(boxes.shape),))
    b = boxes
    if b.stride(1) != 1 or (R > 1 and b.stride(0) < 4):
        b = b.contiguous()
    stride = b.stride(0) if R > 1 else 4
    out = torch.empty((R, 4, K), dtype=torch.float32, device=m.device)
    comb = torch.empty_like(m) if want_combined else None
    if R > 0:
        ptrs = (ctypes.c_void_p * V)(*[v.data_ptr() for v in ms])
        cperm = (ctypes.c_int32 * K)(*perm)
        check(lib().vd_heatmaps_to_keypoints_aug(
            ptrs, V, hf, dsb, usb, cperm, KPS_AUG_HEURS[heur], th, R, K, M, b.data_ptr(),
            int(stride), int(min_size), comb.data_ptr() if want_combined else None,
            out.data_ptr(), _stream()), "vd_heatmaps_to_keypoints_aug")
    return (out, comb) if want_combined else out


# --------------------------------------------------------------------------- #
# keypoint_results: OKS NMS                                                    #
# --------------------------------------------------------------------------- #
OKS_K = 17        # the reference's sigma table (csrc/oks_nms.hip kOksK)
OKS_MAX_D = 512   # detections per frame (kOksMaxD)

OksNmsResult = collections.namedtuple(
    "OksNmsResult", ["keep", "counts", "dets", "classes", "keyps", "scores"])


def _oks_arg(t, name: str, dtype, shape_ok, shape_text: str) -> None:
    """Host checks of one argument, the device last, each a ValueError naming it."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not shape_ok(t):
        raise ValueError("%s must be %s, got %s" % (name, shape_text, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _oks_device(named) -> None:
    dev = None
    for name, t in named:
        if not t.is_cuda:
            raise ValueError("%s must be a device (HIP) tensor; there is no CPU path" % name)
        if dev is not None and t.device != dev:
            raise ValueError("%s is on %s, not on %s like the other arguments"
                             % (name, t.device, dev))
        dev = t.device


def nms_oks_frames(keyps: torch.Tensor, dets: torch.Tensor, classes: torch.Tensor,
                   counts: torch.Tensor, thresh: float = 0.3,
                   counts_host: Optional[Sequence[int]] = None) -> OksNmsResult:
    """nms_oks (lib/utils/keypoints.py:225-266, applied at lib/core/test.py:864-870)
    for all F frames of a step on the device (vd_nms_oks_frames), no host read.
    keyps [rows, 4, 17] fp32 frame-major as heatmaps_to_keypoints writes them (frame
    f's rows start at the prefix sum of the non-negative counts), dets [F, D, 5],
    classes [F, D] int32, counts [F] int32; D <= 512.  Returns new tensors (the inputs
    are not modified): keep [F, D] int32 frame-local indices in kept order (-1 past
    the count), counts [F], dets / classes the kept rows in kept order, keyps
    [rows, 4, 17] the kept rows compacted frame-major (zeros past the total) and
    scores [F, D] the mean logits by input index.  Order: descending score, the
    higher index first among equal scores.  counts_host, when the caller has the
    counts on the host, lets the row total be checked against keyps here; the kernel
    itself never reads past keyps' rows."""
    _oks_arg(keyps, "keyps", torch.float32, lambda t: t.dim() == 3 and t.shape[1] == 4,
             "rows x 4 x K")
    if keyps.shape[2] != OKS_K:
        raise ValueError("keyps: K = %d, OKS NMS needs K == %d (the COCO sigma table)"
                         % (keyps.shape[2], OKS_K))
    _oks_arg(dets, "dets", torch.float32, lambda t: t.dim() == 3 and t.shape[2] == 5,
             "F x D x 5")
    F, D = dets.shape[0], dets.shape[1]
    _oks_arg(classes, "classes", torch.int32, lambda t: tuple(t.shape) == (F, D), "F x D")
    _oks_arg(counts, "counts", torch.int32, lambda t: tuple(t.shape) == (F,), "F")
    if D < 1 or D > OKS_MAX_D:
        raise ValueError("dets: D = %d, OKS NMS supports 1 <= D <= %d" % (D, OKS_MAX_D))
    rows = keyps.shape[0]
    if counts_host is not None:
        need = sum(max(int(c), 0) for c in counts_host)
        if len(counts_host) != F or need > rows:
            raise ValueError("keyps has %d rows, the counts %s need %d"
                             % (rows, list(counts_host), need))
    _oks_device([("keyps", keyps), ("dets", dets), ("classes", classes), ("counts", counts)])
    dev = keyps.device
    res = OksNmsResult(torch.empty((F, D), dtype=torch.int32, device=dev),
                       torch.empty((F,), dtype=torch.int32, device=dev),
                       torch.empty_like(dets), torch.empty_like(classes),
                       torch.empty_like(keyps),
                       torch.empty((F, D), dtype=torch.float32, device=dev))
    if F == 0:
        return res
    check(lib().vd_nms_oks_frames(keyps.data_ptr(), rows, OKS_K, dets.data_ptr(),
                                  classes.data_ptr(), counts.data_ptr(), F, D, float(thresh),
                                  res.keep.data_ptr(), res.counts.data_ptr(),
                                  res.dets.data_ptr(), res.classes.data_ptr(),
                                  res.keyps.data_ptr(), res.scores.data_ptr(), _stream()),
          "vd_nms_oks_frames")
    return res


def compute_oks(src_keypoints: torch.Tensor, src_roi: torch.Tensor,
                dst_keypoints: torch.Tensor) -> torch.Tensor:
    """compute_oks (lib/utils/keypoints.py:243-266) on the device (vd_compute_oks):
    src_keypoints [4, 17] fp32, src_roi [>=4] fp32 (x1, y1, x2, y2 first), dst_keypoints
    [N, 4, 17] fp32 -> [N] float64.  Only the source's box enters."""
    _oks_arg(src_keypoints, "src_keypoints", torch.float32,
             lambda t: t.dim() == 2 and t.shape[0] == 4, "4 x K")
    if src_keypoints.shape[1] != OKS_K:
        raise ValueError("src_keypoints: K = %d, OKS needs K == %d"
                         % (src_keypoints.shape[1], OKS_K))
    _oks_arg(src_roi, "src_roi", torch.float32, lambda t: t.dim() == 1 and t.shape[0] >= 4,
             "a vector of >= 4")
    _oks_arg(dst_keypoints, "dst_keypoints", torch.float32,
             lambda t: t.dim() == 3 and tuple(t.shape[1:]) == (4, OKS_K), "N x 4 x %d" % OKS_K)
    _oks_device([("src_keypoints", src_keypoints), ("src_roi", src_roi),
                 ("dst_keypoints", dst_keypoints)])
    N = dst_keypoints.shape[0]
    out = torch.empty((N,), dtype=torch.float64, device=dst_keypoints.device)
    if N:
        check(lib().vd_compute_oks(src_keypoints.data_ptr(), src_roi.data_ptr(),
                                   dst_keypoints.data_ptr(), N, OKS_K, out.data_ptr(),
                                   _stream()), "vd_compute_oks")
    return out


# --------------------------------------------------------------------------- #
# VOS temporal path: FlowAlign, GroupNorm epilogues, ConvGRU gates             #
# --------------------------------------------------------------------------- #
def _fmt(x: torch.Tensor, name: str) -> int:
    """Memory format of a 4-D fp32 device tensor as a vosdet layout code."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("%s must be a 4-D float32 device tensor" % name)
    if x.is_contiguous():
        return _lib.VD_LAYOUT_NCHW
    if x.is_contiguous(memory_format=torch.channels_last):
        return _lib.VD_LAYOUT_NHWC
    raise ValueError("%s must be contiguous (NCHW or channels_last)" % name)


def _like(x: torch.Tensor, layout: int, name: str) -> torch.Tensor:
    """x in the memory format `layout` (a copy only if it is not already)."""
    want = torch.channels_last if layout == _lib.VD_LAYOUT_NHWC else torch.contiguous_format
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("%s must be a float32 device tensor" % name)
    return x if x.is_contiguous(memory_format=want) else x.contiguous(memory_format=want)


def _empty_as(x: torch.Tensor, layout: int, shape=None) -> torch.Tensor:
    shape = tuple(x.shape) if shape is None else shape
    fmt = torch.channels_last if layout == _lib.VD_LAYOUT_NHWC else torch.contiguous_format
    return torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=fmt)


def flow_align(features: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """FlowAlignFunction.forward (lib_vos/vos_model/flow_align/functions/flow_align.py:13-30):
    features B x C x H x W (NCHW, or channels_last -> the NHWC kernel), flow
    B x 2 x H x W at the feature resolution.  Output in the features' format."""
    lay = _fmt(features, "features")
    fl = _need(flow, "flow")
    B, C, H, W = features.shape
    if tuple(fl.shape) != (B, 2, H, W):
        raise ValueError("flow must be B x 2 x H x W = %s, got %s" % ((B, 2, H, W),
                                                                      tuple(fl.shape)))
    out = _empty_as(features, lay)
    check(lib().vd_flow_align_forward(features.data_ptr(), fl.data_ptr(), B, C, H, W, lay,
                                      out.data_ptr(), _stream()), "vd_flow_align_forward")
    return out


FLOW_STRIDES = (4, 8, 16, 32, 64)  # the FlowAlign levels, finest first (P2 .. P6)
FLOW_TILE = 64  # vd_flow_to_levels: one workgroup per 64 x 64 blob tile


def flow_to_levels(raw_flow: torch.Tensor, im_scale: float, Hp: int, Wp: int,
                   strides: Sequence[int] = FLOW_STRIDES, want_blob: bool = False):
    """flo_to_blob (lib/utils/blob.py:63-75) + every FlowAlign.conv_flow_downsample
    in one launch (vd_flow_to_levels).  raw_flow: F x H x W x 2 fp32 as read from
    the .flo file (u then v per pixel); Hp, Wp: the padded blob size, multiples of
    64.  Returns (levels, blob): levels[i] is the F x 2 x Hp/k x Wp/k flow of
    strides[i] = k, blob the F x 2 x Hp x Wp data_flow when want_blob, else None."""
    if not isinstance(raw_flow, torch.Tensor):
        raise TypeError("raw_flow must be a torch.Tensor")
    if raw_flow.dim() != 4 or raw_flow.shape[3] != 2 or min(raw_flow.shape) < 1:
        raise ValueError("raw_flow must be F x H x W x 2, got %s" % (tuple(raw_flow.shape),))
    Hp, Wp = int(Hp), int(Wp)
    if Hp % FLOW_TILE or Wp % FLOW_TILE:
        raise ValueError("flow_to_levels: the blob %dx%d is not a multiple of %d"
                         % (Hp, Wp, FLOW_TILE))
    strides = tuple(int(k) for k in strides)
    if any(k not in FLOW_STRIDES for k in strides) or len(set(strides)) != len(strides):
        raise ValueError("strides must be distinct values of %s, got %s" % (FLOW_STRIDES, strides))
    if not im_scale > 0:
        raise ValueError("im_scale must be positive, got %r" % (im_scale,))
    rf = _need(raw_flow, "raw_flow")
    F, H, W, _ = rf.shape
    Hr, Wr = resized_hw(H, W, im_scale)
    if Hr < 1 or Wr < 1 or Hp < Hr or Wp < Wr:
        raise ValueError("blob %dx%d does not hold the resized flow %dx%d" % (Hp, Wp, Hr, Wr))
    levels = [torch.empty((F, 2, Hp // k, Wp // k), dtype=torch.float32, device=rf.device)
              for k in strides]
    ptr = {k: t.data_ptr() for k, t in zip(strides, levels)}
    blob = (torch.empty((F, 2, Hp, Wp), dtype=torch.float32, device=rf.device)
            if want_blob else None)
    check(lib().vd_flow_to_levels(rf.data_ptr(), F, H, W, float(im_scale), Hr, Wr, Hp, Wp,
                                  *[ptr.get(k) for k in FLOW_STRIDES],
                                  blob.data_ptr() if want_blob else None, _stream()),
          "vd_flow_to_levels")
    return levels, blob


def _delta_flow_weight(w: torch.Tensor) -> torch.Tensor:
    return w.detach().permute(2, 3, 0, 1).reshape(18, w.shape[1]).contiguous()


def delta_flow_weight_cached(w: torch.Tensor) -> torch.Tensor:
    """A Conv_Delta_Flows_Features weight [2, C, 3, 3] in vd_delta_flow_features'
    layout [18, C] (row (ky * 3 + kx) * 2 + o), through _weight_cached."""
    return _weight_cached(w, _delta_flow_weight)


def delta_flow_features(feats: Sequence[torch.Tensor], weights: Sequence[torch.Tensor],
                        state: Sequence[torch.Tensor], valid: torch.Tensor,
                        layout: Optional[int] = None):
    """The delta-flow head's per-level flow features (vos_model_builder.py:314-323)
    for all levels in one launch (vd_delta_flow_features).  feats[i]: B x C x H_i x W_i
    (NCHW or channels_last, all the same; layout None = read it off the last, largest map);
    weights[i]: the level's Conv2d weight [2, C, 3, 3]; state[i]: the previous
    feature B x 2 x H_i x W_i, updated in place to tanh(conv(feats[i])); valid: B
    int32 on the device, 0 = the row has no previous feature.  Returns the deltas
    (new - previous where valid, else 0), one B x 2 x H_i x W_i tensor per level."""
    n = len(feats)
    if not 1 <= n <= _lib.VD_MAX_LEVELS:
        raise ValueError("feats must hold 1 .. %d levels, got %d" % (_lib.VD_MAX_LEVELS, n))
    if len(weights) != n:
        raise ValueError("weights must hold one tensor per level (%d), got %d" % (n, len(weights)))
    if len(state) != n:
        raise ValueError("state must hold one tensor per level (%d), got %d" % (n, len(state)))
    lay = _fmt(feats[-1], "feats[-1]") if layout is None else int(layout)
    if lay not in (_lib.VD_LAYOUT_NCHW, _lib.VD_LAYOUT_NHWC):
        raise ValueError("layout must be VD_LAYOUT_NCHW or VD_LAYOUT_NHWC, got %r" % (layout,))
    B, C = int(feats[0].shape[0]), int(feats[0].shape[1])
    if C % 64 or C > 512:
        raise ValueError("feats: C must be a multiple of 64 and at most 512, got %d" % C)
    if not isinstance(valid, torch.Tensor) or not valid.is_cuda or valid.dtype != torch.int32 \
            or tuple(valid.shape) != (B,) or not valid.is_contiguous():
        raise ValueError("valid must be a contiguous int32 device vector of B = %d rows" % B)
    arr = (_lib.VdDeltaFlowLevel * n)()
    keep, deltas = [], []
    for i in range(n):
        f = feats[i]
        if f.dim() != 4 or int(f.shape[0]) != B or int(f.shape[1]) != C:
            raise ValueError("feats[%d] must be %d x %d x H x W, got %s" % (i, B, C,
                                                                            tuple(f.shape)))
        f = _like(f, lay, "feats[%d]" % i)
        H, W = int(f.shape[2]), int(f.shape[3])
        w = weights[i]
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != (2, C, 3, 3) or not w.is_cuda \
                or w.dtype != torch.float32:
            raise ValueError("weights[%d] must be a float32 device tensor [2, %d, 3, 3]" % (i, C))
        st = state[i]
        if not isinstance(st, torch.Tensor) or not st.is_cuda or st.dtype != torch.float32 \
                or tuple(st.shape) != (B, 2, H, W) or not st.is_contiguous():
            raise ValueError("state[%d] must be a contiguous float32 device tensor %s"
                             % (i, (B, 2, H, W)))
        wp = delta_flow_weight_cached(w)
        d = torch.empty((B, 2, H, W), dtype=torch.float32, device=f.device)
        arr[i] = _lib.VdDeltaFlowLevel(f.data_ptr(), H, W, wp.data_ptr(), st.data_ptr(),
                                       d.data_ptr())
        keep.append((f, wp))
        deltas.append(d)
    check(lib().vd_delta_flow_features(arr, n, B, C, lay, valid.data_ptr(), _stream()),
          "vd_delta_flow_features")
    return deltas


def delta_flow_to_levels(deltas: Sequence[torch.Tensor], Hp: int, Wp: int,
                         want_blob: bool = False):
    """The rest of the delta-flow head in one launch (vd_delta_flow_to_levels):
    deltas [P6 .. P2] (B x 2 x Hp/k x Wp/k, k = 64 .. 4) bilinearly upsampled to the
    blob, divided by their scales and summed (data_flow, vos_model_builder.py:
    319-323), then every FlowAlign.conv_flow_downsample.  Returns (levels, blob):
    levels[i] the flow of FlowAligns[i] (strides 64 .. 4), blob the B x 2 x Hp x Wp
    data_flow when want_blob, else None (never written)."""
    Hp, Wp = int(Hp), int(Wp)
    if Hp < 1 or Wp < 1 or Hp % FLOW_TILE or Wp % FLOW_TILE:
        raise ValueError("delta_flow_to_levels: the blob %dx%d is not a multiple of %d"
                         % (Hp, Wp, FLOW_TILE))
    if len(deltas) != 5:
        raise ValueError("deltas must hold 5 maps (P6 .. P2), got %d" % len(deltas))
    B = int(deltas[0].shape[0]) if isinstance(deltas[0], torch.Tensor) and deltas[0].dim() == 4 \
        else 0
    ds = []
    for i, k in enumerate(FLOW_STRIDES[::-1]):
        d = _need(deltas[i], "deltas[%d]" % i)
        if tuple(d.shape) != (B, 2, Hp // k, Wp // k) or B < 1:
            raise ValueError("deltas[%d] must be B x 2 x %d x %d, got %s"
                             % (i, Hp // k, Wp // k, tuple(d.shape)))
        ds.append(d)
    dev = ds[0].device
    levels = [torch.empty((B, 2, Hp // k, Wp // k), dtype=torch.float32, device=dev)
              for k in FLOW_STRIDES[::-1]]
    blob = torch.empty((B, 2, Hp, Wp), dtype=torch.float32, device=dev) if want_blob else None
    check(lib().vd_delta_flow_to_levels(*[d.data_ptr() for d in ds], B, Hp, Wp,
                                        *[l.data_ptr() for l in levels],
                                        blob.data_ptr() if want_blob else None, _stream()),
          "vd_delta_flow_to_levels")
    return levels, blob


def flow_align_backward(grad_out, features, flow):
    g = _need(grad_out, "grad_out")
    f = _need(features, "features")
    fl = _need(flow, "flow")
    B, C, H, W = f.shape
    gf = torch.zeros_like(f)
    gfl = torch.zeros((B, 2, H, W), dtype=torch.float32, device=f.device)
    check(lib().vd_flow_align_backward(g.data_ptr(), f.data_ptr(), fl.data_ptr(), B, C, H, W,
                                       gf.data_ptr(), gfl.data_ptr(), _stream()),
          "vd_flow_align_backward")
    return gf, gfl


class FlowAlignFunction(torch.autograd.Function):
    """functions/flow_align.py:7-45 (static autograd Function, as the reference).
    CPU tensors raise like the reference's NotImplementedError branch (:28-29)."""

    @staticmethod
    def forward(ctx, features, flows):
        if not features.is_cuda:
            raise NotImplementedError
        ctx.save_for_backward(features, flows)
        return flow_align(features, flows)

    @staticmethod
    def backward(ctx, grad_output):
        features, flows = ctx.saved_tensors
        return flow_align_backward(grad_output, features, flows)


_ACT = {None: 0, "none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}


def group_norm_act(x: torch.Tensor, num_groups: int, gamma: torch.Tensor, beta: torch.Tensor,
                   eps: float = 1e-5, x2: Optional[torch.Tensor] = None, residual=None,
                   residual_gn=None, upsample_residual: bool = False, act=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(GN(x [+ x2]) + residual) in one statistics + one apply pass
    (vd_group_norm_act).  residual_gn = (gamma_r, beta_r) normalises the residual
    with its own statistics (basic_gn_shortcut).  Works on NCHW or channels_last
    tensors; the output keeps x's memory format.  out may be x (in place)."""
    lay = _fmt(x, "x")
    B, C, H, W = x.shape
    if x2 is not None:
        x2 = _like(x2, lay, "x2")
    mode = 0
    res = None
    if residual is not None:
        mode = 3 if residual_gn is not None else (2 if upsample_residual else 1)
        want = (B, C, H // 2, W // 2) if mode == 2 else (B, C, H, W)
        if tuple(residual.shape) != want:
            raise ValueError("residual shape %s, expected %s" % (tuple(residual.shape), want))
        res = _like(residual, lay, "residual")
    if out is None:
        out = _empty_as(x, lay)
    rg, rb = residual_gn if residual_gn is not None else (None, None)
    nws = lib().vd_group_norm_workspace_size(B, num_groups) * (2 if mode == 3 else 1)
    ws = _ws(nws, x.device)
    check(lib().vd_group_norm_act(
        x.data_ptr(), x2.data_ptr() if x2 is not None else None, B, C, H, W, int(num_groups),
        float(eps), gamma.data_ptr(), beta.data_ptr(), res.data_ptr() if res is not None else None,
        mode, rg.data_ptr() if rg is not None else None, rb.data_ptr() if rb is not None else None,
        _ACT[act], lay, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
        "vd_group_norm_act")
    return out


def convgru_gates(zx, rx, h, zh, rh, num_groups, gamma_z, beta_z, gamma_r, beta_r, eps=1e-5):
    """(z, h*r) of convgrucell.py:85-87 from the six convolution outputs; with
    h None (zero state) returns (z, None)."""
    lay = _fmt(zx, "zx")
    B, C, H, W = zx.shape
    z = _empty_as(zx, lay)
    hr = _empty_as(zx, lay) if h is not None else None
    ws = _ws(2 * lib().vd_group_norm_workspace_size(B, num_groups), zx.device)
    ptr = lambda t: _like(t, lay, "t").data_ptr() if t is not None else None  # noqa: E731
    check(lib().vd_convgru_gates(
        ptr(zh), zx.data_ptr(), ptr(rh), ptr(rx), ptr(h), B, C, H, W, int(num_groups),
        float(eps), gamma_z.data_ptr(), beta_z.data_ptr(), gamma_r.data_ptr(), beta_r.data_ptr(),
        lay, z.data_ptr(), hr.data_ptr() if hr is not None else None, ws.data_ptr(), ws.numel(),
        _stream()), "vd_convgru_gates")
    return z, hr


def convgru_update(hx, hh, z, h, num_groups, gamma_h, beta_h, finer=None, eps=1e-5,
                   out: Optional[torch.Tensor] = None):
    """hn = (1-z)*h + z*tanh(GN_h(hh + hx)) (convgrucell.py:88-91), fused with the
    VOS fusion hn/2 + bilinear_0.5x(finer)/2 (vos_model_builder.py:341-342)."""
    lay = _fmt(hx, "hx")
    B, C, H, W = hx.shape
    if finer is not None and tuple(finer.shape) != (B, C, 2 * H, 2 * W):
        raise ValueError("finer level must be %s, got %s" % ((B, C, 2 * H, 2 * W),
                                                             tuple(finer.shape)))
    if out is None:
        out = _empty_as(hx, lay)
    ws = _ws(lib().vd_group_norm_workspace_size(B, num_groups), hx.device)
    ptr = lambda t: _like(t, lay, "t").data_ptr() if t is not None else None  # noqa: E731
    check(lib().vd_convgru_update(
        ptr(hh), hx.data_ptr(), ptr(z), ptr(h), ptr(finer), B, C, H, W, int(num_groups),
        float(eps), gamma_h.data_ptr(), beta_h.data_ptr(), lay, out.data_ptr(), ws.data_ptr(),
        ws.numel(), _stream()), "vd_convgru_update")
    return out
