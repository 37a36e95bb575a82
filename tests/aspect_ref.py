"""numpy restatement of the aspect-ratio views of the test-time augmentation (TEST
INFRASTRUCTURE ONLY): lib/utils/image.py:27-32 (aspect_ratio_rel), lib/utils/boxes.py:
269-274 (aspect_ratio), lib/core/test.py:330-363, 509-526, 684-702.

cv2 is not importable here, so `resize_width_u8` restates OpenCV's 8-bit INTER_LINEAR
path with dsize given, for a resize of the width alone (imgproc/src/resize.cpp:
fixed-point coefficient tables with INTER_RESIZE_COEF_SCALE = 2048, HResizeLinear in
int32, VResizeLinear's FixedPtCast); parity against an executed cv2 is unpinned, as for
oracle.cv2_resize_fx.  Nothing here imports the product's kernels.
"""
import numpy as np

from oracle import oracle as orc


def aspect_width(im_w, ar):
    """image.py:30."""
    return int(round(ar * im_w))


def stage1_coeffs(W, War):
    """Per column of im_ar: (sx, sx1, a0, a1), the taps and int16 coefficients."""
    inv = float(War) / float(W)
    scale_x = 1.0 / inv
    dx = np.arange(War)
    fx = ((dx + 0.5) * scale_x - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    lo = sx < 0
    fx[lo], sx[lo] = 0, 0
    hi = sx >= W - 1
    fx[hi], sx[hi] = 0, W - 1
    # cvRound of the float product: round half to even, each coefficient on its own
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int16)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int16)
    return sx, np.minimum(sx + 1, W - 1), a0, a1


def resize_width_u8(im, War):
    """cv2.resize(im, dsize=(War, H)) for an H x W x C uint8 image (INTER_LINEAR)."""
    im = np.asarray(im)
    assert im.dtype == np.uint8
    sx, sx1, a0, a1 = stage1_coeffs(im.shape[1], War)
    ex = (slice(None),) + (None,) * (im.ndim - 2)
    D = im[:, sx].astype(np.int32) * a0.astype(np.int32)[ex] \
        + im[:, sx1].astype(np.int32) * a1.astype(np.int32)[ex]
    # the vertical pass, coefficients (2048, 0): ((2048 * (D >> 4)) >> 16) = D >> 9
    return np.clip(((D >> 9) + 2) >> 2, 0, 255).astype(np.uint8)


def aspect_ratio_rel(im, ar):
    """image.py:27-32."""
    return resize_width_u8(im, aspect_width(im.shape[1], ar))


def view_image(im, ar, hflip):
    """The image the network sees: im_ar, flipped after the resize (test.py:296)."""
    im_ar = aspect_ratio_rel(im, ar)
    return np.ascontiguousarray(im_ar[:, ::-1]) if hflip else im_ar


def view_blob(frames, ar, hflip, target_scale, max_size, stride):
    """F x 3 x Hp x Wp float32 blob of an aspect-ratio view and its im_scale:
    get_image_blob of each frame's view_image."""
    blobs, scale = [], None
    for im in frames:
        b, scale, _ = orc.get_image_blob(view_image(im, ar, hflip), target_scale, max_size,
                                         stride)
        blobs.append(b[0])
    return np.stack(blobs), scale


def aspect_ratio(boxes, ar):
    """boxes.py:269-274."""
    boxes_ar = boxes.copy()
    boxes_ar[:, 0::4] = ar * boxes[:, 0::4]
    boxes_ar[:, 2::4] = ar * boxes[:, 2::4]
    return boxes_ar


def flip_boxes(boxes, im_width):
    """boxes.py:261-266."""
    boxes_flipped = boxes.copy()
    boxes_flipped[:, 0::4] = im_width - boxes[:, 2::4] - 1
    boxes_flipped[:, 2::4] = im_width - boxes[:, 0::4] - 1
    return boxes_flipped


def decode_view(rois, deltas, im_scale, H, W, ar, hflip, weights=(10., 10., 5., 5.)):
    """im_detect_bbox's decode (test.py:157-179) on im_ar, im_detect_bbox_hflip's
    inversion (:308-309) and im_detect_bbox_aspect_ratio's (:361) of one view: rois
    [n, 5] in the view's blob coordinates -> boxes [n, 4K] on the original frame.
    ar None: a plain view."""
    Wv = W if ar is None else aspect_width(W, ar)
    boxes = rois[:, 1:5] / float(im_scale)  # a Python float, as get_target_scale returns
    pred = orc.clip_tiled_boxes(orc.bbox_transform(boxes, deltas, weights), (H, Wv))
    if hflip:
        pred = flip_boxes(pred, Wv)
    return pred if ar is None else aspect_ratio(pred, 1.0 / ar)


def head_boxes(boxes, W, ar, hflip):
    """The boxes a mask / keypoint view's head is given (test.py:513-518, 689-694)."""
    if ar is not None:
        boxes = aspect_ratio(boxes, ar)
        W = aspect_width(W, ar)
    return flip_boxes(boxes, W) if hflip else boxes


def head_rois(boxes, im_scale):
    """_get_rois_blob (test.py:896-925) for one image: [0, boxes * im_scale] float32."""
    r = np.hstack([np.zeros((boxes.shape[0], 1)),
                   boxes.astype(np.float64) * float(im_scale)])
    return r.astype(np.float32)
