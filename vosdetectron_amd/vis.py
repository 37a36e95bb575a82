"""viz_mask_result (lib/utils/vis.py:119-157) from device tensors.

The reference decodes every detection's RLE into an H x W plane and paints the
planes in ascending score order: outImg[mask > 0] = class for score >= thresh,
rtv_gt likewise for score > rvt_cls_threshold, and rtv_bboxs[class] collects the
boxes painted into rtv_gt.  Here both maps come from one vd_label_maps launch
(ops.label_maps) over the class-selected mask probabilities; the box lists are
made on the host from the detection rows.

Two rules are this project's own and are written down in DESIGN.md:
  * thresholds are compared in float32 (`np.float32 < python float` under NumPy >= 2);
  * among equal scores the higher row index is painted later (np.argsort is not
    stable, so the reference defines no order for ties).
Engine outputs: engine.frame_label_maps paints every frame of a step at once.
"""
import numpy as np
import torch

from . import ops


def painting_order(scores, thresh) -> np.ndarray:
    """Row indices in painting order: ascending float32 score, equal scores by
    ascending row (stable), rows with score < float32(thresh) left out."""
    s = np.asarray(scores, np.float32)
    order = np.argsort(s, kind="stable")
    return order[~(s[order] < np.float32(thresh))]


def viz_mask_result(masks: torch.Tensor, dets: torch.Tensor, classes: torch.Tensor, im_hw,
                    thresh: float = 0.9, rvt_cls_threshold: float = 0, bin_thresh: float = 0.5,
                    lut=None):
    """One frame: masks [n,R,R] fp32 class-selected probabilities, dets [n,5]
    (x1, y1, x2, y2, score), classes [n] int32, all on the device; im_hw the frame's
    (H, W).  Returns the reference's (rtv_gt, rtv_bboxs, outImg): two H x W uint8 numpy
    maps and a list of 256 lists, rtv_bboxs[c] the float32 boxes of class c with
    score >= thresh and score > rvt_cls_threshold in painting order.  lut maps the
    class to the id written into the maps (default: the class itself)."""
    n = int(dets.shape[0])
    H, W = int(im_hw[0]), int(im_hw[1])
    d = dets.reshape(1, n, 5) if n else dets.new_zeros((1, 1, 5))
    c = classes.reshape(1, n) if n else classes.new_zeros((1, 1))
    counts = torch.full((1,), n, dtype=torch.int32, device=dets.device)
    label, gt = ops.label_maps(masks, d, c, counts, H, W, thresh, rvt_cls_threshold, bin_thresh,
                               lut)
    rows, cls = dets.cpu().numpy(), classes.cpu().numpy()
    rtv_bboxs = [[] for _ in range(256)]
    for i in painting_order(rows[:, 4], thresh):
        if rows[i, 4] > np.float32(rvt_cls_threshold) and 0 <= cls[i] < 256:
            rtv_bboxs[int(cls[i])].append(rows[i, :4])
    return gt[0].cpu().numpy(), rtv_bboxs, label[0].cpu().numpy()


# --------------------------------------------------------------------------- #
# the annotation files (img_saver) and the colour overlay                      #
# --------------------------------------------------------------------------- #
def davis_palette() -> torch.Tensor:
    """[256,3] uint8 RGB: the PASCAL VOC colour map, which DAVIS 2017 annotations
    carry.  Bit k of (i >> 3j) goes to bit 7 - j of channel k, j = 0..7, so the first
    entries are (0,0,0), (128,0,0), (0,128,0), (128,128,0), (0,0,128).  The DAVIS
    toolkit's own palette file was not at hand when this was written: equality with
    it, entry for entry, is not pinned by any test."""
    i = np.arange(256)
    pal = np.zeros((256, 3), np.uint8)
    for j in range(8):
        for k in range(3):
            pal[:, k] |= ((((i >> (3 * j)) >> k) & 1) << (7 - j)).astype(np.uint8)
    return torch.from_numpy(pal)


def png_bytes(streams: torch.Tensor, lengths: torch.Tensor):
    """ops.label_pngs' result on the host: a list of F `bytes`, each a complete PNG
    file.  One small read of lengths, then one copy of streams[:, :lengths.max()]."""
    n = lengths.cpu().numpy()
    if n.size == 0:
        return []
    buf = streams[:, :int(n.max())].cpu().numpy()
    return [buf[f, :int(n[f])].tobytes() for f in range(n.size)]


def write_pngs(paths, streams: torch.Tensor, lengths: torch.Tensor) -> None:
    """Write frame f's file to paths[f] (img_saver of viz_mask_result for a whole step)."""
    files = png_bytes(streams, lengths)
    if len(paths) != len(files):
        raise ValueError("%d paths for %d frames" % (len(paths), len(files)))
    for path, data in zip(paths, files):
        with open(path, "wb") as fh:
            fh.write(data)


def label_colors(label: torch.Tensor, palette: torch.Tensor) -> torch.Tensor:
    """viz_mask_result's clr_mask: label [.., H, W] uint8 -> [.., H, W, 3] uint8 BGR, as
    cv2.imread of the written annotation file gives.  CPU or device tensors."""
    pal = palette.to(label.device)
    return pal[label.long()].flip(-1)


def overlay(frames_bgr: torch.Tensor, clr_bgr: torch.Tensor) -> torch.Tensor:
    """The online loop's blend (lib_vos/tools/train_davis_online.py:605):
    (1.0 * im + 0.4 * clr).clip(max=255).astype(uint8) on the RGB views of two uint8
    [.., H, W, 3] BGR images -> [.., H, W, 3] uint8 RGB.  Evaluated in float64 as numpy
    does; the conversion truncates.  CPU or device tensors."""
    im = frames_bgr.flip(-1).to(torch.float64)
    clr = clr_bgr.flip(-1).to(torch.float64)
    return (1.0 * im + 0.4 * clr).clamp(max=255).to(torch.uint8)
