"""Device-resident per-frame inference engine (the hot path).

Replaces the host-driven chain of lib/core/test.py im_detect_all (:50-111):
im_detect_bbox (:128-190) -> box_results_with_nms_and_limit (:733-797) ->
im_detect_mask (:366-402), for a batch of F frames already resident in HBM:

  u8 frames --vd_image_to_blob--> blob --PyTorch ResNet-FPN--> P2..P6
  --PyTorch RPN convs--> vd_generate_proposals (all levels, all frames)
  --> vd_collect_distribute --> vd_roi_align_fpn (one launch, NHWC pyramid)
  --> PyTorch fc6/fc7/cls/bbox --> vd_box_detections (decode, clip, class NMS,
  top-100) --> vd_mask_rois (mask batch of F x DETECTIONS_PER_IM rows from the
  device counts) --> vd_roi_align_fpn 14x14 --> PyTorch mask head -->
  class-selected 28x28.

The reference crosses host<->device 5+5 times in proposals alone and twice per
roi_feature_transform; here nothing inside the step reads the host: the
detection counts are read once after the step is queued (complete()).  Outputs match the reference's
`cls_boxes` rows (class-major, proposal order) and the class-selected masks
that segm_results consumes; `frame_segms` runs segm_results' paste + RLE on
the device (segm.py).  RaggedFramePipeline runs frames of different sizes in one
step (im_list_to_blob, lib/utils/blob.py:86-114): the per-frame geometry lives in a
RaggedBatch on the device, vd_image_resize_to_blob_ragged builds the blob.
KeypointFramePipeline runs the Keypoint R-CNN configs: after misc_bbox, the pose head
and vd_heatmaps_to_keypoints (im_detect_keypoints + keypoint_results, test.py:97-107)
take the mask stage's place; frame_keypoints groups the result as cls_keyps.
KeypointFramePipeline(nms_oks=...) adds keypoint_results' OKS NMS (vd_nms_oks_frames).
KeypointAugFramePipeline runs the keypoint configs with TEST.BBOX_AUG / TEST.KPS_AUG
(im_detect_keypoints_aug, test.py:567-730): vd_heatmaps_to_keypoints_aug combines the
views' heatmaps inside the decode.

All of them run FramePipeline._run -- box pass, heads over the head views, complete() --
and override the part they change (see FramePipeline; C4FramePipeline has its own _run).
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from . import ops


class StageTimer:
    """utils/timer.Timer's accounting (total_time, calls, average_time) fed with
    HIP-event stage times instead of time.time() tic/toc."""

    def __init__(self, name: str):
        self.name = name
        self.total_time = 0.
        self.calls = 0
        self.average_time = 0.

    def add(self, seconds: float):
        self.total_time += seconds
        self.calls += 1
        self.average_time = self.total_time / self.calls


def nms_options(cfg) -> dict:
    """TEST.SOFT_NMS / TEST.BBOX_VOTE (lib/core/test.py:756-776) as box_detections
    keywords (empty when both are off: the stock vd_box_detections).  The
    reference never passes TEST.BBOX_VOTE.SCORING_METHOD_BETA to box_voting
    (test.py:770-775, vos_test.py:786-791), so beta stays 1.0 here too."""
    tst = cfg.TEST
    opts = {}
    if tst.SOFT_NMS.ENABLED:
        opts.update(soft_nms=tst.SOFT_NMS.METHOD, soft_nms_sigma=tst.SOFT_NMS.SIGMA)
    if tst.BBOX_VOTE.ENABLED:
        opts.update(bbox_vote=tst.BBOX_VOTE.SCORING_METHOD,
                    bbox_vote_thresh=tst.BBOX_VOTE.VOTE_TH,
                    bbox_vote_beta=1.0)
    return opts


class _ViewGeom:
    """Blob geometry of frames of one size at one view (scale, max_size, hflip), the
    identity view of a plain step or a test-time-augmentation view (lib/utils/blob.py:
    37-161): get_target_scale, cv2.resize to round(H*s) x round(W*s) (done on the device
    when s != 1), pad to `stride` (get_max_shape), and the per-frame rows the proposal,
    detection and RoI kernels read -- the fields a RaggedBatch carries per frame.

    An aspect-ratio view (scale, max_size, hflip, ar) (lib/core/test.py:330-363) is the
    geometry of im_ar, the frame with its width resized to War = int(round(ar * W))
    (lib/utils/image.py:27-32): scale, Hr / Wr / Hp / Wp and im_hw = (H, War) come from
    (H, War); ar is the ratio (None on any other view), x_inv = float32(1.0 / ar) the
    factor that maps the view's boxes back, flip_w the width a flip of the view's boxes
    uses (War; W on any other view)."""

    def __init__(self, view, H, W, stride, F, device):
        self.view, self.F = view, F
        self.hflip = bool(view[2])
        self.ar = float(view[3]) if len(view) > 3 else None
        self.x_inv = None
        if self.ar is not None:
            if not (self.ar > 0.0 and math.isfinite(self.ar)):
                raise ValueError("aspect-ratio view %r: the ratio is not a positive finite "
                                 "number" % (view,))
            War = ops.aspect_width(W, self.ar)
            if War < 2:
                raise ValueError("aspect-ratio view %r: at frame width %d the view is %d "
                                 "column(s) wide, under 2" % (view, W, War))
            self.x_inv = float(np.float32(1.0 / self.ar))
            W = War
        self.flip_w = W
        self.scale = ops.target_scale(H, W, view[0], view[1])
        self.Hr, self.Wr = ops.resized_hw(H, W, self.scale)
        self.Hp = int(math.ceil(self.Hr / stride) * stride)
        self.Wp = int(math.ceil(self.Wr / stride) * stride)
        self.im_info = torch.tensor([[self.Hp, self.Wp, self.scale]] * F, dtype=torch.float32,
                                    device=device)
        self.im_scale_t = torch.full((F,), self.scale, dtype=torch.float32, device=device)
        self.im_scale_d = torch.full((F,), self.scale, dtype=torch.float64, device=device)
        self.im_hw = torch.tensor([[H, W]] * F, dtype=torch.int32, device=device)

    def rows(self, F):
        """The geometry of a step of F <= batch frames."""
        if F == self.F:
            return self
        g = copy.copy(self)
        g.F = F
        for k in ("im_info", "im_scale_t", "im_scale_d", "im_hw"):
            setattr(g, k, getattr(self, k)[:F])
        return g


def _flip_dets(dets, width):
    """flip_boxes of detections [..., >= 4], float32: x1' = (width - x2) - 1."""
    dets_hf = dets.clone()
    dets_hf[..., 0] = width - dets[..., 2] - 1
    dets_hf[..., 2] = width - dets[..., 0] - 1
    return dets_hf


def view_dets(dets, g):
    """Detections [..., >= 4] as the heads of view g (a _ViewGeom) take them
    (lib/core/test.py:485, 513-518): aspect_ratio(boxes, ar) for an aspect-ratio view
    (float32 x1, x2 times float32(ar)), then flip_boxes with the view's width for a
    flipped one.  In torch, on the detections' device."""
    if g.ar is not None:
        dets_ar = dets.clone()
        dets_ar[..., 0] = g.ar * dets[..., 0]
        dets_ar[..., 2] = g.ar * dets[..., 2]
        dets = dets_ar
    return _flip_dets(dets, g.flip_w) if g.hflip else dets


GIVEN_BOXES_STEP_CAP = 2048  # csrc/detections.hip kDetRMax: RoI rows per frame of a step


class FramePipeline:
    """The step every pipeline here runs (_run): the box pass (_box_pass: body, box
    stages, detections; leaves each head view's geometry and pyramid in out["_pyrs"]),
    the per-detection heads (_roi_heads) over the head views (_view_rois), and
    complete().  A subclass overrides the part it changes."""
    ASYNC = True  # run(sync=False) queues a step with no host read (see run())
    KEYPOINTS = False  # the class runs the MODEL.KEYPOINTS_ON configs
    TEST_AUG = ()  # which of TEST.BBOX_AUG / MASK_AUG / KPS_AUG the class serves
    GIVEN_BOXES = True  # the class runs MODEL.FASTER_RCNN False: run(box_proposals=...)
    mask_heur = None  # one mask view, no combination

    def __init__(self, model, cfg, frame_hw=(800, 1333), batch=1, channels_last=False,
                 det_cap=256, device="cuda"):
        self._setup(model, cfg, batch, channels_last, det_cap, device)
        self.H, self.W = frame_hw
        # the identity view's geometry (the C4 pipeline, which does not pad, overwrites
        # Hp, Wp and im_info)
        g = self.ident = _ViewGeom(self.head_views[0], self.H, self.W, cfg.FPN.COARSEST_STRIDE,
                                   batch, self.device)
        self.im_scale, self.Hr, self.Wr, self.Hp, self.Wp = g.scale, g.Hr, g.Wr, g.Hp, g.Wp
        self.im_info, self.im_scale_t, self.im_scale_d = g.im_info, g.im_scale_t, g.im_scale_d
        self.im_hw = g.im_hw

    def _setup(self, model, cfg, batch, channels_last, det_cap, device):
        """Everything of the constructor that does not depend on the frame size."""
        tst, name = cfg.TEST, type(self).__name__
        if cfg.MODEL.KEYPOINTS_ON and not self.KEYPOINTS:
            raise NotImplementedError(
                "%s: MODEL.KEYPOINTS_ON configs run on KeypointFramePipeline (FPN, frames of "
                "one size); ragged, C4 and VOS keypoint steps are not built" % name)
        if (tst.BBOX_AUG.ENABLED or tst.KPS_AUG.ENABLED) and self.KEYPOINTS \
                and "KPS_AUG" not in self.TEST_AUG:
            raise NotImplementedError(
                "%s: TEST.BBOX_AUG / TEST.KPS_AUG on a keypoint config run on "
                "KeypointAugFramePipeline (FPN, frames of one size)" % name)
        if (tst.BBOX_AUG.ENABLED or tst.MASK_AUG.ENABLED) and not self.TEST_AUG:
            raise NotImplementedError(
                "%s: TEST.BBOX_AUG / TEST.MASK_AUG run on AugFramePipeline (FPN mask configs, "
                "frames of one size) and, for keypoint configs, on KeypointAugFramePipeline; "
                "ragged, C4 and VOS steps with test-time augmentation are not built" % name)
        if tst.KPS_AUG.ENABLED and "KPS_AUG" not in self.TEST_AUG:
            raise NotImplementedError(
                "%s: TEST.KPS_AUG runs on KeypointAugFramePipeline (FPN keypoint configs, "
                "frames of one size)" % name)
        self.given_boxes = not cfg.MODEL.FASTER_RCNN
        if self.given_boxes and not self.GIVEN_BOXES:
            raise NotImplementedError(
                "%s: MODEL.FASTER_RCNN False (detection from the caller's box_proposals, "
                "lib/core/test.py:128-190) runs on FramePipeline and VOSPipeline; ragged, C4, "
                "augmented and keypoint steps with given boxes are not built" % name)
        if self.given_boxes and cfg.get("TRAIN", {}).get("BBOX_NORMALIZE_TARGETS_PRECOMPUTED"):
            raise NotImplementedError(
                "%s: TRAIN.BBOX_NORMALIZE_TARGETS_PRECOMPUTED (lib/core/test.py:174-177) is not "
                "built" % name)
        if not cfg.MODEL.KEYPOINTS_ON and not hasattr(model, "Mask_Head"):
            raise NotImplementedError(
                "%s: the model has no Mask_Head (MODEL.MASK_ON False); a box-only step is "
                "not built" % type(self).__name__)
        self.model = model
        self.cfg = cfg
        self.F = batch
        self.device = torch.device(device)
        self.channels_last = channels_last
        self.det_cap = det_cap
        self._proposals = None  # the step's box_proposals while run() is inside _run
        self._nms_options = nms_options(cfg)
        # the views whose pyramids the heads read: here the identity view alone
        self.head_views = [(tst.SCALE, tst.MAX_SIZE, False)]
        self.lut = torch.from_numpy(ops.pixel_lut(cfg.PIXEL_MEANS)).to(self.device)
        if cfg.FPN.FPN_ON:
            k_min, k_max = cfg.FPN.RPN_MIN_LEVEL, cfg.FPN.RPN_MAX_LEVEL
            self.rpn_levels = list(range(k_min, k_max + 1))
            self.anchors = [] if self.given_boxes else [
                getattr(model, "anchors_fpn%d" % l).to(self.device) for l in self.rpn_levels]
            self.rpn_scales = [1. / 2 ** l for l in self.rpn_levels]
            self.roi_levels = list(range(cfg.FPN.ROI_MIN_LEVEL, cfg.FPN.ROI_MAX_LEVEL + 1))
            self.roi_scales = [1. / 2 ** l for l in self.roi_levels]
        self.timers = None  # enable_timers(): per-stage HIP-event timing
        self._marks = None

    # ------------------------------------------------------------------ #
    # tracing: the reference threads a defaultdict(Timer) through im_detect_all
    # (lib/core/test.py:62-107, utils/timer.py:11-35, wall clock); here each
    # stage boundary records a HIP event on the launch stream, so the stage
    # times are device times and timing never adds a synchronisation.
    def enable_timers(self, on: bool = True):
        self.timers = {} if on else None
        return self

    def _mark(self, name: str):
        if self._marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._marks.append((name, ev))

    def _collect_marks(self):
        marks, self._marks = self._marks, None
        if not marks:
            return
        marks[-1][1].synchronize()
        for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
            t = self.timers.setdefault(name, StageTimer(name))
            t.add(a.elapsed_time(b) / 1e3)

    def timer_summary(self):
        """{stage: average seconds per call} (Timer.average_time of the reference)."""
        return {k: v.average_time for k, v in (self.timers or {}).items()}

    def make_blob(self, frames, g=None):
        """get_image_blob on the device at view geometry g (None: the pipeline's own):
        identity scale -> vd_image_to_blob, else vd_image_resize_to_blob (mean
        subtraction + INTER_LINEAR resize + pad).  An aspect-ratio view takes the
        UNFLIPPED frames: vd_image_aspect_resize_to_blob resizes the width, then flips."""
        nhwc = self.channels_last
        scale, Hp, Wp = (self.im_scale, self.Hp, self.Wp) if g is None else (g.scale, g.Hp, g.Wp)
        if g is not None and g.ar is not None:
            blob = ops.image_aspect_resize_to_blob(frames, self.lut, g.ar, scale, Hp, Wp,
                                                   hflip=g.hflip, nhwc=nhwc)
        elif scale == 1.0:
            blob = ops.image_to_blob(frames, self.lut, Hp, Wp, nhwc=nhwc)
        else:
            blob = ops.image_resize_to_blob(frames, self.lut, scale, Hp, Wp, nhwc=nhwc)
        return blob.permute(0, 3, 1, 2) if nhwc else blob  # NCHW view

    def backbone(self, frames):
        return self.model.Conv_Body(self.make_blob(frames))  # [P6, P5, P4, P3, P2]

    def _frame_rows(self, frames):
        """The geometry a step's frames run at: F, im_info, im_scale_t (fp32), im_scale_d
        (fp64) and im_hw, the per-frame rows the proposal, detection and RoI kernels read."""
        return self.ident.rows(frames.shape[0])

    def nhwc_pyramid(self, feats):
        """P2..P5 as B x H x W x C (a free view when the body ran channels_last)."""
        out = []
        for lvl in self.roi_levels:
            t = feats[len(feats) - 1 - (lvl - self.rpn_levels[0])]
            if t.is_contiguous(memory_format=torch.channels_last):
                out.append(t.permute(0, 2, 3, 1))
            else:
                out.append(ops.nchw_to_nhwc(t))
        return out

    @torch.no_grad()
    def run(self, frames: torch.Tensor, keep_intermediates: bool = False, sync: bool = True,
            box_proposals=None):
        """frames: F x H x W x 3 uint8 BGR on the device.  Returns a dict of device
        tensors: dets [F,cap,5] (x1,y1,x2,y2,score), classes [F,cap], counts [F],
        masks [M,28,28] for the M = sum(counts) detections in (frame, class,
        proposal) order, and counts_host.  sync=False queues the step without
        any host read (graph-capturable): masks then has mask_rows(F) rows of
        which the first M are real, and complete(out) later reads the counts and
        trims.  Stage marks (enable_timers): conv_body, proposals, box_head
        (together the reference's im_detect_bbox), misc_bbox, im_detect_mask.
        box_proposals = (boxes [F,cap,4] fp32 in frame coordinates, counts [F] int32), on
        the device: required with MODEL.FASTER_RCNN False, where the heads run on the
        caller's boxes (im_detect_all(model, im, box_proposals), lib/core/test.py:56-107):
        the RoIs are de-duplicated at cfg.DEDUP_BOXES (ops.rois_from_boxes), the box head
        sees each distinct RoI once, and every given row takes its RoI's scores and
        decoded box (ops.gather_rows) into box_results_with_nms_and_limit.  out["rois"] /
        ["roi_counts"] / ["cls_prob"] / ["bbox_pred"] are then the distinct RoIs and the
        head's outputs on them, out["box_index"] / ["box_inv_index"] the two maps, and
        out["det_rois"] / ["det_cls_prob"] / ["det_bbox_pred"] / ["det_roi_counts"] the
        rows the detections were made from.  ValueError with MODEL.FASTER_RCNN True,
        where the reference ignores them."""
        self._proposals = self._check_box_proposals(box_proposals, frames)
        if self.timers is not None:
            self._marks = []
            self._mark("start")
        try:
            return self._run(frames, keep_intermediates, sync)
        finally:
            self._proposals = None
            if self.timers is not None:
                self._collect_marks()

    def _check_box_proposals(self, box_proposals, frames):
        name = type(self).__name__
        if box_proposals is not None and not self.GIVEN_BOXES:
            raise NotImplementedError(
                "%s.run: box_proposals (detection from given boxes) run on FramePipeline and "
                "VOSPipeline; ragged, C4, augmented and keypoint steps with given boxes are "
                "not built" % name)
        if not self.given_boxes:
            if box_proposals is not None:
                raise ValueError(
                    "%s.run: box_proposals with MODEL.FASTER_RCNN True: the boxes come from "
                    "the RPN and the reference ignores the caller's (lib/core/test.py:128-160); "
                    "build the model and the pipeline with MODEL.FASTER_RCNN False" % name)
            return None
        if box_proposals is None:
            raise ValueError("%s.run: MODEL.FASTER_RCNN False needs box_proposals = (boxes "
                             "[F,cap,4] float32, counts [F] int32) on the device" % name)
        boxes, counts = box_proposals
        F = int(frames.shape[0])
        for t, what, dt in ((boxes, "boxes", torch.float32), (counts, "counts", torch.int32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt:
                raise ValueError("%s.run: box_proposals %s must be a device tensor of %s"
                                 % (name, what, dt))
        if boxes.dim() != 3 or boxes.shape[0] != F or boxes.shape[2] != 4 \
                or tuple(counts.shape) != (F,):
            raise ValueError("%s.run: box_proposals must be ([F,cap,4], [F]) with F = %d, got "
                             "%s and %s" % (name, F, tuple(boxes.shape), tuple(counts.shape)))
        if not 1 <= boxes.shape[1] <= GIVEN_BOXES_STEP_CAP:
            raise ValueError("%s.run: box_proposals hold cap = %d rows per frame, outside 1..%d "
                             "(vd_box_detections' RoI capacity)"
                             % (name, boxes.shape[1], GIVEN_BOXES_STEP_CAP))
        return boxes.contiguous(), counts.contiguous()

    def _run(self, frames: torch.Tensor, keep_intermediates: bool = False, sync: bool = True):
        out = self._box_pass(frames, keep_intermediates)
        self._roi_heads(out, keep_intermediates)
        if sync:
            self.complete(out)
        return out

    def _box_pass(self, frames: torch.Tensor, keep_intermediates: bool = False):
        """im_detect_bbox and box_results_with_nms_and_limit of one step: the body, the
        box stages and the detections.  -> out; out["_pyrs"] holds, per head view, (the
        step's geometry, the NHWC pyramid, fast)."""
        cfg, tst = self.cfg, self.cfg.TEST
        g = self._frame_rows(frames)
        feats = self.backbone(frames)
        self._mark("conv_body")
        if self.given_boxes:
            stages, index, inv_index = self._given_box_stages(feats, g)
        else:
            stages = self._box_stages(feats, g.im_info)
        rois, rcnt, cls_prob, bbox_pred, probs, deltas, pyr, fast, post = stages
        F, K = g.F, cls_prob.shape[1]
        det_in = (rois, cls_prob.view(F, post, K), bbox_pred.view(F, post, 4 * K), rcnt)
        det_scale = g.im_scale_t
        if self.given_boxes:
            # every given row takes its RoI's scores and deltas and the caller's box of
            # that RoI, which the reference decodes from (boxes[index], test.py:139, :178):
            # the detections read the box rows as RoIs at scale 1
            boxes, counts = self._proposals
            det_in = ops.gather_rows(boxes, det_in[1], det_in[2], index, inv_index, counts,
                                     rcnt)
            det_scale = torch.ones((F,), dtype=torch.float32, device=self.device)
        dets, dcls, dcnt = ops.box_detections(
            *det_in, det_scale, g.im_hw, tst.SCORE_THRESH,
            tst.NMS, tst.DETECTIONS_PER_IM, cfg.MODEL.BBOX_REG_WEIGHTS, self.det_cap,
            nms_cross_class=tst.NMS_CROSS_CLASS, num_det_per_class_pre=tst.NUM_DET_PER_CLASS_PRE,
            **self._nms_options)
        self._post_detections(dets, dcls, dcnt)
        self._mark("misc_bbox")
        out = {"dets": dets, "classes": dcls, "counts": dcnt, "rois": rois, "roi_counts": rcnt,
               "cls_prob": cls_prob, "bbox_pred": bbox_pred}
        if self.given_boxes:
            out.update(box_index=index, box_inv_index=inv_index, det_rois=det_in[0],
                       det_cls_prob=det_in[1], det_bbox_pred=det_in[2],
                       det_roi_counts=det_in[3])
        if keep_intermediates:  # for stage-wise parity tests
            out.update(feats=feats, rpn_probs=probs, rpn_deltas=deltas, pyramid=pyr)
        # the pyramid stays referenced only until complete() (the rare overflow batch
        # reads it); complete() drops it so a kept result does not pin ~1.5 GB
        out["_pyrs"] = {self.head_views[0]: (g, pyr, fast)}
        return out

    def _nhwc_heads(self):
        """The heads take the RoI features as NHWC (the body ran channels_last)."""
        return self.channels_last and getattr(self.model.Box_Head, "nhwc_ready", False)

    def _box_stages(self, feats, im_info):
        """im_detect_bbox's stages between the body and the decode, for the frames
        whose blob geometry im_info holds: RPN heads, proposals, collect, box RoIAlign
        and the box head.  -> (rois, roi counts, cls_prob, the per-class bbox_pred,
        RPN probs, RPN deltas, NHWC pyramid, fast, post)."""
        cfg = self.cfg
        # RPN heads on P2..P6 (finest first for the proposal kernel)
        probs, deltas = [], []
        for lvl in self.rpn_levels:
            t = feats[len(feats) - 1 - (lvl - self.rpn_levels[0])]
            p, d = self.model.RPN.level_outputs(t)
            probs.append(p.contiguous())
            deltas.append(d.contiguous())
        tst = cfg.TEST
        lrois, lprobs, lcnt = ops.generate_proposals(
            probs, deltas, self.anchors, self.rpn_scales, im_info,
            tst.RPN_PRE_NMS_TOP_N, tst.RPN_POST_NMS_TOP_N, tst.RPN_NMS_THRESH, tst.RPN_MIN_SIZE)
        post = int(tst.RPN_POST_NMS_TOP_N * cfg.FPN.RPN_COLLECT_SCALE + 0.5)
        rois, rlvl, rcnt = ops.collect_distribute(lrois, lprobs, lcnt, post,
                                                  cfg.FPN.ROI_MIN_LEVEL, cfg.FPN.ROI_MAX_LEVEL)
        self._mark("proposals")
        pyr, fast, cls_prob, bbox_pred = self._box_head(feats, rois.view(-1, 5), rlvl.view(-1))
        return rois, rcnt, cls_prob, bbox_pred, probs, deltas, pyr, fast, post

    def _box_head(self, feats, flat_rois, flat_lvl):
        """Box RoIAlign over the NHWC pyramid and the box head on flat_rois [R,5] at
        levels flat_lvl (level - ROI_MIN_LEVEL) -> (pyramid, fast, cls_prob, the per-class
        bbox_pred)."""
        pyr = self.nhwc_pyramid(feats)
        fr = self.cfg.FAST_RCNN
        fast = self._nhwc_heads()
        box_feat = ops.roi_align_fpn(pyr, self.roi_scales, flat_rois, flat_lvl,
                                     fr.ROI_XFORM_RESOLUTION, fr.ROI_XFORM_SAMPLING_RATIO,
                                     roi_order=ops.xcd_roi_order(flat_rois, flat_lvl),
                                     out_layout="nhwc" if fast else "nchw")
        x = self.model.Box_Head.mlp_nhwc(box_feat) if fast else self.model.Box_Head.mlp(box_feat)
        cls_prob, bbox_pred = self.model.Box_Outs(x)
        self._mark("box_head")
        bbox_pred = self.model.Box_Outs.per_class_deltas(bbox_pred, cls_prob.shape[1])
        return pyr, fast, cls_prob, bbox_pred

    def _given_box_stages(self, feats, g):
        """_box_stages with MODEL.FASTER_RCNN False (lib/core/test.py:128-154): no RPN
        heads, proposals or collect; the step's box_proposals become the distinct RoIs of
        every frame in one call (_get_rois_blob + DEDUP_BOXES, ops.rois_from_boxes), which
        get their FPN levels (_add_multilevel_rois_for_test) and go through the box head.
        -> (_box_stages' tuple, index, inv_index); the RoI counts are the numbers of distinct
        RoIs.  Rows past them are zero boxes on frame 0 whose outputs nothing reads."""
        cfg, fpn = self.cfg, self.cfg.FPN
        boxes, counts = self._proposals
        rois, ucnt, index, inv_index = ops.rois_from_boxes(
            boxes, counts, g.im_scale_d, cfg.get("DEDUP_BOXES", 1 / 16.))
        flat_rois = rois.view(-1, 5)
        flat_lvl = ops.map_rois_to_fpn_levels(flat_rois, fpn.ROI_MIN_LEVEL, fpn.ROI_MAX_LEVEL,
                                              canonical_scale=fpn.ROI_CANONICAL_SCALE,
                                              canonical_level=fpn.ROI_CANONICAL_LEVEL)
        flat_lvl.sub_(fpn.ROI_MIN_LEVEL)  # the index into the RoI levels roi_align_fpn takes
        self._mark("proposals")
        pyr, fast, cls_prob, bbox_pred = self._box_head(feats, flat_rois, flat_lvl)
        return (rois, ucnt, cls_prob, bbox_pred, [], [], pyr, fast, boxes.shape[1]), index, \
            inv_index

    def _post_detections(self, dets, classes, counts):
        """Hook after box_results_with_nms_and_limit's device steps (the VOS loop
        adds its previous-frame filter)."""

    def mask_rows(self, F: int) -> int:
        """Rows of the step's mask batch: F x DETECTIONS_PER_IM, a multiple of 64
        (a handful of stable shapes for the convolution algorithm search)."""
        return -(-F * int(self.cfg.TEST.DETECTIONS_PER_IM) // 64) * 64

    def _hflip_dets(self, dets):
        """flip_boxes of the detections, float32: x1' = (W - x2) - 1."""
        return _flip_dets(dets, self.W)

    def _view_rois(self, out, src, rows, row0=0):
        """Rows [row0, row0 + rows) of the RoI batch of src's detections (dets, classes,
        counts), once per head view: yields (view, (RoIs at the view's scale, levels,
        classes, device total), pyramid, fast).  The batch is F x DETECTIONS_PER_IM rows
        built on the device from the device counts -- no host read inside the step; a
        flipped or aspect-ratio view takes flip_boxes / aspect_ratio of the detections,
        made once per distinct (ar, hflip)."""
        cfg = self.cfg
        dets, dcls, dcnt = src["dets"], src["classes"], src["counts"]
        made = {(None, False): dets}
        for v in self.head_views:
            g, pyr, fast = out["_pyrs"][v]
            key = (v[3] if len(v) > 3 else None, bool(v[2]))
            if key not in made:
                made[key] = view_dets(dets, g) if key[0] is not None \
                    else self._hflip_dets(dets)
            yield v, ops.mask_rois(made[key], dcls, dcnt, g.im_scale_d, rows,
                                   cfg.FPN.ROI_MIN_LEVEL, cfg.FPN.ROI_MAX_LEVEL, row0=row0), \
                pyr, fast

    @staticmethod
    def _keep_view_rows(views, v, row0, **rows):
        """keep_intermediates: a head view's per-row tensors into out["views"][v],
        appended to the rows already there when complete() runs rows past the batch."""
        if views is not None:
            vd = views.setdefault(v, {})
            for k, t in rows.items():
                vd[k] = torch.cat([vd[k], t]) if row0 and k in vd else t

    def _roi_head(self, pyr, rois, lvl, fast, head, rc, nhwc_fn, nchw_fn):
        """RoIAlign at rc's resolution (cfg.MRCNN / cfg.KRCNN) in the layout `head` takes,
        then the head: -> (nhwc_fn or nchw_fn of the RoI features, the features as NCHW)."""
        if fast and getattr(head, "nhwc_ready", False):
            feat = ops.roi_align_fpn(pyr, self.roi_scales, rois, lvl, rc.ROI_XFORM_RESOLUTION,
                                     rc.ROI_XFORM_SAMPLING_RATIO, out_layout="nhwc")
            return nhwc_fn(feat), feat.permute(0, 3, 1, 2)
        feat = ops.roi_align_fpn(pyr, self.roi_scales, rois, lvl, rc.ROI_XFORM_RESOLUTION,
                                 rc.ROI_XFORM_SAMPLING_RATIO)
        return nchw_fn(feat), feat

    def _mask_batch(self, pyr, mrois, mlvl, mcls, fast):
        """Mask RoIAlign + mask head + class-selected masks for a padded batch
        (padding rows are zero boxes whose outputs are never read)."""
        head, outs = self.model.Mask_Head, self.model.Mask_Outs
        return self._roi_head(pyr, mrois, mlvl, fast, head, self.cfg.MRCNN,
                              lambda x: head.masks_nhwc(x, outs, mcls),
                              lambda x: outs.selected(head.head(x), mcls))

    def _masks(self, out, rows, row0=0):
        """im_detect_mask, or im_detect_mask_aug, for rows [row0, row0 + rows) of the mask
        batch: every head view's masks, combined by mask_heur where the class has one.
        -> (masks, the identity view's mask_rois and mask_feat, the device total)."""
        views, heur = out.get("views"), self.mask_heur
        acc = first = None
        for i, (v, (mrois, mlvl, mcls, mtotal), pyr, fast) in enumerate(
                self._view_rois(out, out, rows, row0)):
            masks, mfeat = self._mask_batch(pyr, mrois, mlvl, mcls, fast)
            if i == 0:
                first = (mrois, mfeat, mtotal)
            if heur is None:
                acc = masks
            else:
                masks = masks.contiguous()
                if i == 0:
                    acc = torch.empty_like(masks)
                ops.mask_aug_accumulate(acc, masks, v[2], heur, first=i == 0)
            self._keep_view_rows(views, v, row0, mask_rois=mrois, masks=masks)
        if heur is not None:
            ops.mask_aug_finish(acc, len(self.head_views), heur)
        return (acc,) + first

    def _roi_heads(self, out, keep_intermediates):
        """The per-detection heads after misc_bbox: here im_detect_mask
        (box_results_with_nms_and_limit keeps <= DETECTIONS_PER_IM per frame barring
        exact score ties at the limit; complete() runs the rest)."""
        out["masks"], out["mask_rois"], out["mask_feat"], out["mask_total"] = \
            self._masks(out, self.mask_rows(out["dets"].shape[0]))
        self._mark("im_detect_mask")

    def _raise_on_failed_counts(self, counts):
        ops.raise_on_failed_counts(counts)

    def _check_counts(self, counts):
        """complete()'s checks of the host counts: a failed frame, more than det_cap."""
        self._raise_on_failed_counts(counts)
        if max(counts, default=0) > self.det_cap:
            raise RuntimeError("detections exceed det_cap=%d: %s" % (self.det_cap, counts))

    @staticmethod
    def _finish_rows(out, keys, M):
        """complete()'s end: the kept pyramids dropped, out[keys] and the head views'
        per-row intermediates trimmed to the M real rows."""
        out.pop("_pyrs", None)
        for k in keys:
            out[k] = out[k][:M]
        for vd in out.get("views", {}).values():
            for k in ("mask_rois", "masks", "kps_rois", "kps_heatmaps", "kps_feat"):
                if k in vd:
                    vd[k] = vd[k][:M]

    def complete(self, out: dict) -> dict:
        """The step's one host read, after everything is queued: the detection
        counts (failure / capacity checks), the masks of detections beyond the
        padded batch (exact score ties at DETECTIONS_PER_IM), through every head view
        again, and the outputs trimmed to the M = sum(counts) real detections.
        Idempotent."""
        if "counts_host" in out:
            return out
        if "box_inv_index" in out:  # given boxes: a frame whose count exceeded cap
            over = [f for f, c in enumerate(out["roi_counts"].cpu().tolist()) if c < 0]
            if over:
                raise ops._lib.VosdetError("box_proposals: the counts of frame(s) %s exceed the "
                                       "cap of %d rows per frame (or are negative)"
                                       % (over, out["box_inv_index"].shape[1]))
        counts = out["counts"].cpu().tolist()
        self._check_counts(counts)
        keys = ("masks", "mask_rois", "mask_feat")
        M, cap = sum(counts), out["masks"].shape[0]
        if M > cap:  # rows [cap, M): a second, rare batch
            more = self._masks(out, -(-(M - cap) // 64) * 64, cap)
            for k, t in zip(keys, more):
                out[k] = torch.cat([out[k], t])
        self._finish_rows(out, keys, M)
        out["counts_host"] = counts
        return out


class KeypointFramePipeline(FramePipeline):
    """FramePipeline for the Keypoint R-CNN configs (FPN): after misc_bbox the step runs
    im_detect_keypoints (lib/core/test.py:529-564) and keypoint_results (:858-874)
    instead of the mask stage, all on the device:

      vd_mask_rois (the keypoint RoI batch: same rows and order as the mask batch)
      --> vd_roi_align_fpn KRCNN.ROI_XFORM_RESOLUTION --> Keypoint_Head (MFMA 3x3
      convs) --> Keypoint_Outs (deconv + bilinear upsample, 56x56 logits)
      --> vd_heatmaps_to_keypoints against the detection boxes as stored in dets.

    out["keyps"] [M,4,K] rows (x, y, logit, prob) for the M = sum(counts)
    detections in (frame, class, proposal) order; with keep_intermediates also
    kps_heatmaps [M,K,S,S], kps_feat [M,C,P,P] and kps_boxes [M,4].  Stage marks:
    im_detect_keypoints, misc_keypoints.

    nms_oks (None / False: off, every output as above; True: the reference's 0.3; a
    float: that threshold) appends keypoint_results' OKS NMS (test.py:864-870) to the
    step as ops.nms_oks_frames, with no host read.  It needs MODEL.NUM_CLASSES == 2:
    the kept indices address cls_boxes[person], which is the frame's detections only
    when person is the only class.  out["dets"], ["classes"], ["counts"] and ["keyps"]
    are then the post-NMS rows in kept order (descending mean logit), as the reference
    returns cls_boxes / cls_keyps; out["oks_keep"] [F,cap] holds the frame-local
    pre-NMS indices (-1 past the count).  kps_rois, kps_heatmaps, kps_feat and
    kps_boxes stay in pre-NMS row order; keep_intermediates adds dets_pre_oks,
    classes_pre_oks, counts_pre_oks and keyps_pre_oks.  Stage mark: misc_oks_nms."""
    KEYPOINTS = True
    GIVEN_BOXES = False
    BOXES_FIRST = True  # _keypoints: the decode's boxes are queued ahead of the head

    def __init__(self, model, cfg, frame_hw=(800, 1333), batch=1, channels_last=False,
                 det_cap=256, device="cuda", nms_oks=None):
        if not cfg.MODEL.KEYPOINTS_ON:
            raise ValueError("KeypointFramePipeline needs a MODEL.KEYPOINTS_ON config")
        if not cfg.FPN.FPN_ON or bool(cfg.get("VOS", False)):
            raise NotImplementedError("KeypointFramePipeline: FPN configs only (no C4 / VOS)")
        self.oks_thresh = None
        if nms_oks is not None and nms_oks is not False:
            if int(cfg.MODEL.NUM_CLASSES) != 2:
                raise ValueError(
                    "KeypointFramePipeline(nms_oks=%r) needs MODEL.NUM_CLASSES == 2 (person "
                    "only), got %d: nms_oks' indices address cls_boxes[person]"
                    % (nms_oks, int(cfg.MODEL.NUM_CLASSES)))
            if det_cap > ops.OKS_MAX_D:
                raise ValueError("KeypointFramePipeline(nms_oks=%r): det_cap = %d exceeds "
                                 "OKS NMS's %d rows per frame" % (nms_oks, det_cap,
                                                                  ops.OKS_MAX_D))
            self.oks_thresh = 0.3 if nms_oks is True else float(nms_oks)  # test.py:866
        super().__init__(model, cfg, frame_hw, batch, channels_last, det_cap, device)
        self._ones_d = torch.ones((batch,), dtype=torch.float64, device=self.device)

    def _keypoint_heatmaps(self, pyr, krois, klvl, fast):
        """im_detect_keypoints of a padded batch: RoIAlign + head + outputs -> (the
        [rows,K,S,S] logits, the RoI features as NCHW)."""
        head = self.model.Keypoint_Head
        x, kfeat = self._roi_head(pyr, krois, klvl, fast, head, self.cfg.KRCNN,
                                  head.head_nhwc, head.head)
        return self.model.Keypoint_Outs(x).contiguous(), kfeat

    def _stored_boxes(self, src, rows, row0):
        """Rows [row0, row0 + rows) of src's dets unscaled, the boxes the decode runs
        against: vd_mask_rois at scale 1 copies the stored boxes bit for bit (a float32
        times 1.0 in float64), in the batch's row order, zeros past the total."""
        cfg, dets = self.cfg, src["dets"]
        return ops.mask_rois(dets, src["classes"], src["counts"], self._ones_d[:dets.shape[0]],
                             rows, cfg.FPN.ROI_MIN_LEVEL, cfg.FPN.ROI_MAX_LEVEL,
                             row0=row0)[0][:, 1:5]

    def _decode(self, heats, kboxes, want_combined):
        """keypoint_results' decode of the head views' heatmaps (here one view's) ->
        (keyps, the maps that were decoded when want_combined)."""
        keyps = ops.heatmaps_to_keypoints(heats[0], kboxes, self.cfg.KRCNN.INFERENCE_MIN_SIZE)
        return keyps, heats[0] if want_combined else None

    def _keypoints(self, out, src, rows, row0=0):
        """im_detect_keypoints, or im_detect_keypoints_aug, + keypoint_results' decode for
        rows [row0, row0 + rows) of the keypoint batch of src's detections (padding rows
        are zero boxes: a 1 x 1 resized map, never read): every head view's heatmaps,
        then _decode.  -> (keyps, the kps_* tensors of those rows -- rois and features of
        the identity view, the decoded heatmaps when the step keeps its intermediates
        -- and the device total).  out["views"], where the step keeps it, is given each
        view's kps_rois, kps_heatmaps and kps_feat."""
        keep, views = out["_kps_keep"], out.get("views")
        # the plain step queues the decode's boxes ahead of the head, the augmented one
        # behind its views
        kboxes = self._stored_boxes(src, rows, row0) if self.BOXES_FIRST else None
        heats, first = [], None
        for v, (krois, klvl, _, ktotal), pyr, fast in self._view_rois(out, src, rows, row0):
            heat, kfeat = self._keypoint_heatmaps(pyr, krois, klvl, fast)
            heats.append(heat)
            if first is None:
                first = (krois, kfeat, ktotal)
            self._keep_view_rows(views, v, row0, kps_rois=krois, kps_heatmaps=heat,
                                 kps_feat=kfeat)
        if kboxes is None:
            kboxes = self._stored_boxes(src, rows, row0)
        self._mark("im_detect_keypoints")
        keyps, comb = self._decode(heats, kboxes, keep)
        self._mark("misc_keypoints")
        more = {"kps_rois": first[0], "kps_feat": first[1], "kps_boxes": kboxes}
        if comb is not None:
            more["kps_heatmaps"] = comb
        return keyps, more, first[2]

    def _oks_nms(self, out, pre, keyps):
        """keypoint_results' OKS NMS of the pre-NMS rows `pre` (dets, classes, counts)
        with their raw keypoints: out's detections and keypoints become the kept rows."""
        res = ops.nms_oks_frames(keyps, pre["dets"], pre["classes"], pre["counts"],
                                 self.oks_thresh)
        out.update(dets=res.dets, classes=res.classes, counts=res.counts, keyps=res.keyps,
                   oks_keep=res.keep)

    def _roi_heads(self, out, keep_intermediates):
        """The keypoint heads and, with nms_oks, the step's OKS NMS of the detections
        and their raw keypoints."""
        out["_kps_keep"] = keep_intermediates
        keyps, more, out["kps_total"] = self._keypoints(
            out, out, self.mask_rows(out["dets"].shape[0]))
        out["keyps"], out["kps_rois"] = keyps, more["kps_rois"]
        if keep_intermediates:
            out.update(more)
        if self.oks_thresh is not None:
            pre = {k: out[k] for k in ("dets", "classes", "counts", "keyps")}
            out["_oks_pre"] = pre
            if keep_intermediates:
                out.update({k + "_pre_oks": v for k, v in pre.items()})
            self._oks_nms(out, pre, keyps)
            self._mark("misc_oks_nms")

    def complete(self, out: dict) -> dict:
        """FramePipeline.complete for the keypoint outputs: the one host read, the
        rare rows past the padded batch, and the trim to the M real detections.  With
        nms_oks the read brings the pre- and post-NMS counts together: keyps, dets and
        classes follow the post-NMS counts (counts_host), the kps_* tensors and the
        *_pre_oks intermediates the pre-NMS ones (counts_pre_oks_host).  The overflow
        batch then decodes the remaining rows and runs the NMS again on the full set,
        replacing the step's result."""
        if "counts_host" in out:
            return out
        pre = out.pop("_oks_pre", None)
        if pre is None:
            counts = before = out["counts"].cpu().tolist()
        else:
            F = out["counts"].numel()
            both = torch.cat([pre["counts"], out["counts"]]).cpu().tolist()
            before, counts = both[:F], both[F:]
        self._check_counts(before)
        keep = out["_kps_keep"]
        keys = ["kps_rois"] + (["kps_heatmaps", "kps_feat", "kps_boxes"] if keep else [])
        raw = out["keyps"] if pre is None else pre["keyps"]  # one row per detection
        M, cap = sum(before), raw.shape[0]
        if M > cap:  # rows [cap, M): a second, rare batch
            k2, more, _ = self._keypoints(out, pre or out, -(-(M - cap) // 64) * 64, cap)
            for k in keys:
                out[k] = torch.cat([out[k], more[k]])
            raw = torch.cat([raw, k2])
            if pre is not None:
                self._oks_nms(out, pre, raw)
                counts = out["counts"].cpu().tolist()
        del out["_kps_keep"]
        self._finish_rows(out, keys, M)
        if pre is None:
            out["keyps"] = raw[:M]
        else:
            out["keyps"] = out["keyps"][:sum(counts)]
            out["counts_pre_oks_host"] = before
            if keep:
                out["keyps_pre_oks"] = raw[:M]
        out["counts_host"] = counts
        return out


def frame_keypoints(pipe: "KeypointFramePipeline", out: dict, num_classes: int = None):
    """keypoint_results (lib/core/test.py:858-874) for every frame of a completed
    KeypointFramePipeline output: a list over frames of cls_keyps -- num_classes lists,
    empty but for the person class's, which holds the frame's [4, K] float32 arrays
    (x, y, logit, prob) in detection order (with nms_oks: the kept rows, grouped by
    the post-NMS counts)."""
    from . import keypoints
    K = int(num_classes or pipe.cfg.MODEL.NUM_CLASSES)
    pipe.complete(out)
    person = keypoints.get_person_class_index()
    kps = out["keyps"].cpu().numpy()
    res, start = [], 0
    for k in (int(c) for c in out["counts_host"]):
        cls_keyps = [[] for _ in range(K)]
        cls_keyps[person] = [kps[i] for i in range(start, start + k)]
        res.append(cls_keyps)
        start += k
    return res


class _AugViews:
    """What the test-time-augmentation pipelines share, mixed in ahead of the plain
    class: the view table with its budgets, and a box pass that runs im_detect_bbox_aug
    over the box views (box_union) and the bodies of the remaining head views."""

    def _setup_views(self, box_views, head_views, cand_cap, pyramid_budget_bytes, kind, key):
        """geom[view] for every distinct view, the union's capacity, and the budget of
        the pyramids kept for the heads (kind, key: the head views' name in its error)."""
        cfg, batch = self.cfg, self.F
        self.box_views, self.head_views = box_views, head_views
        self.geom = {self.ident.view: self.ident}
        for v in box_views + head_views:
            if v not in self.geom:
                self.geom[v] = _ViewGeom(v, self.H, self.W, cfg.FPN.COARSEST_STRIDE, batch,
                                         self.device)
        self._unions = {}
        post = int(cfg.TEST.RPN_POST_NMS_TOP_N * cfg.FPN.RPN_COLLECT_SCALE + 0.5)
        self.cand_cap = int(cand_cap or min(ops.UNION_MAX_CAND, len(box_views) * post))
        kept = sum(self.pyramid_bytes(self.geom[v]) for v in set(head_views))
        if batch * kept > pyramid_budget_bytes:
            raise ValueError(
                "%s: the %d %s views' pyramids take %d x %d bytes, over pyramid_budget_bytes "
                "= %d (fewer frames per step, or fewer %s views)"
                % (type(self).__name__, len(set(head_views)), kind, batch, kept,
                   pyramid_budget_bytes, key))

    def pyramid_bytes(self, g) -> int:
        """Bytes of one frame's RoI pyramid (P2..P5, FPN.DIM channels, fp32) at view g."""
        n = 0
        for lvl in self.roi_levels:
            n += -(-g.Hp // 2 ** lvl) * -(-g.Wp // 2 ** lvl)
        return n * int(self.cfg.FPN.DIM) * 4

    def _union(self, F, K):
        if (F, K) not in self._unions:
            self._unions[(F, K)] = ops.BoxUnion(self.cand_cap, F, K, self.device)
        return self._unions[(F, K)]

    def _view_body(self, frames, flipped, g):
        """View g's blob, of the frames or their horizontal flip, and its body (an
        aspect-ratio view's flip is an argument of its blob kernel)."""
        blob = self.make_blob(flipped if g.hflip and g.ar is None else frames, g)
        return blob, self.model.Conv_Body(blob)

    def _box_pass(self, frames, keep_intermediates=False):
        """The box pass over the box views (box_union) or the plain one, then the bodies
        of the head views it did not run (the reference's im_conv_body_only).  A head
        view keeps its pyramid for the head pass; keep_intermediates adds out["views"]."""
        F = frames.shape[0]
        flipped = frames.flip(2) if any(v[2] and len(v) == 3 for v in self.geom) else None
        views = {}
        if self.box_union:
            out = self._union_pass(frames, flipped, views, keep_intermediates)
        else:
            out = super()._box_pass(frames, keep_intermediates)
        pyrs = out["_pyrs"]
        for v in self.head_views:
            if v not in pyrs:
                g = self.geom[v].rows(F)
                blob, feats = self._view_body(frames, flipped, g)
                pyrs[v] = (g, self.nhwc_pyramid(feats), self._nhwc_heads())
                self._mark("conv_body")
                if keep_intermediates:
                    views.setdefault(v, {}).update(pyramid=pyrs[v][1], blob=blob)
        if keep_intermediates:
            out["views"] = views
        return out

    def _union_pass(self, frames, flipped, views, keep_intermediates):
        """im_detect_bbox_aug + box_results_with_nms_and_limit: every box view's body and
        box stages folded into the union, then the detections."""
        cfg, tst = self.cfg, self.cfg.TEST
        F = frames.shape[0]
        pyrs, union = {}, None
        for i, v in enumerate(self.box_views):
            g = self.geom[v].rows(F)
            blob, feats = self._view_body(frames, flipped, g)
            self._mark("conv_body")
            rois, rcnt, cls_prob, bbox_pred, _, _, pyr, fast, post = \
                self._box_stages(feats, g.im_info)
            K = cls_prob.shape[1]
            union = union or self._union(F, K)
            union.add_view(rois, cls_prob.view(F, post, K), bbox_pred.view(F, post, 4 * K), rcnt,
                           g.im_scale_t, g.im_hw, g.hflip, tst.SCORE_THRESH,
                           cfg.MODEL.BBOX_REG_WEIGHTS, first=i == 0, x_inv=g.x_inv)
            self._mark("union_add_view")
            if v in self.head_views:
                pyrs[v] = (g, pyr, fast)
            if keep_intermediates:
                views[v] = dict(rois=rois, roi_counts=rcnt, cls_prob=cls_prob,
                                bbox_pred=bbox_pred, pyramid=pyr, blob=blob)
        cand = torch.zeros((F, K), dtype=torch.int32, device=self.device)
        dets, dcls, dcnt = union.detections(
            tst.NMS, tst.DETECTIONS_PER_IM, self.det_cap, nms_cross_class=tst.NMS_CROSS_CLASS,
            num_det_per_class_pre=tst.NUM_DET_PER_CLASS_PRE, cand_counts=cand,
            **self._nms_options)
        self._mark("misc_bbox")
        # the identity view is the last box view: its rows are the step's
        return {"dets": dets, "classes": dcls, "counts": dcnt, "cand_counts": cand,
                "rois": rois, "roi_counts": rcnt, "cls_prob": cls_prob, "bbox_pred": bbox_pred,
                "_pyrs": pyrs}

    def _raise_on_failed_union(self, counts):
        if any(c < 0 for c in counts):
            bad = [i for i, c in enumerate(counts) if c < 0]
            raise ops._lib.VosdetError(
                "test-time augmentation failed for frame(s) %s (count -1): a class's union of "
                "the box views holds more than cand_cap = %d candidates, or a view's proposal "
                "selection failed" % (bad, self.cand_cap))


class AugFramePipeline(_AugViews, FramePipeline):
    """FramePipeline with the reference's test-time augmentation (TEST.BBOX_AUG /
    TEST.MASK_AUG, lib/core/test.py:193-363, 405-526) for the FPN mask configs and
    frames of one size; cfg comes from config.load_cfg(..., test_aug=True).

      per distinct view (config.aug_views: scale, max_size, hflip[, ar]), on the frames
      or their horizontal flip (an aspect-ratio view: vd_image_aspect_resize_to_blob on
      the frames, its boxes mapped back by x_inv in the union and its heads' detections
      by aspect_ratio): blob at the view's geometry --> body --> [box views: RPN,
      proposals, collect, box RoIAlign, box head --> vd_box_union_add_view in np.vstack
      order, the identity view last]
      --> vd_box_union_detections (UNION heuristics: one box_results_with_nms_and_limit
      over every view's rows) --> vd_detections_postfilter
      --> per mask view, the identity view first: the final detections (flip_boxes for a
      flipped view) --> vd_mask_rois at the view's scale --> mask RoIAlign + mask head on
      the view's pyramid --> vd_mask_aug_accumulate --> vd_mask_aug_finish.

    The reference runs the body again for every mask view; here a view's pyramid is kept
    from the box pass to the mask pass (pyramid_budget_bytes bounds batch x the kept
    pyramids).  cand_cap: rows of a class's candidate list per image (default min(16384,
    box views x post_nms_topN)); an image whose list overflows fails at complete().
    The result dict is FramePipeline's: masks are the combined masks, mask_rois /
    mask_feat the identity view's.  keep_intermediates adds out["views"]: per distinct
    view a dict with rois, roi_counts, cls_prob, bbox_pred, pyramid and blob (box views)
    and mask_rois, masks (mask views), and out["cand_counts"] [F,K]."""

    TEST_AUG = ("BBOX_AUG", "MASK_AUG")
    GIVEN_BOXES = False
    box_union = True  # one box view too goes through the union

    def __init__(self, model, cfg, frame_hw=(800, 1333), batch=1, channels_last=False,
                 det_cap=256, device="cuda", cand_cap=None, pyramid_budget_bytes=24 << 30):
        from . import config as vcfg
        if not cfg.FPN.FPN_ON or bool(cfg.get("VOS", False)) or cfg.MODEL.KEYPOINTS_ON:
            raise NotImplementedError(
                "AugFramePipeline: FPN mask configs only (test-time augmentation on the C4, "
                "VOS and keypoint pipelines is not built; keypoint configs run on "
                "KeypointAugFramePipeline)")
        vcfg.check_supported(cfg, test_aug=True, aspect_views=True)
        vcfg.check_aspect_ratios(cfg, frame_hw[1])
        super().__init__(model, cfg, frame_hw, batch, channels_last, det_cap, device)
        box_views, self.mask_views = vcfg.aug_views(cfg)
        self.mask_heur = cfg.TEST.MASK_AUG.HEUR if cfg.TEST.MASK_AUG.ENABLED else "SOFT_AVG"
        self._setup_views(box_views, self.mask_views, cand_cap, pyramid_budget_bytes,
                          "mask", "MASK_AUG")

    def _raise_on_failed_counts(self, counts):
        self._raise_on_failed_union(counts)


class KeypointAugFramePipeline(_AugViews, KeypointFramePipeline):
    """KeypointFramePipeline with the reference's test-time augmentation (TEST.BBOX_AUG
    and TEST.KPS_AUG, lib/core/test.py:193-363, 567-730) for the FPN keypoint configs
    and frames of one size; cfg comes from config.load_cfg(..., test_aug=True).

      box pass: with BBOX_AUG AugFramePipeline's (every box view into the union, then
      the detections), without it KeypointFramePipeline's single identity view
      --> per keypoint view (config.kps_aug_views, the identity view first): the
      detections (flip_boxes for a flipped view) --> vd_mask_rois at the view's scale
      --> keypoint RoIAlign + Keypoint_Head + Keypoint_Outs on the view's pyramid (kept
      from the box pass when the view is a box view too, otherwise the body runs as
      im_conv_body_only does)
      --> vd_heatmaps_to_keypoints_aug: the views' heatmaps combined (flip_heatmaps of
      the flipped views, HM_AVG / HM_MAX, with SCALE_SIZE_DEP the views chosen per box
      by its area against AREA_TH) and decoded against the stored detection boxes in
      one launch --> the optional OKS NMS (nms_oks).

    All V views' heatmaps are alive at the decode: heatmap_budget_bytes bounds V x the
    padded batch's rows x K x S x S x 4 bytes, pyramid_budget_bytes batch x the kept
    pyramids.  The result dict is KeypointFramePipeline's.  keep_intermediates adds
    out["views"][view] with kps_rois, kps_heatmaps (as the network returned them, not
    inverted) and kps_feat (and the box views' tensors as AugFramePipeline's),
    out["kps_heatmaps"] = the combined maps, out["kps_boxes"]; kps_rois / kps_feat are
    the identity view's.  Stage marks: conv_body, union_add_view, misc_bbox,
    im_detect_keypoints, misc_keypoints, misc_oks_nms."""

    TEST_AUG = ("BBOX_AUG", "KPS_AUG")
    GIVEN_BOXES = False
    BOXES_FIRST = False

    def __init__(self, model, cfg, frame_hw=(800, 1333), batch=1, channels_last=False,
                 det_cap=256, device="cuda", nms_oks=None, cand_cap=None,
                 pyramid_budget_bytes=24 << 30, heatmap_budget_bytes=8 << 30):
        from . import config as vcfg
        vcfg.check_supported(cfg, test_aug=True, aspect_views=True)
        vcfg.check_aspect_ratios(cfg, frame_hw[1])
        super().__init__(model, cfg, frame_hw, batch, channels_last, det_cap, device, nms_oks)
        tst = cfg.TEST
        self.bbox_aug = self.box_union = bool(tst.BBOX_AUG.ENABLED)
        self.kps_views, self.kps_ds, self.kps_us = vcfg.kps_aug_views(cfg)
        if len(set(self.kps_views)) != len(self.kps_views):
            raise ValueError("KeypointAugFramePipeline: TEST.KPS_AUG lists a view twice: %s"
                             % (self.kps_views,))
        if len(self.kps_views) > ops.KPS_AUG_MAX_VIEWS:
            raise ValueError("KeypointAugFramePipeline: %d keypoint views, the combination "
                             "takes %d" % (len(self.kps_views), ops.KPS_AUG_MAX_VIEWS))
        self.kps_heur = tst.KPS_AUG.HEUR if tst.KPS_AUG.ENABLED else "HM_AVG"
        self.kps_area_th = float(tst.KPS_AUG.AREA_TH) \
            if tst.KPS_AUG.ENABLED and tst.KPS_AUG.SCALE_SIZE_DEP else None
        self._setup_views(vcfg.aug_views(cfg)[0], self.kps_views, cand_cap,
                          pyramid_budget_bytes, "keypoint", "KPS_AUG")
        V, rows = len(self.kps_views), self.mask_rows(batch)
        K, S = int(cfg.KRCNN.NUM_KEYPOINTS), int(cfg.KRCNN.HEATMAP_SIZE)
        if V * rows * K * S * S * 4 > heatmap_budget_bytes:
            raise ValueError(
                "KeypointAugFramePipeline: the views' heatmaps take %d views x %d rows x "
                "(%d x %d x %d x 4 = %d) bytes = %d, over heatmap_budget_bytes = %d (fewer "
                "frames per step, or fewer KPS_AUG views)"
                % (V, rows, K, S, S, K * S * S * 4, V * rows * K * S * S * 4,
                   heatmap_budget_bytes))

    def _decode(self, heats, kboxes, want_combined):
        """One launch combines the views' heatmaps and decodes them (also with one view)."""
        res = ops.heatmaps_to_keypoints_aug(
            heats, [self.geom[v].hflip for v in self.kps_views], self.kps_ds, self.kps_us,
            kboxes, self.cfg.KRCNN.INFERENCE_MIN_SIZE, self.kps_heur, self.kps_area_th,
            want_combined=want_combined)
        return res if want_combined else (res, None)

    def _raise_on_failed_counts(self, counts):
        if self.bbox_aug:
            self._raise_on_failed_union(counts)
        ops.raise_on_failed_counts(counts)


class RaggedBatch:
    """One step's inputs of a RaggedFramePipeline at fixed device addresses: the
    frames packed back to back in `packed` (u8, `capacity` bytes) and, per frame,
    the VdFrameGeom row (`geom`), `im_info` = (Hp_f, Wp_f, s_f), `im_scale_t`
    (fp32), `im_scale_d` (fp64) and `im_hw` = (H_f, W_f).  The per-frame rows are
    views of one device buffer mirrored by one pinned host buffer, so load() is
    a host fill and two H2D copies on the current stream, with no allocation:
    a hipGraph captured on this batch replays with whatever load() put there."""

    def __init__(self, F: int, capacity: int, blob_hw, cfg, device):
        self.F, self.capacity = int(F), int(capacity)
        self.Hb, self.Wb = blob_hw
        self.cfg = cfg
        self.device = torch.device(device)
        self.sizes = None  # [(H, W)] of the loaded frames
        g = ops.GEOM_DTYPE.itemsize
        # layout of the row buffer: 8-byte fields first
        fields = [("geom", torch.uint8, g * F, (F * g,)), ("im_scale_d", torch.float64, 8 * F, (F,)),
                  ("im_info", torch.float32, 12 * F, (F, 3)),
                  ("im_scale_t", torch.float32, 4 * F, (F,)),
                  ("im_hw", torch.int32, 8 * F, (F, 2))]
        total = sum(n for _, _, n, _ in fields)
        self._rows = torch.zeros((total,), dtype=torch.uint8, device=self.device)
        self._h_rows = torch.zeros((total,), dtype=torch.uint8).pin_memory()
        self._host = {}
        pos = 0
        for name, dt, n, shape in fields:
            setattr(self, name, self._rows[pos:pos + n].view(dt).view(shape))
            self._host[name] = self._h_rows[pos:pos + n].view(dt).view(shape).numpy()
            pos += n
        self._host["geom"] = self._host["geom"].view(ops.GEOM_DTYPE)
        self.packed = torch.zeros((self.capacity,), dtype=torch.uint8, device=self.device)
        self._h_packed = torch.zeros((self.capacity,), dtype=torch.uint8).pin_memory()
        self._h_packed_np = self._h_packed.numpy()
        self._copied = torch.cuda.Event()  # the staging area is free again after it

    def load(self, frames):
        """frames: F arrays H_f x W_f x 3 uint8 BGR (numpy, or CPU tensors).  Validates
        them against the blob bound and the capacity (ValueError before anything is
        written), fills the pinned staging area and queues the copies."""
        cfg = self.cfg
        arrs = [f.numpy() if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames]
        if len(arrs) != self.F:
            raise ValueError("the batch holds %d frames, got %d" % (self.F, len(arrs)))
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                raise ValueError("a frame must be H x W x 3 uint8, got %s %s" % (a.shape, a.dtype))
        geo = ops.frame_geometry([a.shape[:2] for a in arrs], cfg.TEST.SCALE, cfg.TEST.MAX_SIZE,
                                 cfg.FPN.COARSEST_STRIDE)
        ops.check_geometry(geo, self.Hb, self.Wb, self.capacity)
        self._copied.synchronize()  # an earlier load's copies have left the staging area
        h = self._host
        for f, a in enumerate(arrs):
            o = geo.offset[f]
            self._h_packed_np[o:o + a.size] = a.reshape(-1)
        geo.fill_rows(h["geom"])
        h["im_info"][:] = geo.im_info()
        h["im_scale_t"][:] = geo.scale
        h["im_scale_d"][:] = geo.scale
        h["im_hw"][:] = geo.sizes
        self.packed[:geo.nbytes].copy_(self._h_packed[:geo.nbytes], non_blocking=True)
        self._rows.copy_(self._h_rows, non_blocking=True)
        self._copied.record()
        self.sizes = list(geo.sizes)
        return self


class RaggedFramePipeline(FramePipeline):
    """FramePipeline for frames of different sizes in one step (FPN configs), after
    the reference's im_list_to_blob (lib/utils/blob.py:86-114): every frame is
    scaled by its own get_target_scale, placed top-left in one F x 3 x Hb x Wb blob
    whose bound `blob_hw` is fixed here (a multiple of FPN.COARSEST_STRIDE, at
    least every frame's own padded size: ops.blob_bound), and zero elsewhere.
    Per frame, im_info = (Hp_f, Wp_f, s_f) is the row the single-image
    get_image_blob gives, boxes are divided by s_f and clipped to H_f x W_f, and
    the mask RoIs are scaled by s_f.

    Not promised: a frame whose own padded size is smaller than the bound does
    not give the detections it gives when run alone.  Alone, the convolutions
    pad the feature maps with zeros at the frame's own edge; in the batch they
    see the bias-driven features of the zero region there (the reference behaves
    the same whenever it batches).  Feature maps are not masked.

    All per-frame geometry lives in a RaggedBatch on the device and no frame size
    is a launch argument, so one captured step replays with other sizes."""
    GIVEN_BOXES = False

    def __init__(self, model, cfg, blob_hw, batch=1, capacity_bytes=None, channels_last=False,
                 det_cap=256, device="cuda"):
        if not cfg.FPN.FPN_ON:
            raise NotImplementedError("RaggedFramePipeline: C4 configs take an unpadded blob; "
                                      "only the FPN configs are supported")
        if bool(cfg.get("VOS", False)) or cfg.FPN.USE_GN or cfg.RESNETS.USE_GN:
            raise NotImplementedError("RaggedFramePipeline: VOS / GroupNorm configs are not "
                                      "supported (GroupNorm statistics would span the padding)")
        Hb, Wb = int(blob_hw[0]), int(blob_hw[1])
        st = int(cfg.FPN.COARSEST_STRIDE)
        if Hb < st or Wb < st or Hb % st or Wb % st:
            raise ValueError("blob_hw must be positive multiples of FPN.COARSEST_STRIDE = %d, "
                             "got %dx%d" % (st, Hb, Wb))
        self._setup(model, cfg, batch, channels_last, det_cap, device)
        self.Hp, self.Wp = Hb, Wb
        # the largest frames that fit the bound are at scale 1
        self.capacity = int(capacity_bytes) if capacity_bytes else batch * Hb * Wb * 3

    def new_batch(self) -> RaggedBatch:
        return RaggedBatch(self.F, self.capacity, (self.Hp, self.Wp), self.cfg, self.device)

    def make_blob(self, batch: RaggedBatch):
        nhwc = self.channels_last
        blob = ops.image_resize_to_blob_ragged(batch.packed, batch.geom, self.lut, self.Hp,
                                               self.Wp, nhwc=nhwc)
        return blob.permute(0, 3, 1, 2) if nhwc else blob  # NCHW view

    def _frame_rows(self, batch: RaggedBatch):
        return batch  # it carries the per-frame rows itself

    @torch.no_grad()
    def run(self, batch: RaggedBatch, keep_intermediates: bool = False, sync: bool = True,
            box_proposals=None):
        """batch: a loaded RaggedBatch of this pipeline (new_batch().load(frames)).
        Returns FramePipeline.run's dict plus im_hw, the batch's [F, 2] device rows;
        sync=False makes no host read and is graph-capturable.  complete() adds
        frame_hw, the host copy of im_hw that frame_segms sizes each RLE by."""
        if not isinstance(batch, RaggedBatch) or batch.F != self.F or \
                (batch.Hb, batch.Wb) != (self.Hp, self.Wp):
            raise ValueError("run() takes a RaggedBatch made by this pipeline's new_batch()")
        if batch.sizes is None:
            raise ValueError("the batch is empty: load() frames first")
        if box_proposals is not None:  # NotImplementedError by name, before batch.shape
            self._check_box_proposals(box_proposals, batch)
        return super().run(batch, keep_intermediates, sync)

    def _run(self, batch, keep_intermediates=False, sync=True):
        out = super()._run(batch, keep_intermediates, sync=False)
        out["im_hw"] = batch.im_hw
        if sync:
            self.complete(out)
        return out

    def complete(self, out: dict) -> dict:
        first = "counts_host" not in out
        out = super().complete(out)
        if first:
            out["frame_hw"] = [tuple(r) for r in out["im_hw"].cpu().tolist()]
        return out


def _ragged_frame_segms(pipe, out, ks, num_classes):
    from . import segm
    boxes = torch.cat([out["dets"][f, :k] for f, k in enumerate(ks)])
    classes = torch.cat([out["classes"][f, :k] for f, k in enumerate(ks)]).cpu().tolist()
    sizes = [list(hw) for hw in out["frame_hw"]]
    det_hw = np.repeat(np.asarray(sizes, np.int32).reshape(-1, 2), ks, axis=0)
    total = sum(ks)
    counts, n = ops.segm_rle_counts_ragged(out["masks"][:total], boxes, det_hw,
                                           pipe.cfg.MRCNN.THRESH_BINARIZE)
    strings = ops.rle_strings(counts, n)
    res, start = [], 0
    for f, k in enumerate(ks):
        rles = [{"size": sizes[f], "counts": s} for s in strings[start:start + k]]
        res.append(segm.group_by_class(rles, classes[start:start + k], num_classes))
        start += k
    return res


def frame_segms(pipe: FramePipeline, out: dict, num_classes: int = 81):
    """segm_results for every frame of a pipeline output: one fused paste + RLE
    launch and one rleToString pass over all frames' detections
    (vosdetectron_amd/segm.py), then the per-frame class grouping.  Returns a
    list over frames of cls_segms.  A RaggedFramePipeline output (completed) takes
    vd_segm_rle_ragged: still one launch, each RLE sized by its own frame."""
    from . import segm
    if isinstance(pipe, VOSPipeline) and pipe.heuristics_on():
        raise ValueError("frame_segms skips TEST.NMS_WITH_MASK_IOU / NMS_SMALL_BOX_IOU: use "
                         "VOSPipeline.frame_results for this config")
    ks = [int(k) for k in out["counts_host"]]
    total = sum(ks)
    if total == 0:
        return [[[] for _ in range(num_classes)] for _ in ks]
    if "frame_hw" in out:
        return _ragged_frame_segms(pipe, out, ks, num_classes)
    boxes = torch.cat([out["dets"][f, :k] for f, k in enumerate(ks)])
    classes = torch.cat([out["classes"][f, :k] for f, k in enumerate(ks)]).cpu().tolist()
    rles = segm.encode_masks(out["masks"][:total], boxes, pipe.H, pipe.W,
                             pipe.cfg.MRCNN.THRESH_BINARIZE)
    res, start = [], 0
    for k in ks:
        res.append(segm.group_by_class(rles[start:start + k], classes[start:start + k],
                                       num_classes))
        start += k
    return res


def frame_label_maps(pipe: FramePipeline, out: dict, thresh: float = 0.25, gt_thresh=None,
                     lut=None, valid=None):
    """viz_mask_result's object-ID maps (lib/utils/vis.py:119-157) of every frame of a
    step in one launch (ops.label_maps): -> (label, gt) uint8 device tensors
    [F, H, W], gt None without gt_thresh (the reference's rvt_cls_threshold).  Serves
    FramePipeline, VOSPipeline and C4FramePipeline outputs, completed or not: the
    counts are read on the device, so a run(sync=False) output needs no complete()
    first (detections past the padded mask batch -- exact score ties at
    DETECTIONS_PER_IM -- are painted only after complete()).  valid [F, det_cap]
    marks the rows a post-filter kept (VOSPipeline.frame_label_maps).  A
    RaggedFramePipeline output is refused: its frames differ in size."""
    if "frame_hw" in out or "im_hw" in out or isinstance(pipe, RaggedFramePipeline):
        raise NotImplementedError("frame_label_maps: a RaggedFramePipeline step holds frames of "
                                  "different sizes; label maps take one frame size per launch")
    # complete() has checked the counts and trimmed the masks to their sum
    return ops.label_maps(out["masks"], out["dets"], out["classes"], out["counts"], pipe.H,
                          pipe.W, thresh, gt_thresh, pipe.cfg.MRCNN.THRESH_BINARIZE, lut, valid,
                          rows_fit="counts_host" in out)


def frame_label_pngs(pipe: FramePipeline, out: dict, thresh: float = 0.25, gt_thresh=None,
                     lut=None, palette=None, valid=None):
    """frame_label_maps, then every frame's `label` as its DAVIS annotation file, an
    8-bit indexed PNG encoded on the device (ops.label_pngs; palette [256,3] uint8 RGB,
    default vis.davis_palette()): -> dict(label, gt, streams [F,cap] uint8, lengths [F]
    int32), all on the device and without a host read; streams[f, :lengths[f]] is
    frame f's file (vis.png_bytes, vis.write_pngs).  Refuses and accepts what
    frame_label_maps does."""
    label, gt = frame_label_maps(pipe, out, thresh, gt_thresh, lut, valid)
    streams, lengths = ops.label_pngs(label, palette)
    return {"label": label, "gt": gt, "streams": streams, "lengths": lengths}


def frame_label_objects(pipe: FramePipeline, out: dict, thresh: float = 0.25, gt_thresh=None,
                        lut=None, valid=None, which: str = "gt", **kw):
    """frame_label_maps, then the objects of every frame's `gt` (or `label`) map
    (ops.label_objects; kw: expand, remap255, obj_cap, rle_cap, want_rle, out): the
    reference's add_gt_annotations_to_entry on the last_gt viz_mask_result returned
    (train_davis_online.py:429), or with expand=None get_bboxes' boxes.  -> the
    ops.label_objects dict plus label and gt, all on the device; (boxes, counts) is a
    box_proposals argument of run().  Refuses and accepts what frame_label_maps does."""
    if which not in ("gt", "label"):
        raise ValueError("which must be 'gt' or 'label', got %r" % (which,))
    if which == "gt" and gt_thresh is None:
        raise ValueError("frame_label_objects: which='gt' needs gt_thresh")
    label, gt = frame_label_maps(pipe, out, thresh, gt_thresh, lut, valid)
    res = dict(ops.label_objects(gt if which == "gt" else label, **kw))
    res["label"], res["gt"] = label, gt
    return res


def check_flow_args(flow, raw_flow, F, frame_hw, blob_hw, device):
    """VOSPipeline.run's flow arguments: at most one of flow (blob resolution) and
    raw_flow (F x H x W x 2 fp32 at frame resolution, on `device`); raw_flow needs
    a blob whose sides are multiples of ops.FLOW_TILE.  ValueError names the
    argument.  Needs no device."""
    if raw_flow is None:
        return
    if flow is not None:
        raise ValueError("VOSPipeline.run: give flow (blob resolution) or raw_flow (frame "
                         "resolution), not both")
    if not isinstance(raw_flow, torch.Tensor) or raw_flow.dtype != torch.float32:
        raise ValueError("VOSPipeline.run: raw_flow must be a float32 tensor")
    want = (int(F), int(frame_hw[0]), int(frame_hw[1]), 2)
    if tuple(raw_flow.shape) != want:
        raise ValueError("VOSPipeline.run: raw_flow must be F x H x W x 2 = %s at the "
                         "pipeline's frame_hw, got %s" % (want, tuple(raw_flow.shape)))
    if raw_flow.device.type != torch.device(device).type:
        raise ValueError("VOSPipeline.run: raw_flow must be on the pipeline's device (%s), "
                         "got %s" % (device, raw_flow.device))
    Hp, Wp = blob_hw
    if Hp % ops.FLOW_TILE or Wp % ops.FLOW_TILE:
        raise ValueError("VOSPipeline.run: raw_flow needs a blob whose sides are multiples of "
                         "%d; this configuration's is %d x %d" % (ops.FLOW_TILE, Hp, Wp))


def check_delta_flow_args(flow, raw_flow, blob_hw):
    """VOSPipeline with MODEL.USE_DELTA_FLOW: the model makes the flow itself, so
    flow= and raw_flow= are refused (the reference silently overwrites them), and
    the blob sides must be multiples of ops.FLOW_TILE.  ValueError names the
    argument.  Needs no device."""
    if flow is not None:
        raise ValueError("VOSPipeline.run: flow was given, but MODEL.USE_DELTA_FLOW is on and "
                         "the model computes its own flow")
    if raw_flow is not None:
        raise ValueError("VOSPipeline.run: raw_flow was given, but MODEL.USE_DELTA_FLOW is on "
                         "and the model computes its own flow")
    Hp, Wp = blob_hw
    if Hp % ops.FLOW_TILE or Wp % ops.FLOW_TILE:
        raise ValueError("VOSPipeline: MODEL.USE_DELTA_FLOW needs a blob whose sides are "
                         "multiples of %d; this configuration's is %d x %d"
                         % (ops.FLOW_TILE, Hp, Wp))


class VOSPipeline(FramePipeline):
    """The VOS frame loop (lib_vos/tools/infer_davis_sequential.py:134-149 driving
    Generalized_VOS_RCNN._forward, vos_model_builder.py:289-447) for F sequences
    in lockstep: batch row b of every step is the next frame of sequence b, and
    the ConvGRU hidden states (one B x H x W x C tensor per level, in HBM) carry
    each sequence's state to its next frame.  `reset` starts new sequences
    (clean_hidden_states, :279-281)."""

    def __init__(self, model, cfg, frame_hw=(480, 854), batch=1, channels_last=False,
                 det_cap=256, device="cuda"):
        super().__init__(model, cfg, frame_hw, batch, channels_last, det_cap, device)
        self._flow = self._raw_flow = None
        # MODEL.USE_DELTA_FLOW: the model's own flow; level_flows holds the last
        # step's five level flows [P6 .. P2] (references, not copies)
        self.delta_flow = bool(cfg.MODEL.USE_DELTA_FLOW)
        self.level_flows = None
        if self.delta_flow:
            check_delta_flow_args(None, None, (self.Hp, self.Wp))
        # each sequence row's previous-frame result (prev_cls_boxes of the
        # reference loop, train_davis_online.py:591-592), for NMS_SMALL_BOX_IOU
        F = batch
        self.prev_dets = torch.zeros((F, det_cap, 5), dtype=torch.float32, device=self.device)
        self.prev_classes = torch.zeros((F, det_cap), dtype=torch.int32, device=self.device)
        self.prev_counts = torch.zeros((F,), dtype=torch.int32, device=self.device)
        # a step whose result frame_results / finalize has not yet recorded as the
        # previous frame (only tracked while a heuristic reads the previous result)
        self._unfinalized = False

    def heuristics_on(self) -> bool:
        """TEST.NMS_WITH_MASK_IOU / NMS_SMALL_BOX_IOU (vos_test.py:113-118, 845-860):
        both need frame_results, the step's mask-IoU NMS and the previous frame's
        final result."""
        tst = self.cfg.TEST
        return float(tst.NMS_WITH_MASK_IOU) > 0 or float(tst.NMS_SMALL_BOX_IOU) > 0

    def reset(self, rows=None):
        """Zero the hidden states (and forget the previous-frame results) of batch
        rows `rows` (all when None).  Resetting every row also drops the pending
        'unfinalized step' guard: no row's next frame reads that result any more."""
        if rows is None:
            self.prev_counts.zero_()
        else:
            self.prev_counts[list(rows)] = 0
        if rows is None or set(range(self.prev_counts.shape[0])) <= set(int(r) for r in rows):
            self._unfinalized = False
        if self.delta_flow:
            self.model.clean_flow_features(rows)
        hs = self.model.hidden_states
        if rows is None or all(h is None for h in hs):
            self.model.clean_hidden_states()
            return
        for h in hs:
            if h is not None:
                h[list(rows)] = 0

    def _post_detections(self, dets, classes, counts):
        """TEST.NMS_SMALL_BOX_IOU (lib_vos/tools/vos_test.py:845-860): each row's
        detections against its previous frame's final result, on the device.  Rows
        without a previous result (a new sequence) pass unchanged."""
        tst = self.cfg.TEST
        if float(tst.NMS_SMALL_BOX_IOU) > 0:
            F = dets.shape[0]
            ops.detections_prev_box_filter(dets, classes, counts, self.prev_dets[:F],
                                           self.prev_classes[:F], self.prev_counts[:F],
                                           tst.NMS_SMALL_BOX_IOU,
                                           tst.NMS_SMALL_BOX_SCORE_THRESHOLD)

    def finalize(self, out: dict) -> dict:
        """The device-only tail of a step: the mask-IoU NMS of every row and the
        record of each row's final result as the previous frame of its sequence
        (prev_cls_boxes, for NMS_SMALL_BOX_IOU), with no host read and no complete():
        after run(sync=False) + finalize(out) the next step can be queued.  With
        TEST.NMS_WITH_MASK_IOU > 0 one ops.mask_iou_nms_frames call over all rows;
        otherwise every row below its count is kept, in row order.  Stores
        out["keep"] [F,det_cap] int32 (row f's kept detections in the reference's
        output order), out["keep_counts"] [F] int32 and out["valid"] [F,det_cap]
        uint8.  A second call on the same out does nothing."""
        if "keep_counts" in out:
            return out
        tst = self.cfg.TEST
        dets, classes, counts = out["dets"], out["classes"], out["counts"]
        F, cap = dets.shape[0], dets.shape[1]
        prev = (self.prev_dets[:F], self.prev_classes[:F], self.prev_counts[:F])
        if float(tst.NMS_WITH_MASK_IOU) > 0:
            keep, keep_counts, valid = ops.mask_iou_nms_frames(
                out["masks"], dets, classes, counts, self.H, self.W,
                float(tst.NMS_WITH_MASK_IOU), int(tst.NUM_DET_PER_CLASS_POST),
                self.cfg.MRCNN.THRESH_BINARIZE, prev=prev, rows_fit="counts_host" in out)
            out["_finalize_rows"] = out["masks"].shape[0]
        else:
            idx = torch.arange(cap, dtype=torch.int32, device=dets.device)
            keep = idx.expand(F, cap).contiguous()
            keep_counts = counts.clone()
            valid = (idx[None, :] < counts[:, None]).to(torch.uint8)
            prev[0].copy_(dets)
            prev[1].copy_(classes)
            prev[2].copy_(counts.clamp(0, cap))
        out["keep"], out["keep_counts"], out["valid"] = keep, keep_counts, valid
        self._unfinalized = False
        return out

    def frame_results(self, out: dict, num_classes: int = None):
        """The tail of the VOS im_detect_all (lib_vos/tools/vos_test.py:50-120) for
        every row of a completed step: segm_results, then nms_with_mask_iou when
        TEST.NMS_WITH_MASK_IOU > 0 (:113-118: finalize()'s one device call over all
        rows, with the per-class cap of NUM_DET_PER_CLASS_POST).
        Returns a list over rows of (cls_boxes, cls_segms) -- cls_boxes[j] an
        [n_j, 5] float32 array -- and, unless finalize() already has, records each
        row's result as the previous frame of its sequence (prev_cls_boxes, for
        NMS_SMALL_BOX_IOU)."""
        from . import segm
        K = num_classes or int(self.cfg.MODEL.NUM_CLASSES)
        self.complete(out)
        self._check_finalize_rows(out)
        self.finalize(out)
        ks = [int(k) for k in out["counts_host"]]
        thr = self.cfg.MRCNN.THRESH_BINARIZE
        keep_h = out["keep"].cpu().numpy()
        nkeep = out["keep_counts"].cpu().tolist()
        dets_h, classes_h = out["dets"].cpu().numpy(), out["classes"].cpu().numpy()
        res, start = [], 0
        for f, k in enumerate(ks):
            dets = out["dets"][f, :k]
            masks = out["masks"][start:start + k]
            start += k
            rles = segm.encode_masks(masks, dets, self.H, self.W, thr)
            kept = keep_h[f, :nkeep[f]].astype(np.int64)
            kd_h, kc_h = dets_h[f][kept], classes_h[f][kept].tolist()
            kept = kept.tolist()
            cls_boxes = [np.zeros((0, 5), np.float32) for _ in range(K)]
            cls_segms = [[] for _ in range(K)]
            for j in sorted(set(kc_h)):
                rows = [i for i, c in enumerate(kc_h) if c == j]
                cls_boxes[j] = kd_h[rows]
                cls_segms[j] = [rles[kept[i]] for i in rows]
            res.append((cls_boxes, cls_segms))
        return res

    @staticmethod
    def _check_finalize_rows(out):
        """A finalize() before complete() saw the padded mask batch; if complete() then
        added rows (exact score ties at DETECTIONS_PER_IM), its NMS missed them."""
        rows = out.get("_finalize_rows")
        if rows is not None and sum(out["counts_host"]) > rows:
            raise RuntimeError("VOSPipeline.finalize ran on %d mask rows but the step holds %d "
                               "detections (score ties at DETECTIONS_PER_IM): complete() the "
                               "step before finalize()" % (rows, sum(out["counts_host"])))

    def frame_label_maps(self, out: dict, thresh: float = 0.25, gt_thresh=None, lut=None):
        """frame_label_maps of a step's output showing exactly the detections
        frame_results returns: with TEST.NMS_WITH_MASK_IOU > 0 the rows kept by the
        mask-IoU NMS (finalize(), run here if it has not: no host read, no complete())
        are passed as `valid`."""
        valid = None
        if float(self.cfg.TEST.NMS_WITH_MASK_IOU) > 0:
            valid = self.finalize(out)["valid"]
        return frame_label_maps(self, out, thresh, gt_thresh, lut, valid)

    def frame_label_pngs(self, out: dict, thresh: float = 0.25, gt_thresh=None, lut=None,
                         palette=None):
        """frame_label_pngs of the maps self.frame_label_maps gives: with
        TEST.NMS_WITH_MASK_IOU > 0 the files show the rows the mask-IoU NMS kept."""
        valid = None
        if float(self.cfg.TEST.NMS_WITH_MASK_IOU) > 0:
            valid = self.finalize(out)["valid"]
        return frame_label_pngs(self, out, thresh, gt_thresh, lut, palette, valid)

    def frame_label_objects(self, out: dict, thresh: float = 0.25, gt_thresh=None, lut=None,
                            which: str = "gt", **kw):
        """frame_label_objects of the maps self.frame_label_maps gives: with
        TEST.NMS_WITH_MASK_IOU > 0 the objects of the rows the mask-IoU NMS kept."""
        valid = None
        if float(self.cfg.TEST.NMS_WITH_MASK_IOU) > 0:
            valid = self.finalize(out)["valid"]
        return frame_label_objects(self, out, thresh, gt_thresh, lut, valid, which, **kw)

    def backbone(self, frames):
        feats = super().backbone(frames)
        if self.delta_flow:  # every step: the head's state must advance
            self.level_flows = self.model.delta_flow(feats)
            return self.model.temporal_fusion(feats, level_flows=self.level_flows)
        return self.model.temporal_fusion(feats, self._flow, level_flows=self._level_flows())

    def _level_flows(self):
        """The step's raw flow as the five FlowAlign level flows [P6 .. P2] (one
        vd_flow_to_levels launch), or None when nothing would read them: no raw
        flow, the static model, or every hidden state still unset."""
        if self._raw_flow is None or not self.cfg.CONVGRU.DYNAMIC_MODEL:
            return None
        if all(h is None for h in self.model.hidden_states):
            return None
        levels, _ = ops.flow_to_levels(self._raw_flow, self.im_scale, self.Hp, self.Wp)
        return levels[::-1]  # FlowAligns[i]: strides 64, 32, 16, 8, 4

    @torch.no_grad()
    def run(self, frames: torch.Tensor, flow: torch.Tensor = None, raw_flow: torch.Tensor = None,
            keep_intermediates=False, sync: bool = True, box_proposals=None):
        """frames: F x H x W x 3 u8 (frame t of each sequence); flow: optional
        F x 2 x Hp x Wp optical flow at blob resolution (flo_to_blob, data_flow);
        raw_flow: instead of flow, the F x H x W x 2 fp32 flow as read from the .flo
        files (flow_io.read_flo) at the pipeline's frame_hw, on the device -- it is
        resized, scaled, padded and brought to the five levels in one launch;
        sync and box_proposals as FramePipeline.run (sync False: complete() reads the
        counts later; box_proposals with MODEL.FASTER_RCNN False: the heads run on the
        caller's boxes, such as the previous step's kept rows that finalize() leaves on
        the device).
        With TEST.NMS_WITH_MASK_IOU / NMS_SMALL_BOX_IOU on, every step's result
        must pass through frame_results or finalize before the next step runs (the
        filter reads the previous frame's final result): raises otherwise."""
        if self._unfinalized and self.heuristics_on():
            raise RuntimeError(
                "VOSPipeline.run: the previous step's result has not been through "
                "frame_results() or finalize(); TEST.NMS_WITH_MASK_IOU / NMS_SMALL_BOX_IOU need "
                "it as the next frame's previous result (lib_vos/tools/vos_test.py:113-118, "
                "845-860)")
        if self.delta_flow:
            check_delta_flow_args(flow, raw_flow, (self.Hp, self.Wp))
        check_flow_args(flow, raw_flow, int(frames.shape[0]), (self.H, self.W), (self.Hp, self.Wp),
                        self.device)
        self._flow, self._raw_flow = flow, raw_flow
        try:
            out = super().run(frames, keep_intermediates, sync=sync,
                              box_proposals=box_proposals)
        finally:
            self._flow = self._raw_flow = None
        self._unfinalized = True
        return out
