"""CPU reference of the test-time augmentation (TEST INFRASTRUCTURE ONLY).

lib/core/test.py:193-363 (im_detect_bbox_aug and its per-view helpers) and :405-526
(im_detect_mask_aug), restated line by line on the oracle's numpy parts and the
independent CPU pipeline (oracle/pipeline.py RefCPUPipeline: torch-CPU convolutions,
numpy proposals, C RoIAlign / NMS).  Nothing here imports the product's kernels.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle as orc


def flip_boxes(boxes, im_width):
    """lib/utils/boxes.py:261-266."""
    boxes_flipped = boxes.copy()
    boxes_flipped[:, 0::4] = im_width - boxes[:, 2::4] - 1
    boxes_flipped[:, 2::4] = im_width - boxes[:, 0::4] - 1
    return boxes_flipped


def views(test_scale, test_max_size, aug, identity_last):
    """The (scale, max_size, hflip) views of test.py:218-261 (identity last) or
    :425-445 (identity first) for one AUG block given as a dict / AttrDict."""
    v = []
    if aug["H_FLIP"]:
        v.append((test_scale, test_max_size, True))
    for s in aug["SCALES"]:
        v.append((s, aug["MAX_SIZE"], False))
        if aug["SCALE_H_FLIP"]:
            v.append((s, aug["MAX_SIZE"], True))
    ident = (test_scale, test_max_size, False)
    return v + [ident] if identity_last else [ident] + v


def logit(y):
    """test.py:465-466."""
    return -1.0 * np.log((1.0 - y) / np.maximum(y, 1e-20))


def combine_masks(masks_ts, heur):
    """test.py:458-474 on the list of per-view masks (already inverted)."""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if heur == "SOFT_AVG":
            return np.mean(masks_ts, axis=0)
        if heur == "SOFT_MAX":
            return np.amax(masks_ts, axis=0)
        if heur == "LOGIT_AVG":
            logit_masks = [logit(y) for y in masks_ts]
            logit_masks = np.mean(logit_masks, axis=0)
            return 1.0 / (1.0 + np.exp(-logit_masks))
    raise NotImplementedError("Heuristic {} not supported".format(heur))


def logit_avg_float32_error(masks_ts):
    """max |float32 evaluation - float64 evaluation| of LOGIT_AVG over the elements
    where the float64 result is finite: the rounding error of the reference's own
    arithmetic on these inputs."""
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        f32 = combine_masks(masks_ts, "LOGIT_AVG")
        m64 = [np.asarray(m, np.float64) for m in masks_ts]
        lg = [-1.0 * np.log((1.0 - y) / np.maximum(y, np.float64(np.float32(1e-20))))
              for y in m64]
        f64 = 1.0 / (1.0 + np.exp(-np.mean(lg, axis=0)))
    ok = np.isfinite(f64) & np.isfinite(f32)
    return float(np.abs(f32[ok].astype(np.float64) - f64[ok]).max()) if ok.any() else 0.0


def invert_masks(masks, hflip):
    """test.py:491: masks_hf[:, :, :, ::-1] (here on class-selected [M, R, R])."""
    return masks[:, :, ::-1] if hflip else masks


def union(scores_ts, boxes_ts):
    """test.py:268-281 with the UNION heuristics."""
    return np.vstack(scores_ts), np.vstack(boxes_ts)


def decode_view(rois, deltas, im_scale, im_shape, hflip, weights=(10., 10., 5., 5.)):
    """im_detect_bbox's decode (test.py:157-179) + im_detect_bbox_hflip's inversion
    (:308-309) of one view: rois [n, 5] in the view's blob coordinates -> boxes [n, 4K]
    on the original frame."""
    boxes = rois[:, 1:5] / im_scale
    pred = orc.clip_tiled_boxes(orc.bbox_transform(boxes, deltas, weights), im_shape)
    return flip_boxes(pred, im_shape[1]) if hflip else pred


class AugRef:
    """im_detect_bbox_aug + box_results_with_nms_and_limit + im_detect_mask_aug on the
    independent CPU pipeline `ref` (a RefCPUPipeline)."""

    def __init__(self, ref, stride=32):
        self.ref, self.stride = ref, stride
        self.level_scales = [1. / 32, 1. / 16, 1. / 8, 1. / 4]

    @torch.no_grad()
    def conv_body(self, im, scale, max_size):
        """im_conv_body_only (test.py:114-125)."""
        blob, im_scale, im_info = orc.get_image_blob(im, target_scale=scale, max_size=max_size,
                                                     stride=self.stride)
        return self.ref.backbone(torch.from_numpy(blob)), im_scale, im_info

    @torch.no_grad()
    def box_view(self, im, scale, max_size, hflip=False):
        """im_detect_bbox / im_detect_bbox_hflip -> (scores [n, K], boxes [n, 4K] on the
        original frame, extra)."""
        r, sd = self.ref, self.ref.sd
        src = im[:, ::-1, :] if hflip else im
        fpn, im_scale, im_info = self.conv_body(np.ascontiguousarray(src), scale, max_size)
        rois_l, probs_l = [], []
        for lvl in range(2, 7):
            t = fpn[6 - lvl]
            h = F.relu(r._conv(t, "RPN.FPN_RPN_conv", 1, 1))
            cls = torch.sigmoid(r._conv(h, "RPN.FPN_RPN_cls_score")).numpy()
            dl = r._conv(h, "RPN.FPN_RPN_bbox_pred").numpy()
            ro, pr = orc.generate_proposals(r.anchors[lvl], 1. / 2 ** lvl, cls, dl, im_info,
                                            r.pre_nms, r.post_nms, r.rpn_nms, 0)
            rois_l.append(ro)
            probs_l.append(pr)
        rois = orc.collect(rois_l, probs_l, r.post_nms)
        blobs = [f.numpy() for f in fpn[1:]]
        bf = orc.roi_feature_transform(blobs, orc.distribute(rois), "rois", r.box_res,
                                       self.level_scales, r.box_sr)
        x = torch.from_numpy(bf).reshape(bf.shape[0], -1)
        x = F.relu(F.linear(x, sd["Box_Head.fc1.weight"], sd["Box_Head.fc1.bias"]))
        x = F.relu(F.linear(x, sd["Box_Head.fc2.weight"], sd["Box_Head.fc2.bias"]))
        scores = F.softmax(F.linear(x, sd["Box_Outs.cls_score.weight"],
                                    sd["Box_Outs.cls_score.bias"]), dim=1).numpy()
        deltas = F.linear(x, sd["Box_Outs.bbox_pred.weight"],
                          sd["Box_Outs.bbox_pred.bias"]).numpy()
        boxes = decode_view(rois, deltas, im_scale, im.shape, hflip)
        return scores, boxes, dict(rois=rois, deltas=deltas, im_scale=im_scale, blobs=blobs)

    @torch.no_grad()
    def mask_view(self, im, scale, max_size, hflip, boxes, classes, blobs=None):
        """im_detect_mask on a view (im_detect_mask_hflip / _scale, test.py:479-506):
        class-selected [M, R, R] masks, a flipped view's inverted."""
        r, sd = self.ref, self.ref.sd
        src = im[:, ::-1, :] if hflip else im
        if blobs is None:
            fpn, im_scale, _ = self.conv_body(np.ascontiguousarray(src), scale, max_size)
            blobs = [f.numpy() for f in fpn[1:]]
        else:
            blobs, im_scale = blobs
        b = flip_boxes(boxes, im.shape[1]) if hflip else boxes
        mrois = np.hstack([np.zeros((b.shape[0], 1)), b.astype(np.float64) * im_scale])
        mrois = mrois.astype(np.float32)
        mf = orc.roi_feature_transform(blobs, orc.distribute(mrois, prefix="mask_rois"),
                                       "mask_rois", r.mask_res, self.level_scales, r.mask_sr)
        y = torch.from_numpy(mf)
        for i in range(4):
            y = F.relu(r._conv(y, "Mask_Head.conv_fcn.%d" % (2 * i), 1, r.mask_dil, r.mask_dil))
        y = F.relu(F.conv_transpose2d(y, sd["Mask_Head.upconv.weight"],
                                      sd["Mask_Head.upconv.bias"], 2))
        m = torch.sigmoid(r._conv(y, "Mask_Outs.classify")).numpy()
        return invert_masks(m[np.arange(len(classes)), classes], hflip), mrois

    def __call__(self, im, box_views, mask_views, heur="SOFT_AVG", **box_results_kw):
        """-> (scores, boxes, classes, combined masks, extra): im_detect_all with both
        AUG blocks (test.py:62-95)."""
        r = self.ref
        per_view, kept = [], {}
        for v in box_views:
            sc, bx, ex = self.box_view(im, *v)
            per_view.append((sc, bx, ex))
            kept[v] = (ex["blobs"], ex["im_scale"])
        scores_c, boxes_c = union([p[0] for p in per_view], [p[1] for p in per_view])
        sc, bx, cls_boxes = orc.box_results_with_nms_and_limit(
            scores_c, boxes_c, r.K, r.score_thresh, r.test_nms, r.dets_per_im, **box_results_kw)
        classes = np.concatenate([[j] * len(cls_boxes[j]) for j in range(1, r.K)] +
                                 [np.zeros((0,))]).astype(np.int32)
        extra = dict(per_view=per_view, scores_c=scores_c, boxes_c=boxes_c)
        if bx.shape[0] == 0:
            return sc, bx, classes, np.zeros((0, 28, 28), np.float32), extra
        # the body of a view is deterministic: a view run in the box pass is not run again
        masks_ts = [self.mask_view(im, *v, boxes=bx, classes=classes, blobs=kept.get(v))[0]
                    for v in mask_views]
        extra["masks_ts"] = masks_ts
        return sc, bx, classes, combine_masks(masks_ts, heur), extra
