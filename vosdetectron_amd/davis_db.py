"""The reference's DAVIS_imdb entries that consume a label map (imdb/vos/davis_db.py),
on maps that live on the device.

get_gt(labels)              :180-189  the 255 remap, as a map
get_bboxes(labels)          :191-204 with lib_vos/tools/get_cls_mapper.py:129-136: one box
                            (x, y, x + w, y + h) float32 per object -- the box_proposals
                            the heads then run on
add_gt_annotations(labels)  :407-517  add_gt_annotations_to_entry's boxes / seg_areas /
                            instance_id / segms fields per frame (the online loop's
                            pseudo ground truth, train_davis_online.py:429)

get_bboxes and add_gt_annotations are one ops.label_objects call (vd_label_objects) over
every frame; the maps are not copied to the host.  The rest of the roidb entry
(gt_overlaps, the class mapping) is not built here.
"""
import numpy as np
import torch

from . import ops


_GT_CHUNK = 1 << 16  # pixels per frame whose scatter index is live at once (F x 512 KiB)
DEFAULT_OBJ_CAP = 32  # objects per frame the entries below make room for (DAVIS has <= 10)


def get_gt(labels: torch.Tensor) -> torch.Tensor:
    """get_gt's map of every frame: where 255 occurs in a frame its pixels take
    len(np.unique(frame)) - 1.  labels [F,H,W] (or [H,W]) uint8; plain torch, no host
    read."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or \
            labels.dim() not in (2, 3):
        raise ValueError("labels must be an F x H x W (or H x W) uint8 tensor")
    lab = labels if labels.dim() == 3 else labels[None]
    F = lab.shape[0]
    flat = lab.reshape(F, -1)
    present = torch.zeros((F, 256), dtype=torch.bool, device=lab.device)
    one = torch.ones((1, 1), dtype=torch.bool, device=lab.device)
    for a in range(0, flat.shape[1], _GT_CHUNK):  # the int64 index of one chunk at a time
        idx = flat[:, a:a + _GT_CHUNK].to(torch.int64)
        present.scatter_(1, idx, one.expand_as(idx))
    target = (present.sum(1) - 1).to(torch.uint8)  # 255 present: at least one value
    out = torch.where(lab == 255, target[:, None, None], lab)
    return out if labels.dim() == 3 else out[0]


def get_bboxes(labels: torch.Tensor, obj_cap: int = DEFAULT_OBJ_CAP):
    """get_bboxes of every frame after get_gt's remap, in get_cls_mapper's box form:
    -> (boxes [F,obj_cap,4] fp32 (x, y, x + w, y + h), counts [F] int32) on the device,
    objects in ascending value order: a box_proposals argument of FramePipeline.run.  A
    frame with more than obj_cap (<= 255) objects has counts[f] = -1, which run() raises
    on."""
    res = ops.label_objects(labels, expand=None, remap255=True, obj_cap=obj_cap, want_rle=False)
    return res["boxes"], res["counts"]


def add_gt_annotations(labels: torch.Tensor, expand: float = 0.05, remap255: bool = False,
                       obj_cap: int = DEFAULT_OBJ_CAP) -> list:
    """add_gt_annotations_to_entry's fields of every frame: a list of F dicts with boxes
    [k,4] float32 (expanded, clipped, filtered), seg_areas [k] float32, instance_id [k]
    int32 and segms, k dicts {'size': [H, W], 'counts': bytes} as mask_util.encode
    returns them.  One device call, then a few KB to the host.  On the device the RLE
    rows take F * obj_cap * (4 W + 2) * 4 bytes (44 MB for 64 maps of 800 x 1333 at the
    default obj_cap of 32; 348 MB at 255); a frame with more than obj_cap (<= 255) kept
    objects raises VosdetError."""
    res = ops.label_objects(labels, expand=expand, remap255=remap255, obj_cap=obj_cap)
    F, H, W = (int(v) for v in labels.shape)
    counts = res["counts"].cpu().numpy()
    ops.raise_on_failed_counts(counts, "label map")
    live = torch.arange(obj_cap, device=labels.device)[None, :] < res["counts"][:, None]
    n = torch.where(live, res["rle_n"], 0).to(torch.int32).reshape(-1).contiguous()
    strings = ops.rle_strings(res["rle_counts"].reshape(F * obj_cap, -1), n)
    boxes, areas, ids = (res[k].cpu().numpy() for k in ("boxes", "areas", "ids"))
    out = []
    for f in range(F):
        k = int(counts[f])
        out.append({
            "boxes": boxes[f, :k].copy(),
            "seg_areas": areas[f, :k].astype(np.float32),
            "instance_id": ids[f, :k].astype(np.int32),
            "segms": [{"size": [H, W], "counts": strings[f * obj_cap + i].encode("ascii")}
                      for i in range(k)],
        })
    return out
