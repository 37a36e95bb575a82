#!/usr/bin/env python3
"""tests/golden/label_objects.npz: the reference's own DAVIS_imdb.get_gt, get_bboxes,
_expand_box and add_gt_annotations_to_entry (imdb/vos/davis_db.py:180-204, :399-535) and
box_utils.xywh_to_xyxy / clip_xyxy_to_image (lib/utils/boxes.py) executed in this container
on one 37 x 83 label map (tests/label_objects_ref.golden_frame()).

imdb/vos/davis_db.py cannot be imported here: at module level it needs the DAVIS API, PIL,
matplotlib, cv2 and pycocotools, and gen_goldens.install_shims itself replaces the module
by a placeholder.  So the four methods are taken out of the reference's file as syntax
trees at run time (nothing is copied into this repository), compiled unchanged and run on
a stub `self` that carries the annotation and the few attributes they read.  utils.boxes is
the reference's module, imported under install_shims.

cv2 and pycocotools are absent, so the two third-party calls are stubs made of the
restatement in tests/label_objects_ref.py: cv2.boundingRect -> bounding_rect,
mask_util.encode -> {'size', 'counts': rle_counts(mask)} (the run lengths, not the
compressed string).  Everything else -- np.unique, the 255 remap, _expand_box, the
conversion and clip, the validity filter, the float32 entry arrays, their order -- is the
reference's code.  Parity of boundingRect and mask.encode with an executed cv2 /
pycocotools is therefore unpinned here; the RLE is pinned against the already pinned
vd_mask_rle in tests/test_label_objects_gpu.py.

Contents: the map; get_gt's map; get_bboxes' [x, y, w, h] rows and get_cls_mapper's
float32 (x, y, x + w, y + h) form of them; and, for the raw map and for get_gt's map, the
entry's boxes (float32), seg_areas, instance_id and the segms' run lengths (concatenated,
with their lengths).  Member timestamps are fixed: the file regenerates byte for byte.

Usage: python tools/gen_label_objects_goldens.py   (writes tests/golden/label_objects.npz)
"""
import ast
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_goldens import OUT, REF, install_shims  # noqa: E402
from gen_label_map_goldens import save_npz  # noqa: E402

METHODS = ("get_gt", "get_bboxes", "_expand_box", "add_gt_annotations_to_entry")


def reference_methods(namespace):
    """The reference's DAVIS_imdb methods, compiled from its own file into `namespace`."""
    path = os.path.join(REF, "imdb", "vos", "davis_db.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DAVIS_imdb")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(n.name for n in fns) == sorted(METHODS)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), namespace)
    return {name: namespace[name] for name in METHODS}


class _Csr:
    """scipy.sparse.csr_matrix as the entry uses it (a holder with toarray and shape)."""

    def __init__(self, a):
        self.a = np.asarray(a)
        self.shape = self.a.shape

    def toarray(self):
        return self.a


def main():
    install_shims()
    import utils.boxes as box_utils
    from tests import label_objects_ref as lo

    cv2 = types.SimpleNamespace(boundingRect=lo.bounding_rect)
    mask_util = types.SimpleNamespace(
        encode=lambda m: {"size": list(m.shape), "counts": lo.rle_counts(m)})
    try:
        import scipy.sparse as sparse
    except ImportError:
        sparse = types.SimpleNamespace(csr_matrix=_Csr)
    ns = {"np": np, "cv2": cv2, "mask_util": mask_util, "box_utils": box_utils,
          "scipy": types.SimpleNamespace(sparse=sparse), "print": lambda *a, **k: None}
    ref = reference_methods(ns)

    lab = np.array(lo.golden_frame())
    H, W = lab.shape
    this = types.SimpleNamespace(
        db=types.SimpleNamespace(annotations=[[lab]]), seq_idx=0, cls_mapper=None,
        use_local_id=True, global_instance_id_start_of_seq=[1], num_classes=256,
        number_of_instance_ids=300)
    for name in METHODS:
        setattr(this, name, types.MethodType(ref[name], this))

    gt = this.get_gt(0)
    assert gt.dtype == np.uint8 and (lab == 255).any() and not (gt == 255).any()
    xywh = np.asarray(this.get_bboxes(0), np.int32).reshape(-1, 4)
    # lib_vos/tools/get_cls_mapper.py:128-136, on the list get_bboxes returned
    new_boxes = []
    for bbox in this.get_bboxes(0):
        new_box = []
        new_box.extend(bbox)
        new_box[2] = new_box[0] + new_box[2]
        new_box[3] = new_box[1] + new_box[3]
        new_boxes.append(new_box)
    rect_boxes = np.array(new_boxes, np.float32)

    def entry_of(a_map):
        entry = {"seq_idx": 0, "idx": 0, "width": W, "height": H,
                 "boxes": np.empty((0, 4), dtype=np.float32), "segms": [],
                 "gt_classes": np.empty((0), dtype=np.int32),
                 "global_instance_id": np.empty((0), dtype=np.int32),
                 "instance_id": np.empty((0), dtype=np.int32),
                 "seg_areas": np.empty((0), dtype=np.float32),
                 "gt_overlaps": sparse.csr_matrix(np.empty((0, 256), dtype=np.float32)),
                 "gt_overlaps_id": sparse.csr_matrix(np.empty((0, 300), dtype=np.float32)),
                 "is_crowd": np.empty((0), dtype=bool),
                 "box_to_gt_ind_map": np.empty((0), dtype=np.int32)}
        this.add_gt_annotations_to_entry(entry, a_map)
        assert entry["boxes"].dtype == np.float32 and entry["seg_areas"].dtype == np.float32
        runs = [np.asarray(s["counts"], np.uint32) for s in entry["segms"]]
        return dict(boxes=entry["boxes"], seg_areas=entry["seg_areas"],
                    instance_id=entry["instance_id"].astype(np.int32),
                    rle=np.concatenate(runs) if runs else np.zeros(0, np.uint32),
                    rle_n=np.asarray([len(r) for r in runs], np.int32))

    raw, mapped = entry_of(lab), entry_of(gt)
    assert len(raw["boxes"]) >= 5 and len(xywh) == len(rect_boxes) >= 5

    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "label_objects.npz")
    arrays = dict(labels=lab, gt=gt, bboxes_xywh=xywh, rect_boxes=rect_boxes,
                  expand=np.float64(0.05))
    for tag, e in (("raw", raw), ("gt", mapped)):
        for k, v in e.items():
            arrays["%s_%s" % (tag, k)] = v
    save_npz(path, **arrays)
    size = os.path.getsize(path)
    assert size <= 1 << 20, size
    print("wrote %s (%d bytes): %d objects, %d kept by the entry filter"
          % (path, size, len(xywh), len(mapped["boxes"])))


if __name__ == "__main__":
    main()
