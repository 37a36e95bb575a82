"""The workspace-taking C entries called with a workspace one byte short and with a null
one (tests/test_guarded_cpu.py).  Run as a module it prints the statuses as JSON; the
test starts it in a child process that sees no device, so an entry whose check were
ever lost could not launch its kernels on the host buffers passed here."""
import ctypes
import json

ENTRY_NAMES = ["vd_roi_align_fpn_tiled_forward", "vd_nms", "vd_mask_iou_nms",
               "vd_generate_proposals", "vd_box_detections", "vd_box_detections_ex",
               "vd_box_union_add_view", "vd_box_union_add_view_ar", "vd_box_union_detections",
               "vd_group_norm_act", "vd_group_norm_act (two sets)", "vd_convgru_gates",
               "vd_convgru_update"]


def ws_entries():
    """name -> (size in bytes, call(workspace pointer or None, workspace_bytes)).  Every
    other pointer argument is a small host buffer: the check comes before any launch,
    so nothing reads it."""
    from vosdetectron_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    w4 = (ctypes.c_float * 4)(10., 10., 5., 5.)
    wp = ctypes.cast(w4, ctypes.c_void_p)
    rpn = (_lib.VdRpnLevel * 1)(_lib.VdRpnLevel(p, p, p, 3, 20, 28, 1. / 16))
    fpn = (_lib.VdFeatLevel * 2)(_lib.VdFeatLevel(p, 50, 84, 0.25), _lib.VdFeatLevel(p, 25, 42, 0.125))
    return {
        "vd_roi_align_fpn_tiled_forward": (
            L.vd_roi_align_fpn_tiled_workspace_size(fpn, 2, 1, 64, 8, 7),
            lambda w, n: L.vd_roi_align_fpn_tiled_forward(fpn, 2, 1, 64, p, p, 8, 7, 2, p, w, n,
                                                          None)),
        "vd_nms": (L.vd_nms_workspace_size(100),
                   lambda w, n: L.vd_nms(p, 100, 5, 0.5, p, p, w, n, None)),
        "vd_mask_iou_nms": (L.vd_mask_iou_nms_workspace_size(5, 37, 53),
                            lambda w, n: L.vd_mask_iou_nms(p, 5, 37, 53, p, 5, p, 0.5, 2, p, p, w,
                                                           n, None)),
        "vd_generate_proposals": (
            L.vd_generate_proposals_workspace_size(rpn, 1, 2, 1000),
            lambda w, n: L.vd_generate_proposals(rpn, 1, 2, p, 1000, 300, 0.7, 0., p, p, p, w, n,
                                                 None)),
        "vd_box_detections": (
            L.vd_box_detections_workspace_size(65, 2, 3),
            lambda w, n: L.vd_box_detections(p, p, p, p, 65, 2, 3, p, p, 0.05, 0.5, 100, wp, 64,
                                             p, p, p, w, n, None)),
        "vd_box_detections_ex": (
            L.vd_box_detections_workspace_size(65, 2, 3),
            lambda w, n: L.vd_box_detections_ex(p, p, p, p, 65, 2, 3, p, p, 0.05, 0.5, 100, wp, 1,
                                                0.5, 0.0001, 1, 0.8, 1.0, 64, p, p, p, w, n,
                                                None)),
        "vd_box_union_add_view": (
            L.vd_box_union_workspace_size(40, 2, 3),
            lambda w, n: L.vd_box_union_add_view(p, p, p, p, 48, 2, 3, p, p, 0, 1, 0.05, wp, 40,
                                                 w, n, None)),
        "vd_box_union_add_view_ar": (
            L.vd_box_union_workspace_size(40, 2, 3),
            lambda w, n: L.vd_box_union_add_view_ar(p, p, p, p, 48, 2, 3, p, p, 1, 0.8, 1, 0.05,
                                                    wp, 40, w, n, None)),
        "vd_box_union_detections": (
            L.vd_box_union_workspace_size(40, 2, 3),
            lambda w, n: L.vd_box_union_detections(40, 2, 3, 0.5, 100, -1, 0.5, 0.0001, -1, 0.8,
                                                   1.0, 64, p, p, p, None, w, n, None)),
        "vd_group_norm_act": (
            L.vd_group_norm_workspace_size(2, 32),
            lambda w, n: L.vd_group_norm_act(p, None, 2, 64, 5, 7, 32, 1e-5, p, p, None, 0, None,
                                             None, 0, 0, p, w, n, None)),
        "vd_group_norm_act (two sets)": (
            2 * L.vd_group_norm_workspace_size(2, 32),
            lambda w, n: L.vd_group_norm_act(p, None, 2, 64, 5, 7, 32, 1e-5, p, p, p, 3, p, p, 1,
                                             0, p, w, n, None)),
        "vd_convgru_gates": (
            2 * L.vd_group_norm_workspace_size(2, 32),
            lambda w, n: L.vd_convgru_gates(p, p, p, p, p, 2, 64, 5, 7, 32, 1e-5, p, p, p, p, 0, p,
                                            p, w, n, None)),
        "vd_convgru_update": (
            L.vd_group_norm_workspace_size(2, 32),
            lambda w, n: L.vd_convgru_update(p, p, p, p, None, 2, 64, 5, 7, 32, 1e-5, p, p, 0, p,
                                             w, n, None)),
    }, buf


def statuses():
    entries, buf = ws_entries()
    assert sorted(entries) == sorted(ENTRY_NAMES)
    ws = ctypes.addressof(buf)
    return {name: [int(size), call(ws, size - 1), call(None, size), call(None, 0)]
            for name, (size, call) in entries.items()}


if __name__ == "__main__":
    print("WS_STATUSES " + json.dumps(statuses()))
