// nms_with_mask_iou's sequential part (lib_vos/tools/vos_test.py:985-1029) for one
// frame in one workgroup, shared by vd_mask_iou_nms (vos_post.hip) and
// vd_mask_iou_nms_frames (mask_nms_frames.hip): the score order, the greedy
// discard pass over the pair intersections, the per-class cap and the
// class-major output order.  One definition, so both entries keep the same rows.
#pragma once
#include "common.hpp"

namespace vd {

static constexpr int kMaxMaskNms = 1024;  // detections per frame (the LDS lists)

// score(d), cls(d), area(d): detection d's score (float), class (int) and mask
// area (integer); inter(i, j), i < j: the pair's intersection (int);
// emit(pos, d): detection d is the pos-th kept row.  order / disc / sel: LDS
// int[kMaxMaskNms].  Every thread of the workgroup calls it; n <= kMaxMaskNms.
// Returns the number of kept rows (the same value in every thread).  order /
// disc / sel may be read after a barrier; emit's writes are not yet fenced.
template <class Score, class Cls, class Area, class Inter, class Emit>
__device__ __forceinline__ int mask_nms_greedy(int n, Score score, Cls cls, Area area, Inter inter,
                                               double iou_th, int max_per_class, int *order,
                                               int *disc, int *sel, Emit emit) {
    const int t = threadIdx.x;
    // np.argsort(-scores), read stably: rank = #{k: s_k > s_t or (s_k == s_t, k < t)}
    for (int d = t; d < n; d += blockDim.x) {
        const float s = score(d);
        int rank = 0;
        for (int k = 0; k < n; ++k) {
            const float sk = score(k);
            rank += (sk > s) || (sk == s && k < d);
        }
        order[rank] = d;
    }
    for (int q = t; q < n; q += blockDim.x) disc[q] = 0;
    __syncthreads();
    for (int p = 0; p < n; ++p) {
        if (!disc[p]) {  // uniform: read after the barrier
            const int i = order[p];
            const double ai = (double)area(i) + 1e-6;
            for (int q = p + 1 + t; q < n; q += blockDim.x) {
                const int j = order[q];
                const int in = inter(min(i, j), max(i, j));
                const double iou1 = (double)in / ai;
                const double iou2 = (double)in / ((double)area(j) + 1e-6);
                if (iou1 > iou_th || iou2 > iou_th) disc[q] = 1;
            }
        }
        __syncthreads();
    }
    // the per-class cap in score order over the kept positions
    for (int q = t; q < n; q += blockDim.x) {
        int ok = 0;
        if (!disc[q]) {
            const int c = cls(order[q]);
            int before = 0;
            for (int u = 0; u < q; ++u) before += !disc[u] && cls(order[u]) == c;
            ok = before < max_per_class;
        }
        sel[q] = ok;
    }
    __syncthreads();
    // class-major output: class ascending, then score order
    int nsel = 0;
    for (int q = t; q < n; q += blockDim.x) {
        if (!sel[q]) continue;
        const int c = cls(order[q]);
        int pos = 0;
        for (int u = 0; u < n; ++u) {
            if (!sel[u]) continue;
            const int cu = cls(order[u]);
            pos += cu < c || (cu == c && u < q);
        }
        emit(pos, order[q]);
    }
    for (int q = 0; q < n; ++q) nsel += sel[q];
    return nsel;
}

}  // namespace vd
