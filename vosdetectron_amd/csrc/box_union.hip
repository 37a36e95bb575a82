// Box test-time augmentation with the UNION heuristics, on device.
//
// Reference (host numpy per frame):
//   im_detect_bbox_aug                      lib/core/test.py:193-287
//     per view im_detect_bbox (:128-190) [+ flip_boxes, lib/utils/boxes.py:261-266,
//     im_detect_bbox_hflip :290-311], then scores_c / boxes_c = np.vstack over the views
//   box_results_with_nms_and_limit on the union   lib/core/test.py:733-797
//
// The union of T views holds T x R rows per image, past what class_nms_kernel
// keeps in LDS (kDetRMax), so the per-class candidate lists live in global memory:
//
// Kernel 1 (vd_box_union_add_view, once per view in vstack order): one workgroup
//   per (class j >= 1, image): ordered compaction of the view's rows with score >=
//   thresh, class_nms_kernel's decode + clip, flip_boxes for a flipped view, the
//   aspect-ratio view's x * (1 / ar) (vd_box_union_add_view_ar, boxes.py:269-274), and
//   the rows appended to the class's list behind the earlier views' (the position
//   is the list's count plus the row's rank in the view, so a list holds the
//   vstack order: view-major, then proposal index).
// Kernel 2 (vd_box_union_detections): one workgroup per (class, image): the list
//   sorted by (score desc, higher vstack index first) with the keys in LDS, then
//   the greedy NMS over the sorted list in blocks of kUnionBlock boxes: a block is
//   first tested against the survivors of the earlier blocks (streamed through
//   LDS), what is left of it is resolved with nms_block.hpp's row masks, and its
//   survivors join the stream.  No n x n mask exists at any point.  TEST.SOFT_NMS
//   and TEST.BBOX_VOTE as in class_nms_kernel (voters: all of the class's
//   candidates).  det_limit_kernel (detections.hip) then makes the image's result.
#include "det_block.hpp"

namespace vd {

static constexpr int kUnionCandMax = 16384;
static constexpr int kUnionBlock = 512;

// Workspace: per (image, class) slot of cand_cap rows
//   cand      5 float planes (x1, y1, x2, y2, score), vstack order      20 B / row
//   cls_dets  the class's result rows [5]; while the NMS runs, the
//             survivors' 5 planes (x1, y1, x2, y2, area)                 20 B / row
//   order     sorted rank -> row of cand                                  4 B / row
//   keep      survivor flag per row of cand                               1 B / row
// and per slot the list's count and the result's count, per image the status
// (-1: a view's proposal selection failed, or a list overflowed cand_cap).
struct UnionWs {
    float *cand;
    float *cls_dets;
    int32_t *order;
    uint8_t *keep;
    int32_t *cand_count;  // cand_count, cls_count and status are contiguous (zeroed together)
    int32_t *cls_count;
    int32_t *status;
    size_t counter_bytes;
};

size_t box_union_workspace_bytes(int cand_cap, int num_images, int K) {
    const size_t slots = (size_t)num_images * K;
    return 2 * al256(slots * cand_cap * 5 * sizeof(float)) + al256(slots * cand_cap * 4) +
           al256(slots * cand_cap) + 2 * al256(slots * 4) + al256((size_t)num_images * 4);
}

static UnionWs union_ws(void *base, int cand_cap, int num_images, int K) {
    const size_t slots = (size_t)num_images * K;
    UnionWs w;
    char *p = (char *)base;
    w.cand = (float *)p;
    p += al256(slots * cand_cap * 5 * sizeof(float));
    w.cls_dets = (float *)p;
    p += al256(slots * cand_cap * 5 * sizeof(float));
    w.order = (int32_t *)p;
    p += al256(slots * cand_cap * 4);
    w.keep = (uint8_t *)p;
    p += al256(slots * cand_cap);
    char *c0 = p;
    w.cand_count = (int32_t *)p;
    p += al256(slots * 4);
    w.cls_count = (int32_t *)p;
    p += al256(slots * 4);
    w.status = (int32_t *)p;
    p += al256((size_t)num_images * 4);
    w.counter_bytes = (size_t)(p - c0);
    return w;
}

__global__ __launch_bounds__(1024) void union_add_view_kernel(
    const float *__restrict__ rois, const float *__restrict__ cls_prob,
    const float *__restrict__ bbox_pred, const int32_t *__restrict__ roi_count, int R_cap, int K,
    const float *__restrict__ im_scale, const int32_t *__restrict__ im_hw, int hflip,
    int use_x_inv, float x_inv, float score_thresh, float4 bbox_w, int cand_cap, UnionWs ws) {
    __shared__ int scratch[32];
    __shared__ float wts[4];
    const int j = blockIdx.x + 1, img = blockIdx.y;
    const size_t slot = (size_t)img * K + j;
    const int rc = roi_count[img];
    if (rc < 0) {  // proposal selection failed in this view: the image fails
        if (threadIdx.x == 0) ws.status[img] = -1;
        return;
    }
    const int R = min(rc, R_cap);
    const int base = ws.cand_count[slot];
    if (threadIdx.x == 0) {
        wts[0] = bbox_w.x;
        wts[1] = bbox_w.y;
        wts[2] = bbox_w.z;
        wts[3] = bbox_w.w;
    }
    const float *prob = cls_prob + (size_t)img * R_cap * K;
    const float *pred = bbox_pred + (size_t)img * R_cap * 4 * K;
    const float *ri = rois + (size_t)img * R_cap * 5;
    const float scale = im_scale[img];
    const float hm1 = (float)(im_hw[img * 2 + 0] - 1), wm1 = (float)(im_hw[img * 2 + 1] - 1);
    const float fw = (float)im_hw[img * 2 + 1];
    float *c = ws.cand + slot * 5 * (size_t)cand_cap;
    __syncthreads();
    const int m = block_compact(
        R, [&](int r) { return prob[(size_t)r * K + j] >= score_thresh; },
        [&](int pos, int r) {
            const int q = base + pos;
            if (q >= cand_cap) return;
            const float *rb = ri + (size_t)r * 5;
            const float bx1 = rb[1] / scale, by1 = rb[2] / scale;
            const float bx2 = rb[3] / scale, by2 = rb[4] / scale;
            float x1, y1, x2, y2;
            decode_box_w(bx1, by1, bx2, by2, pred + (size_t)r * 4 * K + 4 * j, wts, x1, y1, x2,
                         y2);
            x1 = fmaxf(fminf(x1, wm1), 0.f);
            y1 = fmaxf(fminf(y1, hm1), 0.f);
            x2 = fmaxf(fminf(x2, wm1), 0.f);
            y2 = fmaxf(fminf(y2, hm1), 0.f);
            if (hflip) {  // flip_boxes: im_width - boxes[:, 2::4] - 1 in float32
                const float f1 = (fw - x2) - 1.0f, f2 = (fw - x1) - 1.0f;
                x1 = f1;
                x2 = f2;
            }
            if (use_x_inv) {  // aspect_ratio(boxes, 1.0 / ar): float32 times the float
                x1 = x1 * x_inv;
                x2 = x2 * x_inv;
            }
            c[q] = x1;
            c[(size_t)cand_cap + q] = y1;
            c[2 * (size_t)cand_cap + q] = x2;
            c[3 * (size_t)cand_cap + q] = y2;
            c[4 * (size_t)cand_cap + q] = prob[(size_t)r * K + j];
        },
        scratch);
    if (threadIdx.x == 0) {
        if (base + m > cand_cap) {
            ws.status[img] = -1;
            ws.cand_count[slot] = cand_cap;
        } else {
            ws.cand_count[slot] = base + m;
        }
    }
}

// LDS of the NMS phase of union_nms_kernel (the sort's keys and the soft-NMS
// copy overlay it).
struct UnionLds {
    float bx1[kUnionBlock], by1[kUnionBlock], bx2[kUnionBlock], by2[kUnionBlock],
        bar[kUnionBlock];  // the block in processing order
    float cx1[kUnionBlock], cy1[kUnionBlock], cx2[kUnionBlock], cy2[kUnionBlock],
        car[kUnionBlock];  // its boxes no earlier survivor suppresses, compacted
    float tx1[kUnionBlock], ty1[kUnionBlock], tx2[kUnionBlock], ty2[kUnionBlock],
        tar[kUnionBlock];  // a tile of the earlier survivors
    int bidx[kUnionBlock], cidx[kUnionBlock];  // rows of cand
    uint64_t mask[kUnionBlock * (kUnionBlock / 64)];
    uint8_t alive[kUnionBlock], keep_rank[kUnionBlock];
};

static constexpr size_t kUnionStatic = 256;  // the kernel's static LDS (scratch)
static_assert(sizeof(UnionLds) + kUnionStatic <= VD_LDS_BYTES, "NMS phase exceeds LDS");
static_assert((size_t)kUnionCandMax * 8 + kUnionStatic <= VD_LDS_BYTES, "sort keys exceed LDS");
static_assert((size_t)kSoftMax * 21 + kUnionStatic <= VD_LDS_BYTES, "soft-NMS copy exceeds LDS");

static size_t union_lds_bytes(int cand_cap, bool soft) {
    size_t b = sizeof(UnionLds);
    const size_t keys = (size_t)next_pow2(cand_cap < 64 ? 64 : cand_cap) * 8;
    if (keys > b) b = keys;
    if (soft && (size_t)cand_cap * 21 + 16 > b) b = (size_t)cand_cap * 21 + 16;
    return b;
}

__global__ __launch_bounds__(1024) void union_nms_kernel(int cand_cap, int K, float nms_thresh,
                                                         DetOpts opt, UnionWs ws) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    __shared__ int scratch[32];
    const int j = blockIdx.x + 1, img = blockIdx.y;
    const size_t slot = (size_t)img * K + j;
    if (ws.status[img] < 0) return;  // det_limit_kernel writes the image's -1
    const int n = min(ws.cand_count[slot], cand_cap);
    const float *c = ws.cand + slot * 5 * (size_t)cand_cap;
    const float *gx1 = c, *gy1 = c + cand_cap, *gx2 = c + 2 * (size_t)cand_cap,
                *gy2 = c + 3 * (size_t)cand_cap, *gsc = c + 4 * (size_t)cand_cap;
    float *dst = ws.cls_dets + slot * 5 * (size_t)cand_cap;
    if (n == 0) {
        if (threadIdx.x == 0) ws.cls_count[slot] = 0;
        return;
    }
    int kept;
    if (opt.soft_method >= 0) {
        // soft-NMS on a copy in LDS (n <= kSoftMax by the launcher); the
        // candidates in global memory stay box_voting's all_dets
        float *x1 = reinterpret_cast<float *>(lds_raw);
        float *y1 = x1 + n, *x2 = y1 + n, *y2 = x2 + n, *s = y2 + n;
        uint8_t *rem = reinterpret_cast<uint8_t *>(s + n);
        for (int t = threadIdx.x; t < n; t += blockDim.x) {
            x1[t] = gx1[t];
            y1[t] = gy1[t];
            x2[t] = gx2[t];
            y2[t] = gy2[t];
            s[t] = gsc[t];
        }
        __syncthreads();
        if (wave_id() == 0) {
            const int N = soft_nms_wave(x1, y1, x2, y2, s, rem, nullptr, n, nms_thresh, opt);
            if (lane_id() == 0) scratch[16] = N;
        }
        __syncthreads();
        kept = scratch[16];
        for (int u = threadIdx.x; u < kept; u += blockDim.x) {
            float row[5] = {x1[u], y1[u], x2[u], y2[u], s[u]};
            if (opt.vote_method >= 0) vote_box<7>(gx1, gy1, gx2, gy2, gsc, n, opt, row);
            for (int k = 0; k < 5; ++k) dst[u * 5 + k] = row[k];
        }
        if (threadIdx.x == 0) ws.cls_count[slot] = kept;
        return;
    }
    int32_t *order = ws.order + slot * (size_t)cand_cap;
    uint8_t *keep = ws.keep + slot * (size_t)cand_cap;
    {
        uint64_t *keys = reinterpret_cast<uint64_t *>(lds_raw);
        const int np2 = next_pow2(n);
        for (int t = threadIdx.x; t < np2; t += blockDim.x)
            keys[t] = t < n ? ((uint64_t)float_key(gsc[t]) << 32) | (uint32_t)t : 0ull;
        __syncthreads();
        if (n > 1) bitonic_sort_desc(keys, np2);
        for (int rk = threadIdx.x; rk < n; rk += blockDim.x) {
            order[rk] = (int)(uint32_t)keys[rk];
            keep[rk] = 0;
        }
        __threadfence_block();
        __syncthreads();
    }
    UnionLds &L = *reinterpret_cast<UnionLds *>(lds_raw);
    // the survivors so far, in processing order (the planes overlay the class's
    // result rows, which are written only after the last block)
    float *sx1 = dst, *sy1 = dst + cand_cap, *sx2 = dst + 2 * (size_t)cand_cap,
          *sy2 = dst + 3 * (size_t)cand_cap, *sar = dst + 4 * (size_t)cand_cap;
    int S = 0;
    const int box = threadIdx.x & (kUnionBlock - 1), half = threadIdx.x / kUnionBlock;
    for (int b0 = 0; b0 < n; b0 += kUnionBlock) {
        const int bm = min(kUnionBlock, n - b0);
        for (int t = threadIdx.x; t < bm; t += blockDim.x) {
            const int i = order[b0 + t];
            const float a = gx1[i], b = gy1[i], cc = gx2[i], e = gy2[i];
            L.bx1[t] = a;
            L.by1[t] = b;
            L.bx2[t] = cc;
            L.by2[t] = e;
            L.bar[t] = (cc - a + 1) * (e - b + 1);
            L.bidx[t] = i;
            L.alive[t] = 1;
        }
        __syncthreads();
        // against the survivors of the earlier blocks: thread (box, half) tests
        // its box against one half of each tile
        for (int s0 = 0; s0 < S; s0 += kUnionBlock) {
            const int tm = min(kUnionBlock, S - s0);
            for (int t = threadIdx.x; t < tm; t += blockDim.x) {
                L.tx1[t] = sx1[s0 + t];
                L.ty1[t] = sy1[s0 + t];
                L.tx2[t] = sx2[s0 + t];
                L.ty2[t] = sy2[s0 + t];
                L.tar[t] = sar[s0 + t];
            }
            __syncthreads();
            if (box < bm && L.alive[box]) {
                const float jx1 = L.bx1[box], jy1 = L.by1[box], jx2 = L.bx2[box],
                            jy2 = L.by2[box], ja = L.bar[box];
                const int h = (tm + 1) / 2;
                const int u0 = half ? h : 0, u1 = half ? tm : h;
                bool dead = false;
                for (int u = u0; u < u1 && !dead; ++u)
                    dead = suppresses(L.tx1[u], L.ty1[u], L.tx2[u], L.ty2[u], L.tar[u], jx1, jy1,
                                      jx2, jy2, ja, nms_thresh);
                if (dead) L.alive[box] = 0;
            }
            __syncthreads();
        }
        const int m2 = block_compact(
            bm, [&](int t) { return L.alive[t] != 0; },
            [&](int u, int t) {
                L.cx1[u] = L.bx1[t];
                L.cy1[u] = L.by1[t];
                L.cx2[u] = L.bx2[t];
                L.cy2[u] = L.by2[t];
                L.car[u] = L.bar[t];
                L.cidx[u] = L.bidx[t];
            },
            scratch);
        nms_build_mask_rows(L.cx1, L.cy1, L.cx2, L.cy2, L.car, m2, nms_thresh, L.mask, wave_id(),
                            num_waves());
        __syncthreads();
        if (wave_id() == 0) nms_resolve_wave(L.mask, m2, L.keep_rank);
        __syncthreads();
        const int k2 = block_compact(
            m2, [&](int u) { return L.keep_rank[u] != 0; },
            [&](int v, int u) {
                sx1[S + v] = L.cx1[u];
                sy1[S + v] = L.cy1[u];
                sx2[S + v] = L.cx2[u];
                sy2[S + v] = L.cy2[u];
                sar[S + v] = L.car[u];
                keep[L.cidx[u]] = 1;
            },
            scratch);
        S += k2;
        __threadfence_block();
        __syncthreads();
    }
    // survivors ascending by vstack index -> the class's rows
    kept = block_compact(
        n, [&](int t) { return keep[t] != 0; },
        [&](int u, int t) { order[u] = t; }, scratch);
    __threadfence_block();
    __syncthreads();
    for (int u = threadIdx.x; u < kept; u += blockDim.x) {
        const int t = order[u];
        float row[5] = {gx1[t], gy1[t], gx2[t], gy2[t], gsc[t]};
        if (opt.vote_method >= 0) vote_box<7>(gx1, gy1, gx2, gy2, gsc, n, opt, row);
        for (int k = 0; k < 5; ++k) dst[u * 5 + k] = row[k];
    }
    if (threadIdx.x == 0) ws.cls_count[slot] = kept;
}

static bool union_args_ok(int cand_cap, int num_images, int K) {
    return K >= 2 && K <= 1024 && num_images >= 1 && cand_cap >= 1;
}

int launch_box_union_add_view(const float *rois, const float *cls_prob, const float *bbox_pred,
                              const int32_t *roi_count, int R_cap, int num_images, int K,
                              const float *im_scale, const int32_t *im_hw, int hflip,
                              int use_x_inv, float x_inv, int first, float score_thresh,
                              const float *bbox_weights, int cand_cap, void *workspace,
                              size_t ws_bytes, hipStream_t s) {
    if (!union_args_ok(cand_cap, num_images, K) || R_cap < 1) return VD_ERR_ARG;
    if (use_x_inv && !(x_inv > 0.f && x_inv < INFINITY)) return VD_ERR_ARG;
    if (cand_cap > kUnionCandMax) return VD_ERR_SHAPE;
    if (!workspace || ws_bytes < box_union_workspace_bytes(cand_cap, num_images, K))
        return VD_ERR_WORKSPACE;
    UnionWs ws = union_ws(workspace, cand_cap, num_images, K);
    if (first) {
        const int st = zero_async(ws.cand_count, ws.counter_bytes, s);
        if (st != VD_OK) return st;
    }
    const float4 bw = make_float4(bbox_weights[0], bbox_weights[1], bbox_weights[2], bbox_weights[3]);
    hipLaunchKernelGGL(union_add_view_kernel, dim3(K - 1, num_images), dim3(1024), 0, s, rois,
                       cls_prob, bbox_pred, roi_count, R_cap, K, im_scale, im_hw, hflip ? 1 : 0,
                       use_x_inv ? 1 : 0, x_inv, score_thresh, bw, cand_cap, ws);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

int launch_box_union_detections(int cand_cap, int num_images, int K, float nms_thresh,
                                int dets_per_im, int soft_method, float soft_sigma, float soft_min,
                                int vote_method, float vote_th, float vote_beta, int det_cap,
                                float *dets_out, int32_t *det_cls_out, int32_t *det_count_out,
                                int32_t *cand_max_out, void *workspace, size_t ws_bytes,
                                hipStream_t s) {
    if (!union_args_ok(cand_cap, num_images, K) || det_cap < 1) return VD_ERR_ARG;
    if (soft_method < -1 || soft_method > 2 || vote_method < -1 || vote_method > 3)
        return VD_ERR_ARG;
    if (cand_cap > kUnionCandMax || (soft_method >= 0 && cand_cap > kSoftMax)) return VD_ERR_SHAPE;
    if (!workspace || ws_bytes < box_union_workspace_bytes(cand_cap, num_images, K))
        return VD_ERR_WORKSPACE;
    UnionWs ws = union_ws(workspace, cand_cap, num_images, K);
    hipLaunchKernelGGL(union_nms_kernel, dim3(K - 1, num_images), dim3(1024),
                       union_lds_bytes(cand_cap, soft_method >= 0), s, cand_cap, K, nms_thresh,
                       DetOpts{soft_method, soft_sigma, soft_min, vote_method, vote_th, vote_beta},
                       ws);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    if (cand_max_out) {
        const hipError_t e = hipMemcpyAsync(cand_max_out, ws.cand_count,
                                            (size_t)num_images * K * sizeof(int32_t),
                                            hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return VD_ERR_LAUNCH;
    }
    DetWs dw{ws.cls_dets, ws.cls_count, nullptr};
    return launch_det_limit(ws.status, cand_cap, num_images, K, dets_per_im, det_cap, dw, dets_out,
                            det_cls_out, det_count_out, s);
}

}  // namespace vd
