// nms_with_mask_iou (lib_vos/tools/vos_test.py:985-1029) for every frame of a
// step in one call (vd_mask_iou_nms_frames), straight from the class-selected
// R x R mask probabilities and the boxes: the H x W planes vd_paste_masks writes
// are never formed, and no count is read on the host.
//
// frames_prep_kernel (one workgroup per frame): the frame's first mask row (prefix
// sum of the clamped counts) and its count cut to the rows `masks` holds.
//
// frames_pack_kernel (one workgroup per detection): the (R+2)^2 padded mask sits in
// LDS (load_padded); a wave takes 64 consecutive columns of one row on the frame's
// 64-column grid, every lane evaluates paste_pixel (the byte vd_paste_masks writes,
// bit for bit) and the ballot is the packed word.  Only the words that meet the
// clipped box [x_0, x_1) x [y_0, y_1) are written; nothing else of a detection's
// bit rows is ever read, so the workspace needs no clearing.  The popcounts sum to
// the area.
//
// frames_inter_kernel (one workgroup per detection i, walking the pairs (i, j > i)
// of its frame): pairs whose clipped boxes are disjoint get 0 without touching the
// bit rows; the rest are listed in LDS and each wave takes one pair at a time,
// popcounts of the AND over the words of the boxes' common rectangle.  Words are
// aligned to the frame grid, so two detections' words AND directly.
//
// frames_greedy_kernel (one workgroup per frame): mask_nms_greedy, the pass
// vd_mask_iou_nms runs, then keep / valid / the previous-frame record.
#include "common.hpp"
#include "mask_nms_greedy.hpp"
#include "paste_geom.hpp"
#include "vosdet_internal.hpp"

namespace vd {

namespace {

constexpr int kFramesMaxF = 65535;  // gridDim.y
constexpr int kFramesThreads = 256;

struct FramesWs {
    int32_t *base;   // [F] first mask row of the frame
    int32_t *nf;     // [F] detections of the frame (cut to the mask rows)
    int4 *box;       // [rows] clipped box x_0, x_1, y_0, y_1
    int32_t *area;   // [rows]
    int32_t *inter;  // [F][cap][cap], i < j
    uint64_t *bits;  // [rows][im_h][wpr]
};

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline int words_per_row(int im_w) { return (im_w + 63) / 64; }

FramesWs carve_frames_ws(void *p, int F, int cap, int rows, int im_h, int im_w, size_t *total) {
    char *c = (char *)p;
    FramesWs w;
    size_t off = 0;
    w.base = (int32_t *)(c + off);
    off += align256((size_t)F * 4);
    w.nf = (int32_t *)(c + off);
    off += align256((size_t)F * 4);
    w.box = (int4 *)(c + off);
    off += align256((size_t)rows * 16);
    w.area = (int32_t *)(c + off);
    off += align256((size_t)rows * 4);
    w.inter = (int32_t *)(c + off);
    off += align256((size_t)F * cap * cap * 4);
    w.bits = (uint64_t *)(c + off);
    off += align256((size_t)rows * im_h * words_per_row(im_w) * 8);
    if (total) *total = off;
    return w;
}

bool frames_shape_ok(int F, int cap, int rows, int im_h, int im_w) {
    return F >= 1 && F <= kFramesMaxF && cap >= 1 && cap <= kMaxMaskNms && rows >= 0 &&
           im_h >= 1 && im_w >= 1 && (int64_t)im_h * im_w <= 0x7fffffffll &&
           (int64_t)im_h * words_per_row(im_w) <= 0x7fffffffll;
}

__global__ __launch_bounds__(kFramesThreads) void frames_prep_kernel(
    const int32_t *__restrict__ counts, int cap, int rows, FramesWs ws) {
    __shared__ int scratch[16];
    const int f = blockIdx.x, t = threadIdx.x;
    int64_t part = 0;
    for (int j = t; j < f; j += kFramesThreads) part += min(max(counts[j], 0), cap);
    // F * cap <= 65535 * 1024 < 2^31
    const int before = block_sum((int)part, scratch);
    const int n = min(max(counts[f], 0), cap);
    const int b0 = min(before, rows), b1 = min(before + n, rows);
    if (t == 0) {
        ws.base[f] = b0;
        ws.nf[f] = b1 - b0;
    }
}

__global__ __launch_bounds__(kFramesThreads) void frames_pack_kernel(
    const float *__restrict__ masks, int R, const float *__restrict__ dets, int cap, int im_h,
    int im_w, int wpr, float bin_thresh, FramesWs ws) {
    __shared__ float pm[(kPasteMaxR + 2) * (kPasteMaxR + 2)];
    __shared__ int scratch[16];
    const int f = blockIdx.y, i = blockIdx.x;
    if (i >= ws.nf[f]) return;  // uniform
    const int mrow = ws.base[f] + i;
    load_padded(pm, masks + (int64_t)mrow * R * R, R);
    __syncthreads();
    const PasteGeom g = paste_geom(dets + ((int64_t)f * cap + i) * 5, R, im_h, im_w);
    const int lane = lane_id(), nwv = num_waves();
    int cnt = 0;
    if (g.x_1 > g.x_0 && g.y_1 > g.y_0) {
        const int w0 = g.x_0 >> 6, w1 = (g.x_1 - 1) >> 6;
        uint64_t *rowbits = ws.bits + (int64_t)mrow * im_h * wpr;
        for (int w = w0; w <= w1; ++w) {  // a lane keeps its column's taps over the rows
            const int x = w * 64 + lane;
            const bool in = x >= g.x_0 && x < g.x_1;
            const PasteCol c = paste_col(g, in ? x : g.x_0);
            for (int y = g.y_0 + wave_id(); y < g.y_1; y += nwv) {
                const int v = in ? paste_pixel(pm, g, paste_row(g, y), c, x, y, bin_thresh) : 0;
                const uint64_t b = ballot(v != 0);
                if (lane == 0) {
                    rowbits[(int64_t)y * wpr + w] = b;
                    cnt += __popcll(b);
                }
            }
        }
    }
    const int area = block_sum(cnt, scratch);
    if (threadIdx.x == 0) {
        ws.box[mrow] = make_int4(g.x_0, g.x_1, g.y_0, g.y_1);
        ws.area[mrow] = area;
    }
}

__global__ __launch_bounds__(kFramesThreads) void frames_inter_kernel(int cap, int im_h, int wpr,
                                                                      FramesWs ws) {
    __shared__ uint16_t list[kMaxMaskNms];
    __shared__ int nlist;
    const int f = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
    const int n = ws.nf[f];
    if (i + 1 >= n) return;  // uniform: no pair (i, j > i)
    const int base = ws.base[f];
    const int4 bi = ws.box[base + i];
    int32_t *row = ws.inter + ((int64_t)f * cap + i) * cap;
    if (t == 0) nlist = 0;
    __syncthreads();
    for (int j = i + 1 + t; j < n; j += kFramesThreads) {
        const int4 bj = ws.box[base + j];
        // empty boxes (x_1 <= x_0 or y_1 <= y_0) fail this test against anything
        const bool meet = max(bi.x, bj.x) < min(bi.y, bj.y) && max(bi.z, bj.z) < min(bi.w, bj.w);
        if (meet)
            list[atomicAdd(&nlist, 1)] = (uint16_t)j;
        else
            row[j] = 0;
    }
    __syncthreads();
    const int lane = lane_id(), nl = nlist;
    const uint64_t *a = ws.bits + (int64_t)(base + i) * im_h * wpr;
    for (int k = wave_id(); k < nl; k += num_waves()) {
        const int j = list[k];
        const int4 bj = ws.box[base + j];
        const int x0 = max(bi.x, bj.x), x1 = min(bi.y, bj.y);
        const int y0 = max(bi.z, bj.z), y1 = min(bi.w, bj.w);
        const int w0 = x0 >> 6, nwd = ((x1 - 1) >> 6) - w0 + 1;
        const int total = (y1 - y0) * nwd;  // <= im_h * wpr
        const uint64_t *b = ws.bits + (int64_t)(base + j) * im_h * wpr;
        int sum = 0;
        for (int e = lane; e < total; e += VD_WAVE) {
            const int yy = e / nwd, ww = e - yy * nwd;
            const int64_t o = (int64_t)(y0 + yy) * wpr + w0 + ww;
            sum += __popcll(a[o] & b[o]);
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) row[j] = sum;
    }
}

__global__ __launch_bounds__(kMaxMaskNms) void frames_greedy_kernel(
    const float *__restrict__ dets, const int32_t *__restrict__ classes,
    const int32_t *__restrict__ counts, int cap, double iou_th, int max_per_class, FramesWs ws,
    int32_t *__restrict__ keep, int32_t *__restrict__ keep_counts, uint8_t *__restrict__ valid,
    float *__restrict__ prev_dets, int32_t *__restrict__ prev_classes,
    int32_t *__restrict__ prev_counts, int prev_cap) {
    __shared__ int order[kMaxMaskNms];  // position -> detection
    __shared__ int disc[kMaxMaskNms];   // by position; afterwards: kept, by detection
    __shared__ int sel[kMaxMaskNms];    // by position: kept and under the class cap
    __shared__ int outl[kMaxMaskNms];   // output position -> detection
    const int f = blockIdx.x, t = threadIdx.x;
    // A frame an upstream kernel failed keeps its code: propagate, never hide.
    const int c0 = counts[f];
    if (c0 < 0) {  // uniform
        if (t == 0) {
            keep_counts[f] = c0;
            if (prev_counts) prev_counts[f] = 0;
        }
        return;
    }
    const int n = ws.nf[f], base = ws.base[f];
    const float *fd = dets + (int64_t)f * cap * 5;
    const int32_t *fc = classes + (int64_t)f * cap;
    const int32_t *inter = ws.inter + (int64_t)f * cap * cap;
    const int nsel = mask_nms_greedy(
        n, [&](int d) { return fd[d * 5 + 4]; }, [&](int d) { return fc[d]; },
        [&](int d) { return ws.area[base + d]; },
        [&](int i, int j) { return inter[(int64_t)i * cap + j]; }, iou_th, max_per_class, order,
        disc, sel, [&](int pos, int d) { outl[pos] = d; });
    __syncthreads();
    if (valid) {
        for (int i = t; i < n; i += blockDim.x) disc[i] = 0;
        __syncthreads();
        for (int pos = t; pos < nsel; pos += blockDim.x) disc[outl[pos]] = 1;
        __syncthreads();
        for (int i = t; i < n; i += blockDim.x) valid[(int64_t)f * cap + i] = (uint8_t)disc[i];
    }
    for (int pos = t; pos < nsel; pos += blockDim.x) {
        const int d = outl[pos];
        keep[(int64_t)f * cap + pos] = d;
        if (prev_dets) {  // prev_cap >= cap >= nsel
            float *o = prev_dets + ((int64_t)f * prev_cap + pos) * 5;
            for (int k = 0; k < 5; ++k) o[k] = fd[d * 5 + k];
            prev_classes[(int64_t)f * prev_cap + pos] = fc[d];
        }
    }
    if (t == 0) {
        keep_counts[f] = nsel;
        if (prev_counts) prev_counts[f] = nsel;
    }
}

}  // namespace

size_t mask_iou_nms_frames_workspace_bytes(int F, int cap, int rows, int im_h, int im_w) {
    if (!frames_shape_ok(F, cap, rows, im_h, im_w)) return 0;
    size_t total = 0;
    carve_frames_ws(nullptr, F, cap, rows, im_h, im_w, &total);
    return total;
}

int launch_mask_iou_nms_frames(const float *masks, int rows, int R, const float *dets,
                               const int32_t *classes, const int32_t *counts, int F, int cap,
                               int im_h, int im_w, float bin_thresh, double iou_th,
                               int max_per_class, int32_t *keep, int32_t *keep_counts,
                               uint8_t *valid, float *prev_dets, int32_t *prev_classes,
                               int32_t *prev_counts, int prev_cap, void *workspace,
                               size_t workspace_bytes, hipStream_t s) {
    if (R < 1 || R > kPasteMaxR || !frames_shape_ok(F, cap, rows, im_h, im_w) ||
        (prev_dets && prev_cap < cap))
        return VD_ERR_SHAPE;
    size_t total = 0;
    const FramesWs w = carve_frames_ws(workspace, F, cap, rows, im_h, im_w, &total);
    if (workspace_bytes < total) return VD_ERR_WORKSPACE;
    if ((uintptr_t)workspace & 15u) return VD_ERR_ARG;
    const int wpr = words_per_row(im_w);
    hipLaunchKernelGGL(frames_prep_kernel, dim3(F), dim3(kFramesThreads), 0, s, counts, cap, rows,
                       w);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    const dim3 grid(cap, F);
    hipLaunchKernelGGL(frames_pack_kernel, grid, dim3(kFramesThreads), 0, s, masks, R, dets, cap,
                       im_h, im_w, wpr, bin_thresh, w);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    hipLaunchKernelGGL(frames_inter_kernel, grid, dim3(kFramesThreads), 0, s, cap, im_h, wpr, w);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    hipLaunchKernelGGL(frames_greedy_kernel, dim3(F), dim3(kMaxMaskNms), 0, s, dets, classes,
                       counts, cap, iou_th, max_per_class, w, keep, keep_counts, valid, prev_dets,
                       prev_classes, prev_counts, prev_cap);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
