// viz_mask_result's object-ID maps on the device (vd_label_maps).
//
// Reference: lib/utils/vis.py:119-157 viz_mask_result, called per frame from the
// VOS online loop (lib_vos/tools/train_davis_online.py:596-600): every
// detection's decoded H x W plane is painted in ascending score order
// (outImg[mask > 0] = class), detections with score < thresh skipped; rtv_gt is the
// same painting restricted to score > rvt_cls_threshold.
//
// Painting n planes costs n x H x W evaluations and writes.  Here the order is
// turned round: the value of a pixel is the id of the covering detection that
// the reference paints LAST, so each pixel walks the detections from the last
// painted to the first and stops at its first hit.
//
// label_prep_kernel (one workgroup per frame): the frame's first mask row
// (prefix sum of the clamped counts, on the device), which detections are
// painted, their rank in descending priority (score, then row index: among equal
// scores the higher index is painted later and wins), and each one's paste
// geometry (paste_geom) -- written into the workspace in rank order.
//
// label_paint_kernel (one workgroup per kTileW x kTileH tile of a frame): collects,
// in rank order, the detections whose clipped box meets the tile, then for each
// stages its (R+2)^2 padded mask in LDS (load_padded) and lets every still
// undecided pixel inside the box evaluate paste_pixel -- the value vd_paste_masks
// writes, bit for bit.  The workgroup leaves the loop once all its pixels are
// decided.  gt is the winner's id where its score exceeds gt_thresh: the winner
// has the highest score of all detections covering the pixel, so this equals the
// reference's second painting.  A lane owns one column of the tile, so a wave
// stores 64 consecutive bytes of a row.
#include "common.hpp"
#include "paste_geom.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr int kLabelMaxCap = 1024;  // detections per frame (LDS rank / candidate lists)
static constexpr int kLabelMaxF = 65535;   // gridDim.z
static constexpr int kTileW = 64, kTileH = 32;
static constexpr int kLabelThreads = 256;
static constexpr int kRowsPerThread = kTileH / (kLabelThreads / kTileW);  // 8
static constexpr size_t kLabelHeadBytes = 256;  // per-launch header granularity

struct LabelEntry {  // one painted detection, in rank order
    PasteGeom g;
    int32_t mrow;    // its row of `masks`
    int32_t id;      // written id | (gt ? 0x100 : 0)
};

__host__ __device__ inline size_t label_head_bytes(int F) {
    return ((size_t)F * sizeof(int32_t) + kLabelHeadBytes - 1) / kLabelHeadBytes * kLabelHeadBytes;
}

size_t label_maps_workspace_bytes(int F, int cap) {
    if (F < 1 || cap < 1 || cap > kLabelMaxCap || F > kLabelMaxF) return 0;
    return label_head_bytes(F) + (size_t)F * cap * sizeof(LabelEntry);
}

__device__ __forceinline__ int clamp_count(int n, int cap) { return min(max(n, 0), cap); }

__global__ __launch_bounds__(kLabelThreads) void label_prep_kernel(
    const float *__restrict__ dets, const int32_t *__restrict__ classes,
    const int32_t *__restrict__ counts, const uint8_t *__restrict__ valid, int F, int cap, int R,
    int im_h, int im_w, float score_thresh, float gt_thresh, const uint8_t *__restrict__ lut,
    int lut_n, int32_t *__restrict__ npaint, LabelEntry *__restrict__ entries) {
    __shared__ uint32_t key[kLabelMaxCap];  // float_key(score) of a painted row, 0 otherwise
    __shared__ int scratch[16];
    const int f = blockIdx.x, t = threadIdx.x;
    // first mask row of this frame: the sum of the (clamped) counts before it
    int part = 0;
    for (int j = t; j < f; j += kLabelThreads) part += clamp_count(counts[j], cap);
    const int base = block_sum(part, scratch);
    const int n = clamp_count(counts[f], cap);
    const float *fd = dets + (int64_t)f * cap * 5;
    int painted = 0;
    for (int i = t; i < n; i += kLabelThreads) {
        const float s = fd[i * 5 + 4];
        const bool p = (!valid || valid[(int64_t)f * cap + i] != 0) && !(s < score_thresh);
        // 0 marks a row that is not painted; float_key is 0 only for the all-ones NaN
        // pattern, which is folded onto its neighbour
        key[i] = p ? max(float_key(s), 1u) : 0u;
        painted += p;
    }
    __syncthreads();
    const int total = block_sum(painted, scratch);
    if (t == 0) npaint[f] = total;
    LabelEntry *fe = entries + (int64_t)f * cap;
    for (int i = t; i < n; i += kLabelThreads) {
        const uint32_t k = key[i];
        if (k == 0u) continue;
        int rank = 0;  // painted rows of higher priority
        for (int j = 0; j < n; ++j) {
            const uint32_t kj = key[j];
            rank += (kj > k) || (kj == k && j > i);
        }
        const float s = fd[i * 5 + 4];
        const int c = classes[(int64_t)f * cap + i];
        int id = 0;
        if (lut) {
            if (c >= 0 && c < lut_n) id = lut[c];
        } else if (c >= 0 && c <= 255) {
            id = c;
        }
        LabelEntry e;
        e.g = paste_geom(fd + i * 5, R, im_h, im_w);
        e.mrow = base + i;
        e.id = id | ((s > gt_thresh) ? 0x100 : 0);
        fe[rank] = e;
    }
}

__global__ __launch_bounds__(kLabelThreads) void label_paint_kernel(
    const float *__restrict__ masks, int R, int cap, int im_h, int im_w, float bin_thresh,
    const int32_t *__restrict__ npaint, const LabelEntry *__restrict__ entries,
    uint8_t *__restrict__ label, uint8_t *__restrict__ gt) {
    __shared__ float pm[(kPasteMaxR + 2) * (kPasteMaxR + 2)];
    __shared__ uint16_t cand[kLabelMaxCap];
    __shared__ int wtot[16];
    const int f = blockIdx.z, t = threadIdx.x;
    const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
    const int tx1 = min(tx0 + kTileW, im_w), ty1 = min(ty0 + kTileH, im_h);
    const int n = min(npaint[f], cap);
    const LabelEntry *fe = entries + (int64_t)f * cap;

    // candidates: the painted detections whose clipped box meets the tile, rank order kept
    const int ncand = block_compact(
        n,
        [&](int i) {
            const PasteGeom &g = fe[i].g;
            return g.x_1 > g.x_0 && g.y_1 > g.y_0 && g.x_0 < tx1 && g.x_1 > tx0 && g.y_0 < ty1 &&
                   g.y_1 > ty0;
        },
        [&](int pos, int i) { cand[pos] = (uint16_t)i; }, wtot);

    const int x = tx0 + (t & (kTileW - 1));
    const int yofs = ty0 + t / kTileW;  // rows yofs + k * (kLabelThreads / kTileW)
    constexpr int kStep = kLabelThreads / kTileW;
    uint32_t undecided = 0;
    if (x < im_w)
        for (int k = 0; k < kRowsPerThread; ++k)
            if (yofs + k * kStep < im_h) undecided |= 1u << k;
    uint32_t lab[kRowsPerThread], gtv[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) lab[k] = gtv[k] = 0;

    for (int ci = 0; ci < ncand; ++ci) {
        if (!__syncthreads_or(undecided != 0)) break;  // also: pm is free to overwrite
        const LabelEntry &e = fe[cand[ci]];
        load_padded(pm, masks + (int64_t)e.mrow * R * R, R);
        __syncthreads();
        const PasteGeom g = e.g;
        if (undecided == 0 || x < g.x_0 || x >= g.x_1) continue;
        const PasteCol c = paste_col(g, x);
        const uint32_t id = (uint32_t)e.id & 0xffu, gid = (e.id & 0x100) ? id : 0u;
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            const int y = yofs + k * kStep;
            if (!((undecided >> k) & 1u) || y < g.y_0 || y >= g.y_1) continue;
            if (paste_pixel(pm, g, paste_row(g, y), c, x, y, bin_thresh)) {
                lab[k] = id;
                gtv[k] = gid;
                undecided &= ~(1u << k);
            }
        }
    }

    if (x < im_w) {
        const int64_t plane = (int64_t)f * im_h * im_w;
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            const int y = yofs + k * kStep;
            if (y >= im_h) continue;
            const int64_t o = plane + (int64_t)y * im_w + x;
            label[o] = (uint8_t)lab[k];
            if (gt) gt[o] = (uint8_t)gtv[k];
        }
    }
}

int launch_label_maps(const float *masks, int R, const float *dets, const int32_t *classes,
                      const int32_t *counts, const uint8_t *valid, int F, int cap, int im_h,
                      int im_w, float bin_thresh, float score_thresh, float gt_thresh,
                      const uint8_t *lut, int lut_n, uint8_t *label, uint8_t *gt, void *workspace,
                      size_t workspace_bytes, hipStream_t s) {
    if (R < 1 || R > kPasteMaxR || im_h < 1 || im_w < 1 || cap < 1 || cap > kLabelMaxCap ||
        F > kLabelMaxF)
        return VD_ERR_SHAPE;
    const int64_t tiles_y = ((int64_t)im_h + kTileH - 1) / kTileH;
    if (tiles_y > 65535) return VD_ERR_SHAPE;
    if (workspace_bytes < label_maps_workspace_bytes(F, cap)) return VD_ERR_WORKSPACE;
    if (!workspace || ((uintptr_t)workspace & 15u)) return VD_ERR_ARG;
    int32_t *npaint = (int32_t *)workspace;
    LabelEntry *entries = (LabelEntry *)((char *)workspace + label_head_bytes(F));
    hipLaunchKernelGGL(label_prep_kernel, dim3(F), dim3(kLabelThreads), 0, s, dets, classes, counts,
                       valid, F, cap, R, im_h, im_w, score_thresh, gt_thresh, lut, lut_n, npaint,
                       entries);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    const dim3 grid((im_w + kTileW - 1) / kTileW, (unsigned)tiles_y, F);
    hipLaunchKernelGGL(label_paint_kernel, grid, dim3(kLabelThreads), 0, s, masks, R, cap, im_h,
                       im_w, bin_thresh, npaint, entries, label, gt);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
