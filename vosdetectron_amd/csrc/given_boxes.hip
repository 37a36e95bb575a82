// The front of im_detect_bbox for caller-given boxes (MODEL.FASTER_RCNN False):
// _get_rois_blob (lib/core/test.py:877-906) and the DEDUP_BOXES hash with np.unique
// (test.py:132-139), for every frame of a step in one launch (vd_rois_from_boxes), and
// the gather that maps the box head's rows back onto the caller's rows
// (test.py:186-189, vd_gather_rows).
//
// rois_from_boxes_kernel (one workgroup per frame): row r forms its RoI
// (f, float32(float64(box) * im_scale)) and its hash -- float32 products with
// DEDUP_BOXES, rintf (half to even, np.round), then the float64 terms 1, 1e3, 1e6,
// 1e9, 1e12 summed left to right.  Every term and partial sum is an integer below
// 2^53 for blobs under 16000 pixels, so the sum is np.dot's whatever its order.  The
// (hash, row) keys are sorted ascending in LDS by a bitonic network, the hash as an
// orderable uint64 (-0 folded onto +0, which np.unique compares equal), so equal
// hashes lie together lowest row first: np.unique's first occurrence.  Positions past
// the count hold the largest key (above +inf) and stay at the end.  Run heads are
// flagged, a workgroup scan numbers the runs, and index / inv_index / rois are
// written from that numbering.
//
// The keys are two LDS arrays (uint64 hash, int32 row), not one 16-byte record: 48 KiB
// instead of 64.  By the bank rule (not measured): for a partner distance >= 32 each
// 32-lane half of a wave reads 32 consecutive 8-byte words, one 256-byte bank row, which
// ds_read_b64 should serve without a conflict; shorter distances read two such rows,
// which should be 2-way.
#include "common.hpp"
#include "vosdet_internal.hpp"

namespace vd {

namespace {

constexpr int kGivenThreads = 1024;
constexpr int kGivenPer = kGivenBoxesCap / kGivenThreads;  // scan positions per thread
constexpr int kGivenMaxF = 65535;                          // gather: gridDim.y

struct GivenLds {
    uint64_t key[kGivenBoxesCap];
    int32_t row[kGivenBoxesCap];
    int scratch[16];
};
static_assert(sizeof(GivenLds) <= 64 * 1024 && sizeof(GivenLds) <= VD_LDS_BYTES,
              "vd_rois_from_boxes: the sort keys must fit static LDS");
static_assert(kGivenPer * kGivenThreads == kGivenBoxesCap && kGivenThreads / VD_WAVE <= 16,
              "vd_rois_from_boxes: the scan covers the capacity with <= 16 waves");

// unsigned comparison of keys == numeric comparison of the doubles; -0.0 -> +0.0
__device__ __forceinline__ uint64_t double_key(double d) {
    uint64_t u = (uint64_t)__double_as_longlong(d);
    if (u == 0x8000000000000000ull) u = 0ull;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

struct GivenRoi {
    float x1, y1, x2, y2;
};

// _project_im_rois: float64 product, stored as float32 (test.py:890, :904)
__device__ __forceinline__ GivenRoi given_roi(const float *__restrict__ b, double sc) {
    GivenRoi r;
    r.x1 = (float)((double)b[0] * sc);
    r.y1 = (float)((double)b[1] * sc);
    r.x2 = (float)((double)b[2] * sc);
    r.y2 = (float)((double)b[3] * sc);
    return r;
}

__device__ __forceinline__ void store_roi(float *__restrict__ o, int f, const GivenRoi &r) {
    o[0] = (float)f;
    o[1] = r.x1;
    o[2] = r.y1;
    o[3] = r.x2;
    o[4] = r.y2;
}

__global__ __launch_bounds__(kGivenThreads) void rois_from_boxes_kernel(
    const float *__restrict__ boxes, const int32_t *__restrict__ counts,
    const double *__restrict__ im_scale, float dedup, int cap, float *__restrict__ rois,
    int32_t *__restrict__ ucounts, int32_t *__restrict__ index, int32_t *__restrict__ inv_index) {
    __shared__ GivenLds lds;
    const int f = blockIdx.x, t = threadIdx.x;
    const int n = counts[f];
    if (n <= 0 || n > cap) {  // uniform.  A negative count is an upstream failure code: kept
        if (t == 0) ucounts[f] = n > cap ? VD_COUNT_SELECT_FAILED : n;
        return;
    }
    const double sc = im_scale[f];
    const float *fb = boxes + (int64_t)f * cap * 4;
    float *fr = rois + (int64_t)f * cap * 5;
    int32_t *fi = index + (int64_t)f * cap, *fv = inv_index + (int64_t)f * cap;
    if (!(dedup > 0.f)) {  // cfg.DEDUP_BOXES > 0 is the reference's condition
        for (int r = t; r < n; r += kGivenThreads) {
            store_roi(fr + (int64_t)r * 5, f, given_roi(fb + r * 4, sc));
            fi[r] = r;
            fv[r] = r;
        }
        if (t == 0) ucounts[f] = n;
        return;
    }
    const int P = next_pow2(n);  // <= kGivenBoxesCap: n <= cap <= kGivenBoxesCap
    const float q0 = rintf((float)f * dedup);
    for (int r = t; r < P; r += kGivenThreads) {
        uint64_t k = ~0ull;  // padding: above every hash, +inf included
        if (r < n) {
            const GivenRoi g = given_roi(fb + r * 4, sc);
            double h = (double)q0;
            h = h + (double)rintf(g.x1 * dedup) * 1e3;
            h = h + (double)rintf(g.y1 * dedup) * 1e6;
            h = h + (double)rintf(g.x2 * dedup) * 1e9;
            h = h + (double)rintf(g.y2 * dedup) * 1e12;
            k = double_key(h);
        }
        lds.key[r] = k;
        lds.row[r] = r;  // padding rows r >= n: above every real row
    }
    __syncthreads();
    // ascending bitonic network over P keys; thread p of a stage owns the pair
    // (i, i + j) with i = p's bits with a 0 inserted at bit log2(j)
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < (P >> 1); p += kGivenThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int x = i + j;
                const uint64_t a = lds.key[i], b = lds.key[x];
                const int32_t ra = lds.row[i], rb = lds.row[x];
                const bool gt = a > b || (a == b && ra > rb);
                const bool asc = (i & k) == 0;
                if (gt == asc && (a != b || ra != rb)) {
                    lds.key[i] = b;
                    lds.key[x] = a;
                    lds.row[i] = rb;
                    lds.row[x] = ra;
                }
            }
            __syncthreads();
        }
    }
    // run heads, numbered by a workgroup scan: thread t owns positions [4t, 4t + 4)
    const int p0 = t * kGivenPer;
    bool head[kGivenPer];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < kGivenPer; ++e) {
        const int p = p0 + e;
        head[e] = p < n && (p == 0 || lds.key[p] != lds.key[p - 1]);
        mine += head[e] ? 1 : 0;
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < VD_WAVE; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane_id() >= o) incl += v;
    }
    if (lane_id() == VD_WAVE - 1) lds.scratch[wave_id()] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
    for (int w = 0; w < kGivenThreads / VD_WAVE; ++w) {
        const int c = lds.scratch[w];
        if (w < wave_id()) before += c;
        total += c;
    }
    int uid = before - 1;  // the run position p0 - 1 belongs to
#pragma unroll
    for (int e = 0; e < kGivenPer; ++e) {
        const int p = p0 + e;
        if (p >= n) break;
        const int r = lds.row[p];
        if (head[e]) {
            ++uid;
            fi[uid] = r;
            store_roi(fr + (int64_t)uid * 5, f, given_roi(fb + r * 4, sc));
        }
        fv[r] = uid;
    }
    if (t == 0) ucounts[f] = total;
}

// one wave per caller row: rows_per_block rows of one frame per workgroup
__global__ __launch_bounds__(256) void gather_rows_kernel(
    const float *__restrict__ boxes, const float *__restrict__ scores,
    const float *__restrict__ deltas, const int32_t *__restrict__ index,
    const int32_t *__restrict__ inv_index, const int32_t *__restrict__ counts,
    const int32_t *__restrict__ ucounts, int cap, int K, int D, float *__restrict__ rows_out,
    float *__restrict__ scores_out, float *__restrict__ deltas_out,
    int32_t *__restrict__ counts_out) {
    const int f = blockIdx.y;
    const int n = counts[f], u = ucounts[f];
    const bool ok = u >= 0 && n <= cap;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        counts_out[f] = u < 0 ? u : (n > cap ? VD_COUNT_SELECT_FAILED : n);
    const int i = blockIdx.x * (256 / VD_WAVE) + wave_id();
    if (!ok || i >= n) return;
    const int j = inv_index[(int64_t)f * cap + i];
    if (j < 0 || j >= u || j >= cap) return;  // not an index vd_rois_from_boxes wrote
    const int b = index[(int64_t)f * cap + j];  // boxes[index][inv_index], test.py:139, :189
    if (b < 0 || b >= n) return;
    const int64_t src = (int64_t)f * cap + j, dst = (int64_t)f * cap + i;
    const int lane = lane_id();
    if (lane < 5)
        rows_out[dst * 5 + lane] = lane == 0 ? (float)f : boxes[((int64_t)f * cap + b) * 4 + lane - 1];
    for (int c = lane; c < K; c += VD_WAVE) scores_out[dst * K + c] = scores[src * K + c];
    for (int c = lane; c < D; c += VD_WAVE) deltas_out[dst * D + c] = deltas[src * D + c];
}

}  // namespace

size_t rois_from_boxes_workspace_bytes(int F, int cap) {
    (void)F;
    (void)cap;
    return 0;  // the keys live in LDS
}

int launch_rois_from_boxes(const float *boxes, const int32_t *counts, const double *im_scale,
                           float dedup, int F, int cap, float *rois, int32_t *ucounts,
                           int32_t *index, int32_t *inv_index, hipStream_t s) {
    if (F < 1 || cap < 1 || cap > kGivenBoxesCap) return VD_ERR_SHAPE;
    hipLaunchKernelGGL(rois_from_boxes_kernel, dim3(F), dim3(kGivenThreads), 0, s, boxes, counts,
                       im_scale, dedup, cap, rois, ucounts, index, inv_index);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

int launch_gather_rows(const float *boxes, const float *scores, const float *deltas,
                       const int32_t *index, const int32_t *inv_index, const int32_t *counts,
                       const int32_t *ucounts, int F, int cap, int K, int D, float *rows_out,
                       float *scores_out, float *deltas_out, int32_t *counts_out, hipStream_t s) {
    if (F < 1 || F > kGivenMaxF || cap < 1 || cap > kGivenBoxesCap || K < 1 || D < 1)
        return VD_ERR_SHAPE;
    const int per = 256 / VD_WAVE;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((cap + per - 1) / per, F), dim3(256), 0, s, boxes,
                       scores, deltas, index, inv_index, counts, ucounts, cap, K, D, rows_out,
                       scores_out, deltas_out, counts_out);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
