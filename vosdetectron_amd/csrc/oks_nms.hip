// keypoint_results' OKS NMS on the device.
//
// Reference: lib/utils/keypoints.py:225-266 nms_oks / compute_oks, applied per
// frame at lib/core/test.py:864-870: a Python loop over numpy arrays on the host.
// Here all F frames of a step are handled by two stream-ordered launches with no
// host read (graph-capturable):
//
//   nms_oks_frames_kernel   one workgroup per frame
//     score   mean of the 17 logits in float32, numpy's pairwise order
//     rank    bitonic sort of (score, index) keys: descending score, the HIGHER
//             index first among equal scores (numpy's stable sort reversed, its
//             order for n <= 16; for n > 16 the reference's tie order is
//             unspecified and this one is ours).  NaN logits are unsupported.
//     stage   x / y of the frame's rows and the float32 box areas in LDS, in
//             processing order
//     mask    upper-triangular suppression bitmask: one wave ballot per (row,
//             64-column word), each lane the 17 double exps of one pair
//     resolve nms_block.hpp's greedy pass ("i suppresses j" only ever with i
//             before j: exactly the asymmetric use of i's box area)
//     keep    ordered compaction of the kept ranks -> frame-local indices
//   nms_oks_gather_kernel   one workgroup per frame: scans counts_out and copies
//             the kept rows of dets / classes / keyps, compacted, kept order
//
// compute_oks' arithmetic, every operation rounded as numpy 2 rounds it (float32
// until the division by the float64 vars; -ffp-contract=off):
//   area = (x2 - x1 + 1) * (y2 - y1 + 1)                 float32, row i's box only
//   d2   = fl32(fl32(dx * dx) + fl32(dy * dy))           float32
//   e_k  = ((double)d2 / vars[k]) / ((double)area + 2^-52) / 2
//   ovr  = (sum_k exp(-e_k)) / 17                        float64, pairwise order
//   j is dropped when ovr > thresh.
// numpy's pairwise order for 17 terms: r[j] = a[j] + a[8 + j] (j < 8),
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then + a[16].
#include "common.hpp"
#include "nms_block.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr int kOksK = 17;
static constexpr int kOksMaxD = 512;    // detections per frame (vd_detections_postfilter's cap)
static constexpr int kOksThreads = 512;
static constexpr int kOksWords = kOksMaxD / 64;

static_assert(kOksWords <= 64 * kNmsMaxWordsPerLane, "nms_resolve_wave holds the removed words");
static_assert(kOksMaxD <= kOksThreads, "one thread per row in the score phase");
static constexpr size_t kOksLdsBytes =
    2 * sizeof(float) * kOksMaxD * kOksK          // x, y
    + sizeof(float) * kOksMaxD                    // area
    + sizeof(uint64_t) * kOksMaxD                 // sort keys
    + sizeof(uint64_t) * kOksMaxD * kOksWords     // mask
    + sizeof(int) * kOksMaxD + kOksMaxD + 64;     // order, keep flags, scratch
static_assert(kOksLdsBytes <= VD_LDS_BYTES, "OKS NMS state exceeds the workgroup's LDS");

// keypoints.py:251-254: vars = (sigmas / 10.0 * 2) ** 2 in float64
constexpr double oks_var(double sigma) { return (sigma / 10.0 * 2) * (sigma / 10.0 * 2); }
__device__ const double kOksVars[kOksK] = {
    oks_var(.26), oks_var(.25), oks_var(.25), oks_var(.35), oks_var(.35), oks_var(.79),
    oks_var(.79), oks_var(.72), oks_var(.72), oks_var(.62), oks_var(.62), oks_var(1.07),
    oks_var(1.07), oks_var(.87), oks_var(.87), oks_var(.89), oks_var(.89)};

// numpy's pairwise sum of 17 terms (see the header)
template <class T>
__device__ __forceinline__ T pairwise17(const T *a) {
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j] + a[8 + j];
    return (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + a[16];
}

__device__ __forceinline__ float oks_area(const float *b) {
    return (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
}

// compute_oks of source row i (its x / y in registers, its area) against row j
__device__ __forceinline__ double oks_value(const float *ix, const float *iy, float area,
                                            const float *jx, const float *jy) {
    const double da = (double)area + 0x1p-52;  // np.spacing(1)
    double t[kOksK];
#pragma unroll
    for (int k = 0; k < kOksK; ++k) {
        const float dx = jx[k] - ix[k], dy = jy[k] - iy[k];
        const float d2 = dx * dx + dy * dy;
        t[k] = exp(-((double)d2 / kOksVars[k] / da * 0.5));
    }
    return pairwise17(t) / (double)kOksK;
}

// rows of keyps before frame f: the exclusive prefix sum of the non-negative counts
__device__ __forceinline__ int64_t oks_row_base(const int32_t *counts, int f) {
    int64_t b = 0;
    for (int g = 0; g < f; ++g) b += max(counts[g], 0);
    return b;
}

__global__ __launch_bounds__(kOksThreads) void nms_oks_frames_kernel(
    const float *__restrict__ keyps, int64_t rows, const float *__restrict__ dets,
    const int32_t *__restrict__ counts, int D, double thresh, int32_t *__restrict__ keep,
    int32_t *__restrict__ counts_out, float *__restrict__ scores_out) {
    __shared__ float xs[kOksMaxD * kOksK];
    __shared__ float ys[kOksMaxD * kOksK];
    __shared__ float area[kOksMaxD];
    __shared__ uint64_t keys[kOksMaxD];
    __shared__ uint64_t mask[kOksMaxD * kOksWords];
    __shared__ int order[kOksMaxD];
    __shared__ uint8_t kept[kOksMaxD];
    __shared__ int scratch[16];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int cnt = counts[f];
    const int64_t base = oks_row_base(counts, f);
    // a negative count is a failure code: passed on, the frame is empty.  Rows
    // past the keyps buffer are never read (such a frame is cut to the rows there)
    int n = min(max(cnt, 0), D);
    n = (int)min((int64_t)n, max(rows - base, (int64_t)0));
    const float *kp = keyps + base * 4 * kOksK;
    const float *fd = dets + (int64_t)f * D * 5;

    // score = np.mean(kp[i, 2, :]) in float32, and the sort keys
    const int np2 = next_pow2(max(n, 1));
    if (tid < np2) {
        uint64_t key = 0;
        if (tid < n) {
            float a[kOksK];
#pragma unroll
            for (int k = 0; k < kOksK; ++k) a[k] = kp[(int64_t)tid * 4 * kOksK + 2 * kOksK + k];
            const float sc = pairwise17(a) / (float)kOksK;
            if (scores_out) scores_out[(int64_t)f * D + tid] = sc;
            key = ((uint64_t)float_key(sc) << 32) | (uint32_t)tid;
        }
        keys[tid] = key;
    }
    if (scores_out)
        for (int i = n + tid; i < D; i += kOksThreads) scores_out[(int64_t)f * D + i] = 0.f;
    __syncthreads();
    bitonic_sort_desc(keys, np2);
    __syncthreads();

    // stage the rows in processing order
    if (tid < n) {
        const int src = (int)(uint32_t)keys[tid];
        order[tid] = src;
        area[tid] = oks_area(fd + (int64_t)src * 5);
    }
    for (int e = tid; e < n * 2 * kOksK; e += kOksThreads) {
        const int r = e / (2 * kOksK), c = e - r * 2 * kOksK;
        const int src = (int)(uint32_t)keys[r];
        const float v = kp[(int64_t)src * 4 * kOksK + c];  // rows 0 (x) and 1 (y) of [4, K]
        if (c < kOksK) xs[r * kOksK + c] = v;
        else ys[r * kOksK + c - kOksK] = v;
    }
    __syncthreads();

    // suppression bitmask: row i (kept candidate) against every later rank j
    const int words = (n + 63) >> 6;
    const int lane = lane_id();
    for (int i = wave_id(); i < n; i += kOksThreads / VD_WAVE) {
        float ix[kOksK], iy[kOksK];
#pragma unroll
        for (int k = 0; k < kOksK; ++k) {
            ix[k] = xs[i * kOksK + k];
            iy[k] = ys[i * kOksK + k];
        }
        const float ia = area[i];
        for (int w = i >> 6; w < words; ++w) {
            const int j = (w << 6) + lane;
            bool s = false;
            if (j > i && j < n)
                s = oks_value(ix, iy, ia, xs + j * kOksK, ys + j * kOksK) > thresh;
            const uint64_t b = ballot(s);
            if (lane == 0) mask[i * words + w] = b;
        }
    }
    __syncthreads();
    if (wave_id() == 0) nms_resolve_wave(mask, n, kept);
    __syncthreads();

    int32_t *fk = keep + (int64_t)f * D;
    const int nk = block_compact(
        n, [&](int r) { return kept[r] != 0; }, [&](int pos, int r) { fk[pos] = order[r]; },
        scratch);
    for (int i = nk + tid; i < D; i += kOksThreads) fk[i] = -1;
    if (tid == 0) counts_out[f] = cnt < 0 ? cnt : nk;
}

// The kept rows of every frame, compacted: dets_out / classes_out [F, D] in kept
// order (zeros past the count), keyps_out frame-major at the exclusive prefix sum
// of counts_out (zeros past the total).
__global__ __launch_bounds__(256) void nms_oks_gather_kernel(
    const float *__restrict__ keyps, int64_t rows, const float *__restrict__ dets,
    const int32_t *__restrict__ classes, const int32_t *__restrict__ counts, int F, int D,
    const int32_t *__restrict__ keep, const int32_t *__restrict__ counts_out,
    float *__restrict__ dets_out, int32_t *__restrict__ classes_out,
    float *__restrict__ keyps_out) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t in_base = oks_row_base(counts, f), out_base = oks_row_base(counts_out, f);
    const int nk = min(max(counts_out[f], 0), D);
    const int32_t *fk = keep + (int64_t)f * D;
    constexpr int RW = 4 * kOksK;
    for (int e = tid; e < D * 5; e += blockDim.x) {
        const int p = e / 5, c = e - p * 5;
        dets_out[(int64_t)f * D * 5 + e] = p < nk ? dets[((int64_t)f * D + fk[p]) * 5 + c] : 0.f;
    }
    for (int p = tid; p < D; p += blockDim.x)
        classes_out[(int64_t)f * D + p] = p < nk ? classes[(int64_t)f * D + fk[p]] : 0;
    for (int e = tid; e < nk * RW; e += blockDim.x) {
        const int p = e / RW, c = e - p * RW;
        keyps_out[(out_base + p) * RW + c] = keyps[(in_base + fk[p]) * RW + c];
    }
    if (f == F - 1)  // the last frame's workgroup clears the rows past the total
        for (int64_t e = (out_base + nk) * RW + tid; e < rows * RW; e += blockDim.x)
            keyps_out[e] = 0.f;
}

int launch_nms_oks_frames(const float *keyps, int64_t rows, int K, const float *dets,
                          const int32_t *classes, const int32_t *counts, int F, int D,
                          double thresh, int32_t *keep, int32_t *counts_out, float *dets_out,
                          int32_t *classes_out, float *keyps_out, float *scores_out,
                          hipStream_t s) {
    if (K != kOksK) return VD_ERR_ARG;
    if (D > kOksMaxD) return VD_ERR_SHAPE;
    if (F == 0) return VD_OK;
    hipLaunchKernelGGL(nms_oks_frames_kernel, dim3(F), dim3(kOksThreads), 0, s, keyps, rows, dets,
                       counts, D, thresh, keep, counts_out, scores_out);
    hipLaunchKernelGGL(nms_oks_gather_kernel, dim3(F), dim3(256), 0, s, keyps, rows, dets, classes,
                       counts, F, D, keep, counts_out, dets_out, classes_out, keyps_out);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

// compute_oks (keypoints.py:243-266) of one source row against N destination rows
__global__ __launch_bounds__(256) void compute_oks_kernel(const float *__restrict__ src_kp,
                                                          const float *__restrict__ src_roi,
                                                          const float *__restrict__ dst_kp, int N,
                                                          double *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    float ix[kOksK], iy[kOksK];
#pragma unroll
    for (int k = 0; k < kOksK; ++k) {
        ix[k] = src_kp[k];
        iy[k] = src_kp[kOksK + k];
    }
    const float *d = dst_kp + (int64_t)j * 4 * kOksK;
    out[j] = oks_value(ix, iy, oks_area(src_roi), d, d + kOksK);
}

int launch_compute_oks(const float *src_kp, const float *src_roi, const float *dst_kp, int N,
                       int K, double *out, hipStream_t s) {
    if (K != kOksK) return VD_ERR_ARG;
    if (N == 0) return VD_OK;
    hipLaunchKernelGGL(compute_oks_kernel, dim3((N + 255) / 256), dim3(256), 0, s, src_kp, src_roi,
                       dst_kp, N, out);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
