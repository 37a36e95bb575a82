// keypoint_results' heatmap decode on the device.
//
// Reference: lib/utils/keypoints.py:103-157 heatmaps_to_keypoints (+ :214-222
// scores_to_probs), called per frame by lib/core/test.py:858-874: every RoI's
// K x M x M logit maps go to the host, are cv2.resize'd (INTER_CUBIC) to the
// box's own pixel size, softmaxed over space and argmaxed per keypoint.  Here
// the resized map never exists: one workgroup owns one (RoI, keypoint) map and
// walks the Wm x Hm destination in strips of 64 columns.
//
//   src  M x M logits in LDS (loaded once)
//   hz   M x 64: the horizontal pass of the strip (all M source rows)
//   vertical pass out of hz: lane = destination column, wave w takes rows
//   y = w, w + 4, ...; a lane computes the row taps of 64 of its wave's rows at
//   a time and the wave reads them back one row per iteration with
//   v_readlane (uniform operands), so a destination value costs 4 LDS reads,
//   4 multiplies and 3 adds.
//
// Each lane keeps (max, lowest linear index of the max) and a sum of
// exp(v - ref) in fp64 against a per-lane reference ref <= its running max that
// is only moved up when a value exceeds it by more than kKpRebase (so exp never
// overflows and the sum is rescaled a handful of times at most).  The block
// reduces the argmax first (wave butterfly, then the four waves in order; ties
// -> lowest index, np.argmax), rescales every lane's sum to that maximum and
// adds them in fp64 in a fixed butterfly order.  One launch, no workspace, no
// atomics; the launch geometry is fixed, so the result is a function of the
// inputs alone.
//
// The interpolation is OpenCV's INTER_CUBIC for float images restated
// (interpolateCubic with A = -0.75, HResizeCubic then VResizeCubic, replicated
// borders), every product and sum rounded as written (-ffp-contract=off):
//   scale = (double)M / Wm; f = (float)((d + 0.5) * scale - 0.5);
//   s = floor(f); t = f - s; taps s-1 .. s+2 clamped to [0, M-1];
//   c0 = ((A*(t+1) - 5A)*(t+1) + 8A)*(t+1) - 4A
//   c1 = ((A+2)*t - (A+3))*t*t + 1
//   c2 = ((A+2)*(1-t) - (A+3))*(1-t)*(1-t) + 1
//   c3 = 1 - c0 - c1 - c2
//   value = ((S0*c0 + S1*c1) + S2*c2) + S3*c3, rows first, then columns.
//
// The kernel is a template on what fills src: KpPlainMaps copies the map
// (vd_heatmaps_to_keypoints), KpAugMaps makes it from the TEST.KPS_AUG views
// (vd_heatmaps_to_keypoints_aug: im_detect_keypoints_aug's combination, lib/core/test.py:
// 567-730).  Everything after the fill is shared.
#include "common.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr int kKpMaxM = 64;      // heatmap side (LDS: M x M + M x 64 floats)
static constexpr int kKpMaxK = 32;
static constexpr int kKpStrip = 64;     // destination columns per pass: one lane each
static constexpr int kKpWaves = 4;
static constexpr int kKpMaxSide = 8192; // resized map side (the library's widest frame)
static constexpr float kKpRebase = 64.f;

struct CubicTaps {
    int i0, i1, i2, i3;
    float c0, c1, c2, c3;
};

__device__ __forceinline__ CubicTaps cubic_taps(int d, double scale, int M) {
    const float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    const int s = (int)fl;
    const float t = f - fl;
    const float A = -0.75f;
    const float t1 = t + 1.f, u = 1.f - t;
    CubicTaps k;
    k.c0 = ((A * t1 - 5.f * A) * t1 + 8.f * A) * t1 - 4.f * A;
    k.c1 = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    k.c2 = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
    k.c3 = 1.f - k.c0 - k.c1 - k.c2;
    k.i0 = min(max(s - 1, 0), M - 1);
    k.i1 = min(max(s, 0), M - 1);
    k.i2 = min(max(s + 1, 0), M - 1);
    k.i3 = min(max(s + 2, 0), M - 1);
    return k;
}

__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// later (v, i) replaces (bv, bi): larger value, or the same value at a lower index
__device__ __forceinline__ bool kp_better(float v, int i, float bv, int bi) {
    return v > bv || (v == bv && i < bi);
}

// The map a workgroup decodes: one R x K x M x M array read as it is.
struct KpPlainMaps {
    const float *maps;
    __device__ __forceinline__ void fill(float *src, int r, int k, int K, int M,
                                         const float *b) const {
        const float *m = maps + ((int64_t)r * K + k) * M * M;
        for (int i = threadIdx.x; i < M * M; i += blockDim.x) src[i] = m[i];
    }
};

// The map a workgroup decodes: im_detect_keypoints_aug's combination of V views
// (lib/core/test.py:567-651, 705-730), made while the map is loaded.  Per element the
// views are walked in heatmaps_ts order: a view the row's box area drops is skipped
// (combine_heatmaps_size_dep: area < area_th drops the ds views, area >= area_th the us
// views; area = (x2 - x1 + 1) * (y2 - y1 + 1) in float32, every operation rounded), a
// flipped view is read as flip_heatmaps inverts it (channel perm[k], column M - 1 - x),
// and the values fold as np.mean / np.amax over axis 0 do: the first kept value, then
// + or max in order, HM_AVG divided by float(T_row) (the float64 quotient of float32
// operands rounded to float32 is the correctly rounded float32 quotient).  Everything
// travels by value in the kernel arguments: no device-side pointer table.
struct KpAugMaps {
    const float *maps[VD_KPS_AUG_MAX_VIEWS];
    int8_t perm[kKpMaxK];
    uint32_t hflip, ds, us;
    int V, heur;
    float area_th;
    float *combined;  // R x K x M x M or nullptr
    __device__ __forceinline__ void fill(float *src, int r, int k, int K, int M,
                                         const float *b) const {
        uint32_t keep = V >= 32 ? 0xffffffffu : (1u << V) - 1u;
        if (area_th >= 0.f) {
            const float bw = b[2] - b[0] + 1.f, bh = b[3] - b[1] + 1.f;
            const float area = bw * bh;
            keep &= area < area_th ? ~ds : ~us;
        }
        const float T = (float)__popc(keep);
        const int64_t plain = ((int64_t)r * K + k) * M * M;
        const int64_t swapped = ((int64_t)r * K + perm[k]) * M * M;
        float *c = combined ? combined + plain : nullptr;
        for (int i = threadIdx.x; i < M * M; i += blockDim.x) {
            const int y = i / M, x = i - y * M;
            const int fi = y * M + (M - 1 - x);
            float acc = 0.f;
            bool any = false;
            for (int v = 0; v < V; ++v) {
                if (!((keep >> v) & 1u)) continue;
                const bool hf = (hflip >> v) & 1u;
                const float val = hf ? maps[v][swapped + fi] : maps[v][plain + i];
                if (!any)
                    acc = val;
                else
                    acc = heur == VD_KPS_AUG_HM_MAX ? fmaxf(acc, val) : acc + val;
                any = true;
            }
            if (heur == VD_KPS_AUG_HM_AVG) acc = (float)((double)acc / (double)T);
            src[i] = acc;
            if (c) c[i] = acc;
        }
    }
};

template <class Maps>
__global__ __launch_bounds__(kKpWaves * VD_WAVE) void heatmaps_to_keypoints_kernel(
    const Maps maps, int K, int M, const float *__restrict__ boxes,
    int box_stride, int min_size, float *__restrict__ out) {
    __shared__ float src[kKpMaxM * kKpMaxM];
    __shared__ float hz[kKpMaxM * kKpStrip];
    __shared__ float red_v[kKpWaves];
    __shared__ int red_i[kKpWaves];
    __shared__ double red_s[kKpWaves];
    const int r = blockIdx.x / K, k = blockIdx.x - r * K;
    const int lane = lane_id(), wv = wave_id();
    const float *b = boxes + (int64_t)r * box_stride;
    maps.fill(src, r, k, K, M, b);

    const float x1 = b[0], y1 = b[1];
    const float w = fmaxf(b[2] - x1, 1.f), h = fmaxf(b[3] - y1, 1.f);
    int Wm = (int)ceilf(w), Hm = (int)ceilf(h);
    if (min_size > 0) {
        Wm = max(Wm, min_size);
        Hm = max(Hm, min_size);
    }
    Wm = min(max(Wm, 1), kKpMaxSide);
    Hm = min(max(Hm, 1), kKpMaxSide);
    const double sx = (double)M / (double)Wm, sy = (double)M / (double)Hm;

    float bv = -INFINITY, mref = -INFINITY;
    int bi = 0x7fffffff;
    double sum = 0.;
    for (int xb = 0; xb < Wm; xb += kKpStrip) {
        const int x = xb + lane;
        const bool xin = x < Wm;
        const CubicTaps tx = cubic_taps(xin ? x : Wm - 1, sx, M);
        __syncthreads();  // src is loaded / the previous strip's hz has been read
        for (int rr = wv; rr < M; rr += kKpWaves) {
            const float *s = src + rr * M;
            hz[rr * kKpStrip + lane] = s[tx.i0] * tx.c0 + s[tx.i1] * tx.c1 + s[tx.i2] * tx.c2 +
                                       s[tx.i3] * tx.c3;
        }
        __syncthreads();
        // this wave's rows y = yb + kKpWaves * j, 64 at a time: lane j computes row j's taps
        for (int yb = wv; yb < Hm; yb += kKpWaves * VD_WAVE) {
            const CubicTaps ty = cubic_taps(min(yb + kKpWaves * lane, Hm - 1), sy, M);
            const int rows = ty.i0 | (ty.i1 << 6) | (ty.i2 << 12) | (ty.i3 << 18);
            const int nj = min(VD_WAVE, (Hm - yb + kKpWaves - 1) / kKpWaves);
            for (int j = 0; j < nj; ++j) {
                const float c0 = readlane_f(ty.c0, j), c1 = readlane_f(ty.c1, j);
                const float c2 = readlane_f(ty.c2, j), c3 = readlane_f(ty.c3, j);
                const int pk = __builtin_amdgcn_readlane(rows, j);
                if (!xin) continue;
                const float v = hz[(pk & 63) * kKpStrip + lane] * c0 +
                                hz[((pk >> 6) & 63) * kKpStrip + lane] * c1 +
                                hz[((pk >> 12) & 63) * kKpStrip + lane] * c2 +
                                hz[((pk >> 18) & 63) * kKpStrip + lane] * c3;
                const int idx = (yb + kKpWaves * j) * Wm + x;  // < 2^26
                if (kp_better(v, idx, bv, bi)) {
                    bv = v;
                    bi = idx;
                }
                float d = v - mref;
                if (d > kKpRebase) {  // first value (mref = -inf), or far above the reference
                    sum *= (double)expf(mref - v);
                    mref = v;
                    d = 0.f;
                }
                sum += (double)expf(d);
            }
        }
    }

    // argmax: wave butterfly, then the waves in order
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (kp_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        red_v[wv] = bv;
        red_i[wv] = bi;
    }
    __syncthreads();
    float gv = red_v[0];
    int gi = red_i[0];
    for (int q = 1; q < kKpWaves; ++q) {
        if (kp_better(red_v[q], red_i[q], gv, gi)) {
            gv = red_v[q];
            gi = red_i[q];
        }
    }
    // sum of exp(v - max): every lane's sum moved from its reference to the maximum
    // (a lane without values has sum 0 and reference -inf: 0 * exp(-inf) = 0)
    double s = sum * (double)expf(mref - gv);
    for (int o = 32; o > 0; o >>= 1)
        s += __longlong_as_double((long long)shfl_xor64((uint64_t)__double_as_longlong(s), o));
    if (lane == 0) red_s[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = red_s[0];
        for (int q = 1; q < kKpWaves; ++q) tot += red_s[q];
        const int yi = gi / Wm, xi = gi - yi * Wm;
        // fp64 quotient of fp32 operands rounded to fp32 = the correctly rounded fp32 quotient
        const float wc = (float)((double)w / (double)Wm), hc = (float)((double)h / (double)Hm);
        float *o = out + (int64_t)r * 4 * K + k;
        o[0] = (float)(((double)xi + 0.5) * (double)wc + (double)x1);
        o[K] = (float)(((double)yi + 0.5) * (double)hc + (double)y1);
        o[2 * K] = gv;
        o[3 * K] = 1.f / (float)tot;
    }
}

int launch_heatmaps_to_keypoints(const float *maps, int R, int K, int M, const float *boxes,
                                 int box_stride, int min_size, float *out, hipStream_t s) {
    if (R == 0) return VD_OK;
    if (M < 1 || M > kKpMaxM || K < 1 || K > kKpMaxK) return VD_ERR_SHAPE;
    if ((int64_t)R * K > 0x7fffffffll) return VD_ERR_SHAPE;
    hipLaunchKernelGGL(heatmaps_to_keypoints_kernel<KpPlainMaps>, dim3(R * K),
                       dim3(kKpWaves * VD_WAVE), 0, s, KpPlainMaps{maps}, K, M, boxes, box_stride,
                       min_size, out);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

int launch_heatmaps_to_keypoints_aug(const float *const *view_maps, int V, uint32_t hflip_mask,
                                     uint32_t ds_mask, uint32_t us_mask, const int32_t *flip_perm,
                                     int heur, float area_th, int R, int K, int M,
                                     const float *boxes, int box_stride, int min_size,
                                     float *combined_out, float *out, hipStream_t s) {
    if (R == 0) return VD_OK;
    if (M < 1 || M > kKpMaxM || K < 1 || K > kKpMaxK) return VD_ERR_SHAPE;
    if (V < 1 || V > VD_KPS_AUG_MAX_VIEWS) return VD_ERR_SHAPE;
    if ((int64_t)R * K > 0x7fffffffll) return VD_ERR_SHAPE;
    KpAugMaps a = {};
    for (int v = 0; v < V; ++v) a.maps[v] = view_maps[v];
    for (int k = 0; k < K; ++k) a.perm[k] = (int8_t)flip_perm[k];
    a.hflip = hflip_mask;
    a.ds = ds_mask;
    a.us = us_mask;
    a.V = V;
    a.heur = heur;
    a.area_th = area_th;
    a.combined = combined_out;
    hipLaunchKernelGGL(heatmaps_to_keypoints_kernel<KpAugMaps>, dim3(R * K),
                       dim3(kKpWaves * VD_WAVE), 0, s, a, K, M, boxes, box_stride, min_size, out);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
