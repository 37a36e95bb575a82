// Box post-processing building blocks (device code) shared by the single-view
// kernels (detections.hip) and the test-time-augmentation union (box_union.hip):
// the box decode of im_detect_bbox, the compiled .pyx overlap arithmetic,
// cython_nms.soft_nms by one wave, box_voting's sums in numpy's order, and the
// per-class workspace that det_limit_kernel reads.
#pragma once

#include "nms_block.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr double kClip = 4.135166556742356;  // np.log(1000. / 16.)
static constexpr int kSoftMax = 4096;  // rows of a soft-NMS (its boxes live in LDS)

__host__ __device__ inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

struct DetWs {
    float *cls_dets;     // [img][K][R_cap][5]
    int32_t *cls_count;  // [img][K]
    uint64_t *mask;      // [img][K][R_cap*words]
};

// The detections limit over the per-class rows of ws (det_limit_kernel,
// detections.hip): status[img] < 0 marks a failed image (count -1).
int launch_det_limit(const int32_t *status, int R_cap, int num_images, int K, int dets_per_im,
                     int det_cap, DetWs ws, float *dets_out, int32_t *det_cls_out,
                     int32_t *det_count_out, hipStream_t s);

__device__ __forceinline__ void decode_box_w(float bx1, float by1, float bx2, float by2,
                                             const float *d, const float *wts, float &x1,
                                             float &y1, float &x2, float &y2) {
    const float widths = bx2 - bx1 + 1.0f;
    const float heights = by2 - by1 + 1.0f;
    const float ctr_x = bx1 + 0.5f * widths;
    const float ctr_y = by1 + 0.5f * heights;
    const float dx = d[0] / wts[0], dy = d[1] / wts[1];
    const double dw = fmin((double)(d[2] / wts[2]), kClip);
    const double dh = fmin((double)(d[3] / wts[3]), kClip);
    const float pcx = dx * widths + ctr_x;
    const float pcy = dy * heights + ctr_y;
    const double pw = fmax(exp(dw) * (double)widths, 1.0);
    const double ph = fmax(exp(dh) * (double)heights, 1.0);
    x1 = (float)((double)pcx - 0.5 * pw);
    y1 = (float)((double)pcy - 0.5 * ph);
    x2 = (float)((double)pcx + 0.5 * pw - 1.0);
    y2 = (float)((double)pcy + 0.5 * ph - 1.0);
}

// TEST.SOFT_NMS / TEST.BBOX_VOTE (lib/core/test.py:756-776).
struct DetOpts {
    int soft_method;  // -1: cython NMS; 0 hard, 1 linear, 2 gaussian (cython_nms.soft_nms)
    float soft_sigma, soft_min;  // sigma, score_thresh (0.0001 at test.py:760)
    int vote_method;  // -1 off; 0 ID, 1 AVG, 2 IOU_AVG, 3 QUASI_SUM (boxes.py:277-333)
    float vote_th, vote_beta;
};

// The compiled .pyx arithmetic (cython_nms.soft_nms :166-171, cython_bbox.bbox_overlaps):
// Cython emits the literal 1 of `x2 - x1 + 1` as 1.0, so each side is the float
// difference widened to double, products / sums in double, rounded to float on
// assignment; iw * ih is a float product; ov a float division.
__device__ __forceinline__ float cy_area(float x1, float y1, float x2, float y2) {
    return (float)(((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0));
}

// IoU of a kept / top box a with box b (area_b = cy_area(b)); false when they
// do not overlap (iw or ih <= 0: soft_nms leaves the box, bbox_overlaps 0).
__device__ __forceinline__ bool cy_iou(float ax1, float ay1, float ax2, float ay2, float bx1,
                                       float by1, float bx2, float by2, float area_b,
                                       float &ov) {
    const float iw = (float)((double)(fminf(ax2, bx2) - fmaxf(ax1, bx1)) + 1.0);
    if (!(iw > 0.f)) return false;
    const float ih = (float)((double)(fminf(ay2, by2) - fmaxf(ay1, by1)) + 1.0);
    if (!(ih > 0.f)) return false;
    const float inter = iw * ih;
    const float ua = (float)(((double)(ax2 - ax1) + 1.0) * ((double)(ay2 - ay1) + 1.0) +
                             (double)area_b - (double)inter);
    ov = inter / ua;
    return true;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// cython_nms.soft_nms (cython_nms.pyx:98-203) by one wave over the m boxes in
// (x1, y1, x2, y2, s), rearranged in place as the reference rearranges its copy:
// step i swaps the first maximum of s[i, N) to i; every later box that overlaps
// it is decayed (each box is decayed once per step wherever the sequential loop
// would meet it, so the decays run in parallel); a decayed score below soft_min
// removes the box by moving the current last box into its place and looking at
// that one again (the holes are filled in ascending order by the wave's lane 0).
// rem: LDS byte per position; ind (optional) follows the rows (the keep indices).
// Returns N, the boxes kept in [0, N).
__device__ inline int soft_nms_wave(float *x1, float *y1, float *x2, float *y2, float *s,
                                    uint8_t *rem, int *ind, int m, float Nt, const DetOpts &o) {
    const int lane = lane_id();
    int N = m;
    for (int i = 0; i < N; ++i) {
        float best = -INFINITY;
        int bp = 0x7fffffff;
        for (int p = i + lane; p < N; p += VD_WAVE) {
            const float v = s[p];
            if (v > best) {
                best = v;
                bp = p;
            }
        }
        for (int off = VD_WAVE / 2; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int op = __shfl_xor(bp, off);
            if (ob > best || (ob == best && op < bp)) {
                best = ob;
                bp = op;
            }
        }
        if (bp != i && lane == 0) {
            float t;
            t = x1[i]; x1[i] = x1[bp]; x1[bp] = t;
            t = y1[i]; y1[i] = y1[bp]; y1[bp] = t;
            t = x2[i]; x2[i] = x2[bp]; x2[bp] = t;
            t = y2[i]; y2[i] = y2[bp]; y2[bp] = t;
            t = s[i]; s[i] = s[bp]; s[bp] = t;
            if (ind) {
                const int k = ind[i];
                ind[i] = ind[bp];
                ind[bp] = k;
            }
        }
        wave_sync();
        const float tx1 = x1[i], ty1 = y1[i], tx2 = x2[i], ty2 = y2[i];
        for (int p = i + 1 + lane; p < N; p += VD_WAVE) {
            const float bx1 = x1[p], by1 = y1[p], bx2 = x2[p], by2 = y2[p];
            float ov;
            uint8_t r = 0;
            if (cy_iou(tx1, ty1, tx2, ty2, bx1, by1, bx2, by2, cy_area(bx1, by1, bx2, by2), ov)) {
                float w;
                if (o.soft_method == 1)
                    w = ov > Nt ? 1.f - ov : 1.f;
                else if (o.soft_method == 2)
                    w = (float)exp((double)((-(ov * ov)) / o.soft_sigma));
                else
                    w = ov > Nt ? 0.f : 1.f;
                const float ns = w * s[p];
                s[p] = ns;
                r = ns < o.soft_min;
            }
            rem[p] = r;
        }
        wave_sync();
        for (int base = i + 1; base < N; base += VD_WAVE) {
            const int p = base + lane;
            uint64_t mask = ballot(p < N && rem[p]);
            while (mask) {
                const int q = base + __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
                if (q >= N) break;
                for (;;) {  // boxes[q] = boxes[N-1]; N -= 1; look at q again
                    const int last = N - 1;
                    if (lane == 0 && last != q) {
                        x1[q] = x1[last];
                        y1[q] = y1[last];
                        x2[q] = x2[last];
                        y2[q] = y2[last];
                        s[q] = s[last];
                        rem[q] = rem[last];
                        if (ind) ind[q] = ind[last];
                    }
                    N = last;
                    wave_sync();
                    if (q >= N || !rem[q]) break;
                }
            }
        }
    }
    return N;
}

// box_voting's sums for one top box, in numpy's order: the voters (rows of the
// class's candidates with bbox_overlaps >= vote_th, ascending) stream by; the
// weighted box sums run sequentially down the rows (a (n,4) axis-0 reduction),
// the 1-D sums (weights, weight * overlap, overlap) in numpy's pairwise order.
struct VoteAcc {
    float w, wo, o;
};

__device__ __forceinline__ VoteAcc va_add(VoteAcc a, VoteAcc b) {
    return {a.w + b.w, a.wo + b.wo, a.o + b.o};
}

struct VoteStream {
    const float *x1, *y1, *x2, *y2, *s;
    int cur;
    float tx1, ty1, tx2, ty2, th;
    float c0, c1, c2, c3;
    __device__ float overlap(int i) const {
        float ov;
        return cy_iou(tx1, ty1, tx2, ty2, x1[i], y1[i], x2[i], y2[i],
                      cy_area(x1[i], y1[i], x2[i], y2[i]), ov) ? ov : 0.f;
    }
    __device__ VoteAcc next() {  // the caller asks for exactly the counted voters
        for (;; ++cur) {
            const float ov = overlap(cur);
            if (ov >= th) {
                const int i = cur++;
                const float w = s[i];
                c0 = c0 + x1[i] * w;
                c1 = c1 + y1[i] * w;
                c2 = c2 + x2[i] * w;
                c3 = c3 + y2[i] * w;
                return {w, w * ov, ov};
            }
        }
    }
};

// numpy pairwise_sum (loops_utils.h): < 8 sequential from 0; <= 128 eight strided
// accumulators ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) then the tail; else halves at
// a multiple of 8.  D bounds the recursion (n <= 128 << D).
template <int D>
__device__ VoteAcc pw_sum(VoteStream &st, int n) {
    if (n < 8) {
        VoteAcc r = {0.f, 0.f, 0.f};
        for (int i = 0; i < n; ++i) r = va_add(r, st.next());
        return r;
    }
    if constexpr (D > 0) {
        if (n > 128) {
            int n2 = n / 2;
            n2 -= n2 % 8;
            const VoteAcc a = pw_sum<D - 1>(st, n2);
            const VoteAcc b = pw_sum<D - 1>(st, n - n2);
            return va_add(a, b);
        }
    }
    VoteAcc r[8];
    for (int k = 0; k < 8; ++k) r[k] = st.next();
    int i = 8;
    for (; i < n - n % 8; i += 8)
        for (int k = 0; k < 8; ++k) r[k] = va_add(r[k], st.next());
    VoteAcc res = va_add(va_add(va_add(r[0], r[1]), va_add(r[2], r[3])),
                         va_add(va_add(r[4], r[5]), va_add(r[6], r[7])));
    for (; i < n; ++i) res = va_add(res, st.next());
    return res;
}

// box_voting (boxes.py:277-333) of one top row against the m candidates.  D as
// pw_sum's: 5 covers m <= 4096 (the single-view kernels), 7 the union's 16384.
template <int D = 5>
__device__ inline void vote_box(const float *x1, const float *y1, const float *x2,
                                const float *y2, const float *s, int m, const DetOpts &o,
                                float *row) {
    VoteStream st{x1, y1, x2, y2, s, 0, row[0], row[1], row[2], row[3], o.vote_th,
                  0.f, 0.f, 0.f, 0.f};
    int n = 0;
    for (int i = 0; i < m; ++i) n += st.overlap(i) >= o.vote_th;
    if (n == 0) return;  // numpy raises (weights sum to zero); never for a top row itself
    const VoteAcc sum = pw_sum<D>(st, n);
    const float scl = 0.f + sum.w;
    row[0] = st.c0 / scl;
    row[1] = st.c1 / scl;
    row[2] = st.c2 / scl;
    row[3] = st.c3 / scl;
    if (o.vote_method == 1)
        row[4] = scl / (float)n;
    else if (o.vote_method == 2)
        row[4] = (0.f + sum.wo) / (0.f + sum.o);
    else if (o.vote_method == 3)
        row[4] = scl / (float)pow((double)n, (double)o.vote_beta);
}

}  // namespace vd
