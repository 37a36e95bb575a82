// Optical flow as read from a .flo file -> the five level flows FlowAlign warps by.
//
// Reference: im_detect_all(model, im, flo) takes the flow at frame resolution;
// flo_to_blob (lib/utils/blob.py:63-75) resizes it with prep_im_for_blob's
// cv2.resize(fx = fy = im_scale, INTER_LINEAR), multiplies the values by the
// scale (`flo[0] * flo_scale`: a float32 array times a Python list, which numpy
// computes in float64; the blob assignment rounds once to float32), zero-pads
// to FPN.COARSEST_STRIDE and transposes to NCHW.  Each FlowAlign module then
// runs conv_flow_downsample over that blob (lib_vos/vos_model/flow_align/
// modules/flow_align.py:12-25): a frozen 2 -> 2 convolution, kernel = stride =
// k, diagonal weight (1/k)^3, for k = 64, 32, 16, 8, 4 -- five passes over the
// same tensor to form scaled block sums.
//
// Here one launch reads the raw flow (F x H x W x 2, u then v per pixel) once
// and writes every level (and, when asked, the blob itself):
//
//   blob(f,c,y,x) = float(double(R(f,y,x,c)) * im_scale)   y < Hr, x < Wr
//                 = 0                                        elsewhere
//   out_k(f,c,Y,X) = (1/k)^3 * sum of blob over the k x k block
//
// R is the resize of vd_image_resize_to_blob on float input: the identity at
// im_scale == 1, OpenCV's 2 x 2 INTER_AREA fast path at exactly 0.5 (a full
// block ((a + b) + c) + d times 0.25f, a partial block at an odd edge the sum of
// the taps inside over their count), else the scalar float INTER_LINEAR
//   f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s   (scale = 1/im_scale, double)
//   columns: s < 0 -> (0, 0); s >= W-1 -> (W-1, 0);  rows: taps clamped, f kept
//   D = S[s] * (1 - f) + S[s+1] * f  horizontally, then D0 * (1 - fy) + D1 * fy,
// every product and sum rounded as written (-ffp-contract=off).
//
// One workgroup of 256 threads owns one 64 x 64 blob tile of one frame, so Hp
// and Wp must be multiples of 64.  The summation order is fixed:
//
//   S4  thread (by, bx) forms its own 4 x 4 block: each row ((p0 + p1) + p2) + p3,
//       then the four row sums ((r0 + r1) + r2) + r3;
//   S8  = (S4[2Y][2X] + S4[2Y][2X+1]) + (S4[2Y+1][2X] + S4[2Y+1][2X+1]) out of LDS;
//   S16, S32, S64 likewise from the next finer level;
//   out_k = S_k * (1/k)^3  (a power of two: exact).
//
// A block sum is therefore a function of the block's blob values alone: it does
// not depend on F, on which outputs are requested, or on the launch.  No
// workspace, no atomics, no host synchronisation.
#include "common.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr int kFlowTile = 64;

enum { kFlowIdentity = 0, kFlowArea2 = 1, kFlowLinear = 2 };

struct FlowTaps {
    int i0, i1;
    float w0, w1;
};

// VResizeLinear row taps: indices clamped, the coefficient kept
__device__ __forceinline__ FlowTaps flow_row_taps(int y, double scale, int H) {
    float f = (float)((y + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    FlowTaps t;
    t.i0 = min(max(s, 0), H - 1);
    t.i1 = min(max(s + 1, 0), H - 1);
    t.w0 = 1.f - f;
    t.w1 = f;
    return t;
}

// HResizeLinear column taps (cv::resize's coefficient table)
__device__ __forceinline__ FlowTaps flow_col_taps(int x, double scale, int W) {
    float f = (float)((x + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= W - 1) { f = 0.f; s = W - 1; }
    FlowTaps t;
    t.i0 = s;
    t.i1 = min(s + 1, W - 1);
    t.w0 = 1.f - f;
    t.w1 = f;
    return t;
}

__device__ __forceinline__ float flow_area2(float a, float b, float c, float d) {
    return (((a + b) + c) + d) * 0.25f;
}

// One resized pixel (both channels) on the 2 x 2 area path
__device__ __forceinline__ float2 flow_area2_pixel(const float2 *__restrict__ frame, int H, int W,
                                                   int y, int x) {
    const int ys = 2 * y, xs = 2 * x;
    const float2 *p = frame + (int64_t)ys * W + xs;
    if (ys + 1 < H && xs + 1 < W) {
        const float2 a = p[0], b = p[1], c = p[W], d = p[W + 1];
        return make_float2(flow_area2(a.x, b.x, c.x, d.x), flow_area2(a.y, b.y, c.y, d.y));
    }
    float su = 0.f, sv = 0.f;
    int cnt = 0;
    for (int dy = 0; dy < 2 && ys + dy < H; ++dy)
        for (int dx = 0; dx < 2 && xs + dx < W; ++dx) {
            const float2 t = p[(int64_t)dy * W + dx];
            su += t.x;
            sv += t.y;
            ++cnt;
        }
    return make_float2(su / (float)cnt, sv / (float)cnt);
}

struct FlowLevels {
    float *p[5];  // strides 4, 8, 16, 32, 64; NULL = not wanted
};

__device__ __forceinline__ float flow_quad(const float *s, int pitch, int Y, int X) {
    const float *q = s + 2 * Y * pitch + 2 * X;
    return (q[0] + q[1]) + (q[pitch] + q[pitch + 1]);
}

template <int MODE>
__global__ __launch_bounds__(256) void flow_to_levels_kernel(
    const float *__restrict__ raw, int H, int W, double scale, double im_scale, int Hr, int Wr,
    int Hp, int Wp, int vec4, FlowLevels out, float *__restrict__ blob) {
    __shared__ float s4[2][16][16], s8[2][8][8], s16[2][4][4], s32[2][2][2];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int bx = tid & 15, by = tid >> 4;
    const int y0 = blockIdx.y * kFlowTile + by * 4, x0 = blockIdx.x * kFlowTile + bx * 4;
    const float2 *frame = reinterpret_cast<const float2 *>(raw) + (int64_t)f * H * W;

    float2 v[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = make_float2(0.f, 0.f);

    if (y0 < Hr && x0 < Wr) {
        if (MODE == kFlowIdentity) {
            if (vec4 && x0 + 3 < Wr) {  // (y * W + x0) is even: 16-byte aligned
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (y0 + r >= Hr) continue;
                    const float4 *p =
                        reinterpret_cast<const float4 *>(frame + (int64_t)(y0 + r) * W + x0);
                    const float4 a = p[0], b = p[1];
                    v[r][0] = make_float2(a.x, a.y);
                    v[r][1] = make_float2(a.z, a.w);
                    v[r][2] = make_float2(b.x, b.y);
                    v[r][3] = make_float2(b.z, b.w);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (y0 + r < Hr && x0 + c < Wr)
                            v[r][c] = frame[(int64_t)(y0 + r) * W + x0 + c];
            }
        } else if (MODE == kFlowArea2) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (y0 + r < Hr && x0 + c < Wr)
                        v[r][c] = flow_area2_pixel(frame, H, W, y0 + r, x0 + c);
        } else {
            FlowTaps tx[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) tx[c] = flow_col_taps(x0 + c, scale, W);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (y0 + r >= Hr) continue;
                const FlowTaps ty = flow_row_taps(y0 + r, scale, H);
                const float2 *row0 = frame + (int64_t)ty.i0 * W;
                const float2 *row1 = frame + (int64_t)ty.i1 * W;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (x0 + c >= Wr) continue;
                    const float2 a0 = row0[tx[c].i0], a1 = row0[tx[c].i1];
                    const float2 b0 = row1[tx[c].i0], b1 = row1[tx[c].i1];
                    const float du0 = a0.x * tx[c].w0 + a1.x * tx[c].w1;
                    const float du1 = b0.x * tx[c].w0 + b1.x * tx[c].w1;
                    const float dv0 = a0.y * tx[c].w0 + a1.y * tx[c].w1;
                    const float dv1 = b0.y * tx[c].w0 + b1.y * tx[c].w1;
                    v[r][c] = make_float2(du0 * ty.w0 + du1 * ty.w1, dv0 * ty.w0 + dv1 * ty.w1);
                }
            }
        }
        if (MODE != kFlowIdentity) {  // flo[0] * flo_scale in float64, one rounding
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    v[r][c].x = (float)((double)v[r][c].x * im_scale);
                    v[r][c].y = (float)((double)v[r][c].y * im_scale);
                }
        }
    }

    const int64_t plane = (int64_t)Hp * Wp;
    if (blob) {
        float *d = blob + (int64_t)f * 2 * plane + (int64_t)y0 * Wp + x0;  // 16-byte aligned
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            *reinterpret_cast<float4 *>(d + (int64_t)r * Wp) =
                make_float4(v[r][0].x, v[r][1].x, v[r][2].x, v[r][3].x);
            *reinterpret_cast<float4 *>(d + plane + (int64_t)r * Wp) =
                make_float4(v[r][0].y, v[r][1].y, v[r][2].y, v[r][3].y);
        }
    }

    float ru[4], rv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ru[r] = ((v[r][0].x + v[r][1].x) + v[r][2].x) + v[r][3].x;
        rv[r] = ((v[r][0].y + v[r][1].y) + v[r][2].y) + v[r][3].y;
    }
    const float su = ((ru[0] + ru[1]) + ru[2]) + ru[3];
    const float sv = ((rv[0] + rv[1]) + rv[2]) + rv[3];
    s4[0][by][bx] = su;
    s4[1][by][bx] = sv;

    // level sizes and this tile's origin in each level
    const int tY = blockIdx.y, tX = blockIdx.x;
    if (out.p[0]) {
        const int Hk = Hp / 4, Wk = Wp / 4;
        float *d = out.p[0] + ((int64_t)f * 2 * Hk + tY * 16 + by) * Wk + tX * 16 + bx;
        d[0] = su * (1.f / 64.f);
        d[(int64_t)Hk * Wk] = sv * (1.f / 64.f);
    }
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 6, Y = (tid >> 3) & 7, X = tid & 7;
        const float s = flow_quad(&s4[c][0][0], 16, Y, X);
        s8[c][Y][X] = s;
        if (out.p[1]) {
            const int Hk = Hp / 8, Wk = Wp / 8;
            out.p[1][(((int64_t)f * 2 + c) * Hk + tY * 8 + Y) * Wk + tX * 8 + X] =
                s * (1.f / 512.f);
        }
    }
    __syncthreads();
    if (tid < 32) {
        const int c = tid >> 4, Y = (tid >> 2) & 3, X = tid & 3;
        const float s = flow_quad(&s8[c][0][0], 8, Y, X);
        s16[c][Y][X] = s;
        if (out.p[2]) {
            const int Hk = Hp / 16, Wk = Wp / 16;
            out.p[2][(((int64_t)f * 2 + c) * Hk + tY * 4 + Y) * Wk + tX * 4 + X] =
                s * (1.f / 4096.f);
        }
    }
    __syncthreads();
    if (tid < 8) {
        const int c = tid >> 2, Y = (tid >> 1) & 1, X = tid & 1;
        const float s = flow_quad(&s16[c][0][0], 4, Y, X);
        s32[c][Y][X] = s;
        if (out.p[3]) {
            const int Hk = Hp / 32, Wk = Wp / 32;
            out.p[3][(((int64_t)f * 2 + c) * Hk + tY * 2 + Y) * Wk + tX * 2 + X] =
                s * (1.f / 32768.f);
        }
    }
    __syncthreads();
    if (tid < 2 && out.p[4]) {
        const int c = tid;
        const float s = flow_quad(&s32[c][0][0], 2, 0, 0);
        const int Hk = Hp / 64, Wk = Wp / 64;
        out.p[4][(((int64_t)f * 2 + c) * Hk + tY) * Wk + tX] = s * (1.f / 262144.f);
    }
}

int launch_flow_to_levels(const float *raw, int F, int H, int W, double im_scale, int Hr, int Wr,
                          int Hp, int Wp, float *const levels[5], float *blob, hipStream_t s) {
    if (!raw || F < 1 || H < 1 || W < 1 || !(im_scale > 0.0) || Hr < 1 || Wr < 1) return VD_ERR_ARG;
    if (Hp < Hr || Wp < Wr || Hp % kFlowTile || Wp % kFlowTile) return VD_ERR_SHAPE;
    if (F > 65535 || Hp / kFlowTile > 65535) return VD_ERR_SHAPE;
    if ((reinterpret_cast<uintptr_t>(raw) & 7) || (reinterpret_cast<uintptr_t>(blob) & 15))
        return VD_ERR_ARG;
    FlowLevels out;
    bool any = blob != nullptr;
    for (int i = 0; i < 5; ++i) {
        out.p[i] = levels[i];
        any = any || levels[i];
    }
    if (!any) return VD_OK;
    const double scale = 1.0 / im_scale;  // cv::resize: scale = 1 / inv_scale
    const dim3 grid(Wp / kFlowTile, Hp / kFlowTile, F), block(256);
    if (im_scale == 1.0) {
        if (Hr > H || Wr > W) return VD_ERR_SHAPE;
        const int vec4 = (W % 2 == 0) && !(reinterpret_cast<uintptr_t>(raw) & 15);
        hipLaunchKernelGGL(flow_to_levels_kernel<kFlowIdentity>, grid, block, 0, s, raw, H, W,
                           scale, im_scale, Hr, Wr, Hp, Wp, vec4, out, blob);
    } else if (scale == 2.0) {
        // every 2 x 2 block starts inside the frame
        if (Hr > (H + 1) / 2 || Wr > (W + 1) / 2) return VD_ERR_SHAPE;
        hipLaunchKernelGGL(flow_to_levels_kernel<kFlowArea2>, grid, block, 0, s, raw, H, W, scale,
                           im_scale, Hr, Wr, Hp, Wp, 0, out, blob);
    } else {  // tap indices are clamped to the frame
        hipLaunchKernelGGL(flow_to_levels_kernel<kFlowLinear>, grid, block, 0, s, raw, H, W, scale,
                           im_scale, Hr, Wr, Hp, Wp, 0, out, blob);
    }
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
