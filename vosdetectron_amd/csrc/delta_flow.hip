// The delta-flow head of Generalized_VOS_RCNN (MODEL.USE_DELTA_FLOW,
// lib_vos/vos_modeling/vos_model_builder.py:95-104, 314-326): the model makes its
// own flow from the change of a two-channel "flow feature" of every FPN level.
//
//   feat_i = tanh(conv3x3_i(P_i))           i = 0..4 on [P6..P2], C -> 2, no bias
//   d_i    = feat_i - previous feat_i       (nothing without a previous one)
//   data_flow = sum_i bilinear_up(d_i, 1/s_i) / s_i      s_i = 1/64 .. 1/4
//   level_j   = s_j^3 * (k_j x k_j block sums of data_flow)   (conv_flow_downsample)
//
// Two launches, neither reads a host value that changes from step to step.
//
// delta_flow_features_kernel (all levels and frames): one workgroup of 256
// threads owns a 16 x 16 tile of one frame of one level.
//   phase 1  every input pixel of the 18 x 18 halo tile gets its 18 partial dot
//            products over the C channels (9 taps x 2 outputs) into LDS: a 3x3
//            conv with two outputs is 18 1x1 convs whose results are shifted and
//            added, so the C-channel pixel is read once per tile and the 256-channel
//            input tile is never staged.  Halo ratio 324 / 256 = 1.27, the re-reads
//            served by L2.
//            NHWC (the product layout): 16 lanes share a pixel, each loads float4
//            channel groups 16 B apart from its neighbour (256 contiguous bytes per
//            pixel and pass), the weights ([18][C], staged in LDS) are read as
//            float4 and used for two pixels, and the 16 lanes' sums are added by
//            DPP row operations (no LDS traffic).  The loads of the next pixel
//            pair are in flight during the arithmetic of this one.  C % 64 == 0.
//            NCHW: one lane per pixel (coalesced along x), channels in a loop,
//            weights wave-uniform.
//   phase 2  thread (y, x) adds its nine shifted partials per output, tanh,
//            delta = valid[b] ? new - state : 0, state = new.  The thread that
//            writes a state element is the one that read it.
//
// delta_flow_to_levels_kernel: one workgroup per 64 x 64 blob tile of a frame,
// thread (by, bx) owns a 4 x 4 block (the structure of flow_prep.hip).  Of a
// level with stride k >= 8 the whole block interpolates inside one 2 x 2 source
// window, of the stride-4 level inside a 3 x 3 one, so a thread loads 25 source
// values per channel and not 320.  Per pixel, coarsest level first,
//   v = hy0 * (hx0 * s00 + hx1 * s01) + hy1 * (hx0 * s10 + hx1 * s11)
//   acc = acc + v * k                      (k = 1/s: a power of two, exact)
// with the align_corners=False source position max((dst + 0.5) / k - 0.5, 0),
// the upper tap clamped to the last row / column; all weights are exact.  Block
// sums: the thread's 4 x 4 pairwise ((p0+p1)+(p2+p3) per row, the rows likewise),
// then 2 x 2 of the next finer level out of LDS -- a value depends on its block
// alone.  No workspace, no atomics.
#include "common.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr int kDfTile = 16;                  // output tile side
static constexpr int kDfHalo = kDfTile + 2;         // 18
static constexpr int kDfHaloPix = kDfHalo * kDfHalo;  // 324
static constexpr int kDfTaps = 18;                  // 9 taps x 2 outputs

typedef float df_float2 __attribute__((ext_vector_type(2)));

// sum over the 16 lanes of a DPP row, in every lane of the row
__device__ __forceinline__ float row16_sum(float v) {
    // quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));
    return v;
}

template <bool NHWC>
__global__ __launch_bounds__(256) void delta_flow_features_kernel(DeltaFlowLevels lv, int nlev,
                                                                  int B, int C,
                                                                  const int32_t *__restrict__ valid) {
    extern __shared__ float4 wl[];  // NHWC: the level's weights, [18][C / 4] float4
    __shared__ float part[kDfHaloPix][kDfTaps];
    const int tid = threadIdx.x;

    // this workgroup's level, frame and tile
    int blk = blockIdx.x;
    const float *x = nullptr, *w = nullptr;
    float *feat = nullptr, *delta = nullptr;
    int H = 0, W = 0, ntx = 1, nty = 1;
    bool found = false;
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        if (l < nlev && !found) {
            const int tx = (lv.W[l] + kDfTile - 1) / kDfTile, ty = (lv.H[l] + kDfTile - 1) / kDfTile;
            const int n = B * tx * ty;
            if (blk < n) {
                found = true;
                x = lv.x[l];
                w = lv.w[l];
                feat = lv.feat[l];
                delta = lv.delta[l];
                H = lv.H[l];
                W = lv.W[l];
                ntx = tx;
                nty = ty;
            } else {
                blk -= n;
            }
        }
    }
    if (!found) return;  // uniform over the workgroup
    const int b = blk / (ntx * nty);
    const int t2 = blk - b * ntx * nty;
    const int y0 = (t2 / ntx) * kDfTile, x0 = (t2 % ntx) * kDfTile;

    if (NHWC) {
        const int C4 = C >> 2;
        const float4 *w4 = reinterpret_cast<const float4 *>(w);
        for (int i = tid; i < kDfTaps * C4; i += 256) wl[i] = w4[i];
        __syncthreads();
        const int g = tid >> 4, j = tid & 15;
        const float4 *frame = reinterpret_cast<const float4 *>(x) + (int64_t)b * H * W * C4;
        // A step is one pixel pair (q0 = g + 32 * n and q0 + 16) times one chunk of
        // 256 channels (four float4 per lane and pixel); the loads of step n + 1
        // are issued before the arithmetic of step n.
        const int nchunk = (C4 + 63) >> 6;
        const int steps = ((kDfHaloPix + 31) / 32) * nchunk;
        float4 xa[4], xc[4], na[4], nc[4];
        bool any = false, nany = false;
        auto load = [&](int step, float4(&a)[4], float4(&c)[4], bool &some) {
            const int q0 = g + 32 * (step / nchunk), chunk = step % nchunk;
            // every load is unconditional and 16 bytes wide, from an address clamped
            // into the frame; what lies outside is replaced by zero afterwards
            auto pixel = [&](int q, bool &in) -> const float4 * {
                const int iy = y0 - 1 + q / kDfHalo, ix = x0 - 1 + q % kDfHalo;
                in = q < kDfHaloPix && iy >= 0 && iy < H && ix >= 0 && ix < W;
                return frame + ((int64_t)min(max(iy, 0), H - 1) * W + min(max(ix, 0), W - 1)) * C4;
            };
            bool in0, in1;
            const float4 *p0 = pixel(q0, in0), *p1 = pixel(q0 + 16, in1);
            some = in0 || in1;  // uniform over the 16 lanes of the pixel pair
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int c4 = min(chunk * 64 + v * 16 + j, C4 - 1);
                const float4 ta = p0[c4], tc = p1[c4];
                a[v] = in0 ? ta : z;
                c[v] = in1 ? tc : z;
            }
        };
        df_float2 acc[kDfTaps];
#pragma unroll
        for (int t = 0; t < kDfTaps; ++t) acc[t] = df_float2{0.f, 0.f};
        load(0, xa, xc, any);
        for (int step = 0; step < steps; ++step) {
            if (step + 1 < steps) load(step + 1, na, nc, nany);
            const int q0 = g + 32 * (step / nchunk), chunk = step % nchunk;
            if (any) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (chunk * 64 + v * 16 < C4) {  // uniform: C4 is a multiple of 16
                        const int c4 = chunk * 64 + v * 16 + j;
                        const float4 a = xa[v], c = xc[v];
#pragma unroll
                        for (int t = 0; t < kDfTaps; ++t) {
                            const float4 wv = wl[t * C4 + c4];
                            df_float2 s = acc[t];
                            s = __builtin_elementwise_fma(df_float2{a.x, c.x}, df_float2{wv.x, wv.x}, s);
                            s = __builtin_elementwise_fma(df_float2{a.y, c.y}, df_float2{wv.y, wv.y}, s);
                            s = __builtin_elementwise_fma(df_float2{a.z, c.z}, df_float2{wv.z, wv.z}, s);
                            s = __builtin_elementwise_fma(df_float2{a.w, c.w}, df_float2{wv.w, wv.w}, s);
                            acc[t] = s;
                        }
                    }
                }
            }
            if (chunk == nchunk - 1) {
                if (any) {
#pragma unroll
                    for (int t = 0; t < kDfTaps; ++t) {
                        acc[t].x = row16_sum(acc[t].x);
                        acc[t].y = row16_sum(acc[t].y);
                    }
                }
                // lane t of the 16 writes tap t (taps 16, 17 by lanes 0, 1)
                if (q0 < kDfHaloPix) {
#pragma unroll
                    for (int t = 0; t < kDfTaps; ++t) {
                        if (j == (t & 15)) {
                            part[q0][t] = acc[t].x;
                            if (q0 + 16 < kDfHaloPix) part[q0 + 16][t] = acc[t].y;
                        }
                    }
                }
#pragma unroll
                for (int t = 0; t < kDfTaps; ++t) acc[t] = df_float2{0.f, 0.f};
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                xa[v] = na[v];
                xc[v] = nc[v];
            }
            any = nany;
        }
    } else {
        const int64_t plane = (int64_t)H * W;
        const float *frame = x + (int64_t)b * C * plane;
        // halo pixels tid and tid + 256 (the second for tid < 68)
        const float *p[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int q = tid + e * 256;
            const int iy = y0 - 1 + q / kDfHalo, ix = x0 - 1 + q % kDfHalo;
            const bool in = q < kDfHaloPix && iy >= 0 && iy < H && ix >= 0 && ix < W;
            p[e] = in ? frame + (int64_t)iy * W + ix : nullptr;
        }
        float acc[2][kDfTaps];
#pragma unroll
        for (int t = 0; t < kDfTaps; ++t) acc[0][t] = acc[1][t] = 0.f;
        if (p[0] || p[1]) {
            for (int c = 0; c < C; ++c) {
                const float a = p[0] ? p[0][c * plane] : 0.f;
                const float d = p[1] ? p[1][c * plane] : 0.f;
#pragma unroll
                for (int t = 0; t < kDfTaps; ++t) {
                    const float wv = w[t * C + c];  // wave-uniform
                    acc[0][t] = __builtin_fmaf(a, wv, acc[0][t]);
                    acc[1][t] = __builtin_fmaf(d, wv, acc[1][t]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < kDfTaps; ++t) {
            part[tid][t] = acc[0][t];
            if (tid + 256 < kDfHaloPix) part[tid + 256][t] = acc[1][t];
        }
    }
    __syncthreads();

    const int oy = tid >> 4, ox = tid & 15;
    const int y = y0 + oy, xx = x0 + ox;
    if (y >= H || xx >= W) return;
    float pre[2] = {0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float *q = part[(oy + ky) * kDfHalo + ox + kx] + (ky * 3 + kx) * 2;
            pre[0] += q[0];
            pre[1] += q[1];
        }
    const int ok = valid[b];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        const int64_t i = (((int64_t)b * 2 + o) * H + y) * W + xx;
        const float nw = tanhf(pre[o]);
        const float old = feat[i];
        delta[i] = ok ? nw - old : 0.f;
        feat[i] = nw;
    }
}

int launch_delta_flow_features(const DeltaFlowLevels &lv, int nlev, int B, int C, int nhwc,
                               const int32_t *valid, hipStream_t s) {
    if (nlev < 1 || nlev > 5 || B < 1 || C < 1 || !valid) return VD_ERR_ARG;
    if (C % 64 || C > 512) return VD_ERR_SHAPE;  // 18 * C * 4 bytes of weights in LDS
    int64_t blocks = 0;
    for (int l = 0; l < nlev; ++l) {
        if (!lv.x[l] || !lv.w[l] || !lv.feat[l] || !lv.delta[l] || lv.H[l] < 1 || lv.W[l] < 1)
            return VD_ERR_ARG;
        if ((reinterpret_cast<uintptr_t>(lv.x[l]) | reinterpret_cast<uintptr_t>(lv.w[l])) & 15)
            return VD_ERR_ARG;
        if ((int64_t)B * lv.H[l] * lv.W[l] * 2 > 0x7fffffff) return VD_ERR_SHAPE;
        blocks += (int64_t)B * ((lv.H[l] + kDfTile - 1) / kDfTile) *
                  ((lv.W[l] + kDfTile - 1) / kDfTile);
    }
    if (blocks > 0x7fffffff) return VD_ERR_SHAPE;
    const dim3 grid((unsigned)blocks), block(256);
    if (nhwc)
        hipLaunchKernelGGL(delta_flow_features_kernel<true>, grid, block,
                           (size_t)kDfTaps * C * sizeof(float), s, lv, nlev, B, C, valid);
    else
        hipLaunchKernelGGL(delta_flow_features_kernel<false>, grid, block, 0, s, lv, nlev, B, C,
                           valid);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

// ------------------------------------------------------------------ to levels
static constexpr int kDfBlobTile = 64;

struct DeltaMaps {
    const float *d[5];  // strides 64, 32, 16, 8, 4 (the reference's order)
    float *out[5];      // level flows, same order; NULL = not wanted
};

// acc[r][c] (both channels) += bilinear_up(d, K)(y0 + r, x0 + c) * K for the
// thread's 4 x 4 block; d is B x 2 x Hs x Ws
template <int K>
__device__ __forceinline__ void df_add_level(const float *__restrict__ d, int f, int Hs, int Ws,
                                             int y0, int x0, float (&au)[4][4],
                                             float (&av)[4][4]) {
    constexpr int NW = K == 4 ? 3 : 2;  // source window side of a 4 x 4 block
    constexpr float inv = 1.0f / K, scale = (float)K;
    int ys[4], xs[4];
    float ly[4], lx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float sy = fmaxf((y0 + i + 0.5f) * inv - 0.5f, 0.f);
        const float sx = fmaxf((x0 + i + 0.5f) * inv - 0.5f, 0.f);
        ys[i] = (int)sy;
        xs[i] = (int)sx;
        ly[i] = sy - (float)ys[i];
        lx[i] = sx - (float)xs[i];
    }
    const int ym = ys[0], xm = xs[0];
    float s[2][NW][NW];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const float *pl = d + ((int64_t)f * 2 + ch) * Hs * Ws;
#pragma unroll
        for (int r = 0; r < NW; ++r) {
            const float *row = pl + (int64_t)min(ym + r, Hs - 1) * Ws;
#pragma unroll
            for (int c = 0; c < NW; ++c) s[ch][r][c] = row[min(xm + c, Ws - 1)];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool dy = NW == 3 && ys[r] != ym;  // window row 1, 2 in place of 0, 1
        const float hy1 = ly[r], hy0 = 1.f - hy1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool dx = NW == 3 && xs[c] != xm;
            const float hx1 = lx[c], hx0 = 1.f - hx1;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                float t[2][2];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float lo = s[ch][a][e];
                        const float hi = s[ch][NW == 3 ? a + 1 : a][NW == 3 ? e + 1 : e];
                        const float ylo = s[ch][NW == 3 ? a + 1 : a][e];
                        const float xlo = s[ch][a][NW == 3 ? e + 1 : e];
                        t[a][e] = dy ? (dx ? hi : ylo) : (dx ? xlo : lo);
                    }
                const float v = hy0 * (hx0 * t[0][0] + hx1 * t[0][1]) +
                                hy1 * (hx0 * t[1][0] + hx1 * t[1][1]);
                if (ch == 0) au[r][c] = au[r][c] + v * scale;
                else av[r][c] = av[r][c] + v * scale;
            }
        }
    }
}

__device__ __forceinline__ float df_quad(const float *s, int pitch, int Y, int X) {
    const float *q = s + 2 * Y * pitch + 2 * X;
    return (q[0] + q[1]) + (q[pitch] + q[pitch + 1]);
}

__global__ __launch_bounds__(256) void delta_flow_to_levels_kernel(DeltaMaps m, int Hp, int Wp,
                                                                   float *__restrict__ blob) {
    __shared__ float s4[2][16][16], s8[2][8][8], s16[2][4][4], s32[2][2][2];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int bx = tid & 15, by = tid >> 4;
    const int y0 = blockIdx.y * kDfBlobTile + by * 4, x0 = blockIdx.x * kDfBlobTile + bx * 4;

    float au[4][4], av[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) au[r][c] = av[r][c] = 0.f;
    df_add_level<64>(m.d[0], f, Hp / 64, Wp / 64, y0, x0, au, av);
    df_add_level<32>(m.d[1], f, Hp / 32, Wp / 32, y0, x0, au, av);
    df_add_level<16>(m.d[2], f, Hp / 16, Wp / 16, y0, x0, au, av);
    df_add_level<8>(m.d[3], f, Hp / 8, Wp / 8, y0, x0, au, av);
    df_add_level<4>(m.d[4], f, Hp / 4, Wp / 4, y0, x0, au, av);

    const int64_t plane = (int64_t)Hp * Wp;
    if (blob) {
        float *d = blob + (int64_t)f * 2 * plane + (int64_t)y0 * Wp + x0;  // 16-byte aligned
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            *reinterpret_cast<float4 *>(d + (int64_t)r * Wp) =
                make_float4(au[r][0], au[r][1], au[r][2], au[r][3]);
            *reinterpret_cast<float4 *>(d + plane + (int64_t)r * Wp) =
                make_float4(av[r][0], av[r][1], av[r][2], av[r][3]);
        }
    }

    float ru[4], rv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ru[r] = (au[r][0] + au[r][1]) + (au[r][2] + au[r][3]);
        rv[r] = (av[r][0] + av[r][1]) + (av[r][2] + av[r][3]);
    }
    const float su = (ru[0] + ru[1]) + (ru[2] + ru[3]);
    const float sv = (rv[0] + rv[1]) + (rv[2] + rv[3]);
    s4[0][by][bx] = su;
    s4[1][by][bx] = sv;

    const int tY = blockIdx.y, tX = blockIdx.x;
    if (m.out[4]) {
        const int Hk = Hp / 4, Wk = Wp / 4;
        float *d = m.out[4] + ((int64_t)f * 2 * Hk + tY * 16 + by) * Wk + tX * 16 + bx;
        d[0] = su * (1.f / 64.f);
        d[(int64_t)Hk * Wk] = sv * (1.f / 64.f);
    }
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 6, Y = (tid >> 3) & 7, X = tid & 7;
        const float s = df_quad(&s4[c][0][0], 16, Y, X);
        s8[c][Y][X] = s;
        if (m.out[3]) {
            const int Hk = Hp / 8, Wk = Wp / 8;
            m.out[3][(((int64_t)f * 2 + c) * Hk + tY * 8 + Y) * Wk + tX * 8 + X] =
                s * (1.f / 512.f);
        }
    }
    __syncthreads();
    if (tid < 32) {
        const int c = tid >> 4, Y = (tid >> 2) & 3, X = tid & 3;
        const float s = df_quad(&s8[c][0][0], 8, Y, X);
        s16[c][Y][X] = s;
        if (m.out[2]) {
            const int Hk = Hp / 16, Wk = Wp / 16;
            m.out[2][(((int64_t)f * 2 + c) * Hk + tY * 4 + Y) * Wk + tX * 4 + X] =
                s * (1.f / 4096.f);
        }
    }
    __syncthreads();
    if (tid < 8) {
        const int c = tid >> 2, Y = (tid >> 1) & 1, X = tid & 1;
        const float s = df_quad(&s16[c][0][0], 4, Y, X);
        s32[c][Y][X] = s;
        if (m.out[1]) {
            const int Hk = Hp / 32, Wk = Wp / 32;
            m.out[1][(((int64_t)f * 2 + c) * Hk + tY * 2 + Y) * Wk + tX * 2 + X] =
                s * (1.f / 32768.f);
        }
    }
    __syncthreads();
    if (tid < 2 && m.out[0]) {
        const int c = tid;
        const float s = df_quad(&s32[c][0][0], 2, 0, 0);
        const int Hk = Hp / 64, Wk = Wp / 64;
        m.out[0][(((int64_t)f * 2 + c) * Hk + tY) * Wk + tX] = s * (1.f / 262144.f);
    }
}

int launch_delta_flow_to_levels(const float *const deltas[5], int B, int Hp, int Wp,
                                float *const levels[5], float *blob, hipStream_t s) {
    if (B < 1 || Hp < 1 || Wp < 1) return VD_ERR_ARG;
    if (Hp % kDfBlobTile || Wp % kDfBlobTile) return VD_ERR_SHAPE;
    if (B > 65535 || Hp / kDfBlobTile > 65535) return VD_ERR_SHAPE;
    if ((int64_t)B * 2 * Hp * Wp > 0x7fffffff) return VD_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(blob) & 15) return VD_ERR_ARG;
    DeltaMaps m;
    bool any = blob != nullptr;
    for (int i = 0; i < 5; ++i) {
        if (!deltas[i]) return VD_ERR_ARG;
        m.d[i] = deltas[i];
        m.out[i] = levels[i];
        any = any || levels[i];
    }
    if (!any) return VD_OK;
    const dim3 grid(Wp / kDfBlobTile, Hp / kDfBlobTile, B), block(256);
    hipLaunchKernelGGL(delta_flow_to_levels_kernel, grid, block, 0, s, m, Hp, Wp, blob);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
