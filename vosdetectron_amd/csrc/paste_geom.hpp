// The paste geometry and pixel function of segm_results, shared by the kernels
// that evaluate pasted masks (segm.hip: vd_paste_masks, vd_segm_rle; label_map.hip:
// vd_label_maps).  One definition, so every user gives bit-identical pixels.  The
// arithmetic is described at the top of segm.hip; build with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace vd {

static constexpr int kPasteMaxR = 62;  // (R+2)^2 floats in LDS

// One detection's paste geometry (expand_boxes, the clipped box, OpenCV's
// resize scales) and its pixel function over the zero-padded mask in LDS.
struct PasteGeom {
    int S, bx0, by0, x_0, x_1, y_0, y_1;
    double scale_x, scale_y;
    bool area2;
};

__device__ __forceinline__ PasteGeom paste_geom(const float *b, int R, int im_h, int im_w) {
    PasteGeom g;
    g.S = R + 2;
    // expand_boxes in float32 (numpy: float32 array op python float), then
    // astype(int32) truncates toward zero
    const float scale = (float)((R + 2.0) / R);
    float w_half = (b[2] - b[0]) * .5f, h_half = (b[3] - b[1]) * .5f;
    const float x_c = (b[2] + b[0]) * .5f, y_c = (b[3] + b[1]) * .5f;
    w_half *= scale;
    h_half *= scale;
    const int bx0 = (int)(x_c - w_half), bx2 = (int)(x_c + w_half);
    const int by0 = (int)(y_c - h_half), by2 = (int)(y_c + h_half);
    const int w = max(bx2 - bx0 + 1, 1), h = max(by2 - by0 + 1, 1);
    g.bx0 = bx0;
    g.by0 = by0;
    g.x_0 = max(bx0, 0);
    g.x_1 = min(bx2 + 1, im_w);
    g.y_0 = max(by0, 0);
    g.y_1 = min(by2 + 1, im_h);
    g.scale_x = 1. / ((double)w / (double)g.S);
    g.scale_y = 1. / ((double)h / (double)g.S);
    // OpenCV's resize dispatch turns INTER_LINEAR into INTER_AREA's fast path
    // when both scales are exactly 2 (a 15 x 15 box for R = 28): the mean of
    // each 2 x 2 block, ((a + b) + c) + d) * 0.25f in its scalar loop order
    // (restated from OpenCV's resize.cpp as remembered; cv2 absent: unpinned)
    g.area2 = g.scale_x == 2.0 && g.scale_y == 2.0;
    return g;
}

struct PasteRow {  // VResizeLinear taps of one output row
    int r0, r1;
    float b0, b1;
};

__device__ __forceinline__ PasteRow paste_row(const PasteGeom &g, int y) {
    PasteRow r;
    const int dy = y - g.by0;
    float fy = (float)((dy + 0.5) * g.scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    r.r0 = min(max(sy, 0), g.S - 1);
    r.r1 = min(max(sy + 1, 0), g.S - 1);
    r.b0 = 1.f - fy;
    r.b1 = fy;
    return r;
}

struct PasteCol {  // HResizeLinear taps of one output column
    int sx, sx1;
    float a0, a1;
};

__device__ __forceinline__ PasteCol paste_col(const PasteGeom &g, int x) {
    PasteCol c;
    const int dx = x - g.bx0;
    float fx = (float)((dx + 0.5) * g.scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= g.S - 1) { fx = 0.f; sx = g.S - 1; }
    c.sx = sx;
    c.sx1 = min(sx + 1, g.S - 1);
    c.a0 = 1.f - fx;
    c.a1 = fx;
    return c;
}

// Binarised pasted value of in-box pixel (x, y): cv2.resize(...) > thresh.
__device__ __forceinline__ int paste_pixel(const float *pm, const PasteGeom &g, const PasteRow &r,
                                           const PasteCol &c, int x, int y, float thresh) {
    const int S = g.S;
    if (g.area2) {
        const int dx = x - g.bx0, dy = y - g.by0;
        const float *p0 = pm + (2 * dy) * S + 2 * dx, *p1 = p0 + S;
        const float val = (((p0[0] + p0[1]) + p1[0]) + p1[1]) * 0.25f;
        return val > thresh ? 1 : 0;
    }
    const float d0 = pm[r.r0 * S + c.sx] * c.a0 + pm[r.r0 * S + c.sx1] * c.a1;
    const float d1 = pm[r.r1 * S + c.sx] * c.a0 + pm[r.r1 * S + c.sx1] * c.a1;
    const float val = d0 * r.b0 + d1 * r.b1;
    return val > thresh ? 1 : 0;
}

// (R+2)^2 zero-padded mask of detection m into LDS
__device__ __forceinline__ void load_padded(float *pm, const float *src, int R) {
    const int S = R + 2;
    for (int i = threadIdx.x; i < S * S; i += blockDim.x) {
        const int y = i / S, x = i - y * S;
        pm[i] = (y >= 1 && y <= R && x >= 1 && x <= R) ? src[(y - 1) * R + (x - 1)] : 0.f;
    }
}

}  // namespace vd
