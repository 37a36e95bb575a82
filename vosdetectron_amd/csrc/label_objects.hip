// The objects of a label map on the device (vd_label_objects): what the reference's
// host loops over np.unique(gt) make of an H x W object-ID map.
//
// Reference: DAVIS_imdb.get_gt / get_bboxes (imdb/vos/davis_db.py:180-204) with the box
// form of lib_vos/tools/get_cls_mapper.py:129-136, and add_gt_annotations_to_entry
// (davis_db.py:407-517): per distinct non-zero value the binary mask,
// cv2.boundingRect, _expand_box, xywh_to_xyxy, clip_xyxy_to_image, the area, the
// validity filter and mask_util.encode.
//
// label_stats_init_kernel: the per-frame 256-entry table (min x, max x, min y, max y,
// count) in the workspace set to its neutral element.
//
// label_stats_kernel (grid: blocks x frames): the maps are read once, 16 bytes per
// lane at 16-byte aligned addresses (the first and last chunk of a frame byte by
// byte), a wave reading 1024 consecutive bytes.  A span of equal bytes in flat
// (row-major) order updates one table entry: on one row it covers [x0, x1], on more
// than one it covers a whole row's width.  A wave whose 1024 bytes are all equal
// -- most of a DAVIS map is background -- makes one update; otherwise each lane
// walks the runs of its 16 bytes.  Updates go to a table in LDS (atomics), which is
// merged into the frame's table with integer global atomics (min / max / add):
// order-independent, so the table is the same in every run.
//
// label_finish_kernel (one workgroup per frame, one thread per value): get_gt's 255
// remap on the table (255 joins value len(vals) - 1: union rect, summed count), the
// box arithmetic in float64, the validity filter, the ascending compaction
// (block_compact), and the (value, second value, rect) slot list the RLE pass reads.
//
// label_rle_kernel (one workgroup per frame and object slot): segm.hip's fused RLE
// with `label == value` in place of the pasted pixel.  Outside the bounding rect the
// plane is 0, so every change lies in a rect column.  A wave walks one column 64 rows
// at a time: a lane reads its pixel, compares with the lane above (lane 0 with the
// previous chunk's last value) and a ballot counts / places the changes.  Pass 1
// counts per column, a block scan orders the columns, pass 2 writes the positions and
// they are differenced in place into run lengths.  No column tile is staged in LDS:
// the lanes of a wave read one byte each from 64 rows, and the waves of the workgroup
// walk neighbouring columns at the same time, so a fetched line serves them from cache.
#include "common.hpp"
#include "vosdet_internal.hpp"

#include <limits.h>

#include <algorithm>

namespace vd {

namespace {

constexpr int kObjMaxCap = 255;
constexpr int kObjMaxF = 65535;   // gridDim.y
constexpr int kObjMaxW = 8192;    // the RLE pass's column table in LDS
constexpr int kStatThreads = 256;
constexpr int kStatChunksPerThread = 4;  // 64 bytes per lane and workgroup visit
constexpr int kStatMaxBlocks = 1024;     // per frame; more chunks: the workgroups stride
constexpr int kRleThreads = 1024;
constexpr int kTableInts = 256 * 5;      // min x, max x, min y, max y, count
constexpr size_t kHeadBytes = 16;        // per frame: the number of slots

struct ObjSlot {  // one kept object of a frame, for the RLE pass
    int32_t value, alt;  // the mask is label == value || label == alt
    int32_t x, y, w, h;
    int32_t pad0, pad1;
};
static_assert(sizeof(ObjSlot) == 32, "ObjSlot is 32 bytes");
// label_stats_kernel's short cut tests ballot() == ~0ull: every wave must be whole and no
// lane may leave the chunk loop before the ballot
static_assert(kStatThreads % VD_WAVE == 0, "label_stats_kernel: whole waves only");

__host__ __device__ inline size_t frame_ws_bytes(int obj_cap) {
    return (size_t)kTableInts * sizeof(int32_t) + kHeadBytes + (size_t)obj_cap * sizeof(ObjSlot);
}

__global__ __launch_bounds__(256) void label_stats_init_kernel(int32_t *__restrict__ ws,
                                                               size_t frame_ints) {
    int32_t *tab = ws + (size_t)blockIdx.x * frame_ints;
    const int v = threadIdx.x;
    tab[v * 5 + 0] = INT_MAX;
    tab[v * 5 + 1] = -1;
    tab[v * 5 + 2] = INT_MAX;
    tab[v * 5 + 3] = -1;
    tab[v * 5 + 4] = 0;
}

// a span of n >= 1 equal bytes of value v in flat order, its first pixel at (x, y)
__device__ __forceinline__ void table_add(int32_t *tab, int v, int x, int y, int n, int W) {
    int x0 = x, x1 = x + n - 1, y1 = y;
    if (x1 >= W) {  // more than one row: the span covers a full width
        y1 = y + x1 / W;
        x0 = 0;
        x1 = W - 1;
    }
    atomicMin(&tab[v * 5 + 0], x0);
    atomicMax(&tab[v * 5 + 1], x1);
    atomicMin(&tab[v * 5 + 2], y);
    atomicMax(&tab[v * 5 + 3], y1);
    atomicAdd(&tab[v * 5 + 4], n);
}

__global__ __launch_bounds__(kStatThreads) void label_stats_kernel(
    const uint8_t *__restrict__ labels, int H, int W, int32_t *__restrict__ ws,
    size_t frame_ints) {
    __shared__ int32_t tab[kTableInts];
    const int f = blockIdx.y, t = threadIdx.x;
    for (int i = t; i < 256; i += kStatThreads) {
        tab[i * 5 + 0] = INT_MAX;
        tab[i * 5 + 1] = -1;
        tab[i * 5 + 2] = INT_MAX;
        tab[i * 5 + 3] = -1;
        tab[i * 5 + 4] = 0;
    }
    __syncthreads();
    const int64_t hw = (int64_t)H * W;  // < 2^31
    const uint8_t *p = labels + (int64_t)f * hw;
    const int mis = (int)((uintptr_t)p & 15u);
    // chunk c holds the flat pixels [16 c - mis, 16 c - mis + 16) of the frame
    const int64_t nchunks = (hw + mis + 15) / 16;
    const int64_t per_visit = (int64_t)kStatThreads * kStatChunksPerThread;
    for (int64_t base = (int64_t)blockIdx.x * per_visit; base < nchunks;
         base += (int64_t)gridDim.x * per_visit) {
#pragma unroll 1
        for (int k = 0; k < kStatChunksPerThread; ++k) {
            const int64_t c = base + (int64_t)k * kStatThreads + t;
            const int64_t q0 = c * 16 - mis;  // first flat pixel of the chunk (may be < 0)
            const bool any = c < nchunks;
            const bool full = any && q0 >= 0 && q0 + 16 <= hw;
            uint64_t wl = 0ull, wh = 0ull;  // bytes 0..7 and 8..15 of the chunk
            int lo = 0, hi = 0;             // valid bytes [lo, hi)
            if (full) {
                const uint4 u = *reinterpret_cast<const uint4 *>(p + q0);
                wl = ((uint64_t)u.y << 32) | u.x;
                wh = ((uint64_t)u.w << 32) | u.z;
                hi = 16;
            } else if (any) {
                lo = q0 < 0 ? (int)-q0 : 0;
                hi = (int)min((int64_t)16, hw - q0);
                for (int b = lo; b < hi; ++b) {
                    const uint64_t v = (uint64_t)p[q0 + b] << (8 * (b & 7));
                    if (b < 8) wl |= v; else wh |= v;
                }
            }
            auto byte_at = [&](int b) -> uint32_t {
                return (uint32_t)((b < 8 ? wl : wh) >> (8 * (b & 7))) & 0xffu;
            };
            const uint32_t v0 = (uint32_t)wl & 0xffu;
            const bool uni = full && wl == v0 * 0x0101010101010101ull && wh == wl;
            // the wave's 1024 bytes are one span of one value.  All 64 lanes reach this
            // ballot (the loops above are workgroup-uniform, no lane has left them); a
            // partial wave would only miss the short cut, never take it wrongly
            const uint32_t vl = (uint32_t)__builtin_amdgcn_readfirstlane((int)v0);
            if (ballot(uni && v0 == vl) == ~0ull) {
                if (lane_id() == 0) {
                    const int y = (int)((uint32_t)q0 / (uint32_t)W);  // full: 0 <= q0 < 2^31
                    table_add(tab, (int)v0, (int)q0 - y * W, y, 16 * VD_WAVE, W);
                }
                continue;
            }
            if (hi <= lo) continue;
            const int64_t qs = q0 + lo;
            int y = (int)((uint32_t)qs / (uint32_t)W), x = (int)qs - y * W;  // 0 <= qs < 2^31
            if (uni) {
                table_add(tab, (int)v0, x, y, 16, W);
                continue;
            }
            int b = lo;
            while (b < hi) {
                const uint32_t v = byte_at(b);
                int e = b + 1;
                while (e < hi && byte_at(e) == v) ++e;
                table_add(tab, (int)v, x, y, e - b, W);
                x += e - b;
                while (x >= W) {
                    x -= W;
                    ++y;
                }
                b = e;
            }
        }
    }
    __syncthreads();
    int32_t *g = ws + (size_t)f * frame_ints;
    for (int i = t; i < 256; i += kStatThreads) {
        const int n = tab[i * 5 + 4];
        if (n > 0) {
            atomicMin(&g[i * 5 + 0], tab[i * 5 + 0]);
            atomicMax(&g[i * 5 + 1], tab[i * 5 + 1]);
            atomicMin(&g[i * 5 + 2], tab[i * 5 + 2]);
            atomicMax(&g[i * 5 + 3], tab[i * 5 + 3]);
            atomicAdd(&g[i * 5 + 4], n);
        }
    }
}

__global__ __launch_bounds__(256) void label_finish_kernel(
    int32_t *__restrict__ ws, size_t frame_ints, int H, int W, int remap255, double expand,
    int obj_cap, uint8_t *__restrict__ ids, int32_t *__restrict__ rects,
    int32_t *__restrict__ areas, float *__restrict__ boxes, int32_t *__restrict__ counts) {
    __shared__ int32_t tab[kTableInts];
    __shared__ int scratch[16];
    const int f = blockIdx.x, v = threadIdx.x;
    int32_t *fw = ws + (size_t)f * frame_ints;
    int32_t *nslots = fw + kTableInts;
    ObjSlot *slots = reinterpret_cast<ObjSlot *>((char *)(fw + kTableInts) + kHeadBytes);
#pragma unroll
    for (int k = 0; k < 5; ++k) tab[v * 5 + k] = fw[v * 5 + k];
    __syncthreads();
    const int nvals = block_sum(tab[v * 5 + 4] > 0 ? 1 : 0, scratch);  // np.unique of the raw map
    int x0 = tab[v * 5 + 0], x1 = tab[v * 5 + 1], y0 = tab[v * 5 + 2], y1 = tab[v * 5 + 3];
    int area = tab[v * 5 + 4];
    int alt = v;
    const bool has255 = remap255 && tab[255 * 5 + 4] > 0;
    const int target = nvals - 1;  // get_gt: out[ann == 255] = len(vals) - 1
    if (has255 && target != 255) {
        if (v == 255) area = 0;
        if (v == target) {  // the two objects merge, as they do in the reference
            x0 = min(x0, tab[255 * 5 + 0]);
            x1 = max(x1, tab[255 * 5 + 1]);
            y0 = min(y0, tab[255 * 5 + 2]);
            y1 = max(y1, tab[255 * 5 + 3]);
            area += tab[255 * 5 + 4];
            alt = 255;
        }
    }
    const int rx = x0, ry = y0, rw = x1 - x0 + 1, rh = y1 - y0 + 1;  // cv2.boundingRect
    double bx1 = 0.0, by1 = 0.0, bx2 = 0.0, by2 = 0.0;
    bool keep = v != 0 && area > 0;
    if (expand < 0.0) {  // get_cls_mapper.py:129-136
        bx1 = rx, by1 = ry, bx2 = rx + rw, by2 = ry + rh;
    } else if (keep) {
        // _expand_box, xywh_to_xyxy, clip_xyxy_to_image: float64, every step rounded
        const double e = __dsqrt_rn((double)((int64_t)rw * rh)) * expand;
        const double x = (double)rx - e / 2.0, y = (double)ry - e / 2.0;
        const double h = (double)rh + e, w = (double)rw + e;
        bx1 = x, by1 = y;
        bx2 = x + fmax(0.0, w - 1.0);
        by2 = y + fmax(0.0, h - 1.0);
        bx1 = fmin((double)W - 1.0, fmax(0.0, bx1));
        by1 = fmin((double)H - 1.0, fmax(0.0, by1));
        bx2 = fmin((double)W - 1.0, fmax(0.0, bx2));
        by2 = fmin((double)H - 1.0, fmax(0.0, by2));
        keep = bx2 > bx1 && by2 > by1;
    }
    __syncthreads();
    tab[v] = keep ? 1 : 0;  // reused as the predicate of the compaction
    __syncthreads();
    const int kept = block_sum(tab[v], scratch);
    if (kept > obj_cap) {
        if (v == 0) {
            counts[f] = VD_COUNT_SELECT_FAILED;
            *nslots = 0;
        }
        return;
    }
    block_compact(
        256, [&](int i) { return tab[i] != 0; },
        [&](int pos, int i) {  // i == v: thread i evaluates its own value
            const int64_t o = (int64_t)f * obj_cap + pos;
            ids[o] = (uint8_t)v;
            rects[o * 4 + 0] = rx, rects[o * 4 + 1] = ry, rects[o * 4 + 2] = rw, rects[o * 4 + 3] = rh;
            areas[o] = area;
            boxes[o * 4 + 0] = (float)bx1, boxes[o * 4 + 1] = (float)by1;
            boxes[o * 4 + 2] = (float)bx2, boxes[o * 4 + 3] = (float)by2;
            ObjSlot s;
            s.value = v, s.alt = alt, s.x = rx, s.y = ry, s.w = rw, s.h = rh, s.pad0 = s.pad1 = 0;
            slots[pos] = s;
        },
        scratch);
    if (v == 0) {
        counts[f] = kept;
        *nslots = kept;
    }
}

// the changes of rect column x, rows [y0, y1): counted, and with WRITE their
// column-major positions stored at pos[0 ..).  The same walk as segm.hip's
// segm_column_changes with the pixel read from the map.
template <bool WRITE>
__device__ int label_column_changes(const uint8_t *__restrict__ p, int va, int vb, int x, int x0,
                                    int x1, int y0, int y1, int H, int W, uint32_t *pos) {
    const int lane = lane_id();
    auto pix = [&](int xx, int yy) -> int {
        const int v = p[(int64_t)yy * W + xx];
        return (v == va || v == vb) ? 1 : 0;
    };
    int prev = 0;  // the plane value just before (x, y0) in column-major order
    if (y0 == 0 && y1 == H && x > x0) prev = pix(x - 1, H - 1);
    int cnt = 0;
    for (int yb = y0; yb < y1; yb += VD_WAVE) {
        const int y = yb + lane;
        const bool in = y < y1;
        const int v = in ? pix(x, y) : 0;
        int vp = __shfl_up(v, 1);
        if (lane == 0) vp = prev;
        const bool ch = in && v != vp;
        const uint64_t b = ballot(ch);
        if (WRITE && ch) pos[cnt + lane_prefix(b)] = (uint32_t)((int64_t)x * H + y);
        cnt += __popcll(b);
        prev = __shfl(v, min(VD_WAVE - 1, y1 - 1 - yb));
    }
    // 1 -> 0 after the column's last rect pixel, unless that next position is the first
    // pixel of the next rect column (which compares against it itself)
    const int64_t q = (int64_t)x * H + y1;
    if (prev == 1 && q < (int64_t)H * W && !(y1 == H && y0 == 0 && x + 1 < x1)) {
        if (WRITE && lane == 0) pos[cnt] = (uint32_t)q;
        ++cnt;
    }
    return cnt;
}

__global__ __launch_bounds__(kRleThreads) void label_rle_kernel(
    const uint8_t *__restrict__ labels, int H, int W, const int32_t *__restrict__ ws,
    size_t frame_ints, int obj_cap, uint32_t *__restrict__ rle_counts, int rle_cap,
    int32_t *__restrict__ rle_n) {
    __shared__ int colofs[kObjMaxW + 1];
    __shared__ int part[kRleThreads];
    const int k = blockIdx.x, f = blockIdx.y, t = threadIdx.x, nt = blockDim.x;
    const int32_t *fw = ws + (size_t)f * frame_ints;
    if (k >= fw[kTableInts]) return;  // uniform: rows past the count are not written
    const ObjSlot s =
        reinterpret_cast<const ObjSlot *>((const char *)(fw + kTableInts) + kHeadBytes)[k];
    const uint8_t *p = labels + (int64_t)f * H * W;
    const int x0 = s.x, x1 = s.x + s.w, y0 = s.y, y1 = s.y + s.h;
    const int ncol = s.w;
    const int64_t row = (int64_t)f * obj_cap + k;
    uint32_t *cnt = rle_counts + row * rle_cap;
    const int wv = wave_id(), nw = num_waves();
    for (int ci = wv; ci < ncol; ci += nw) {
        const int c = label_column_changes<false>(p, s.value, s.alt, x0 + ci, x0, x1, y0, y1, H, W,
                                                  nullptr);
        if (lane_id() == 0) colofs[ci] = c;
    }
    __syncthreads();
    // exclusive scan of the per-column counts: contiguous chunk per thread
    const int per = (ncol + nt - 1) / nt;
    const int a0 = min(t * per, ncol), a1 = min(a0 + per, ncol);
    int sum = 0;
    for (int i = a0; i < a1; ++i) sum += colofs[i];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const int total = part[nt - 1];
    int run = part[t] - sum;
    for (int i = a0; i < a1; ++i) {
        const int c = colofs[i];
        colofs[i] = run;
        run += c;
    }
    const int n = total + 1;  // the leading (possibly empty) zero run + one per change
    if (t == 0) rle_n[row] = n <= rle_cap ? n : -n;
    if (n > rle_cap) return;  // the caller retries with rle_cap >= n
    __syncthreads();
    for (int ci = wv; ci < ncol; ci += nw)
        label_column_changes<true>(p, s.value, s.alt, x0 + ci, x0, x1, y0, y1, H, W,
                                   cnt + 1 + colofs[ci]);
    if (t == 0) cnt[0] = 0;
    __threadfence_block();
    __syncthreads();
    // run lengths in place, lowest chunk first, as mask_rle_kernel does
    const uint32_t hw = (uint32_t)((int64_t)H * W);
    const int nchunks = (n + nt - 1) / nt;
    for (int c = 0; c < nchunks; ++c) {
        const int i = c * nt + t;
        uint32_t a = 0, bnext = 0;
        if (i < n) {
            a = cnt[i];
            bnext = i + 1 < n ? cnt[i + 1] : hw;
        }
        __threadfence_block();
        __syncthreads();
        if (i < n) cnt[i] = bnext - a;
        __threadfence_block();
        __syncthreads();
    }
}

bool shape_ok(int F, int H, int W, int obj_cap) {
    return F >= 1 && F <= kObjMaxF && H >= 1 && W >= 1 && W <= kObjMaxW &&
           (int64_t)H * W < (1ll << 31) && obj_cap >= 1 && obj_cap <= kObjMaxCap;
}

}  // namespace

size_t label_objects_workspace_bytes(int F, int H, int W, int obj_cap) {
    if (!shape_ok(F, H, W, obj_cap)) return 0;
    return (size_t)F * frame_ws_bytes(obj_cap);
}

int launch_label_objects(const uint8_t *labels, int F, int H, int W, int remap255, double expand,
                         int obj_cap, int rle_cap, uint8_t *ids, int32_t *rects, int32_t *areas,
                         float *boxes, int32_t *counts, uint32_t *rle_counts, int32_t *rle_n,
                         void *workspace, size_t workspace_bytes, hipStream_t s) {
    if (!shape_ok(F, H, W, obj_cap)) return VD_ERR_SHAPE;
    if (workspace_bytes < label_objects_workspace_bytes(F, H, W, obj_cap)) return VD_ERR_WORKSPACE;
    if (!workspace || ((uintptr_t)workspace & 15u)) return VD_ERR_ARG;
    int32_t *ws = (int32_t *)workspace;
    const size_t frame_ints = frame_ws_bytes(obj_cap) / sizeof(int32_t);
    hipLaunchKernelGGL(label_stats_init_kernel, dim3(F), dim3(256), 0, s, ws, frame_ints);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    const int64_t nchunks = ((int64_t)H * W + 15 + 15) / 16;  // any misalignment
    const int64_t per_visit = (int64_t)kStatThreads * kStatChunksPerThread;
    const int blocks = (int)std::min<int64_t>((nchunks + per_visit - 1) / per_visit, kStatMaxBlocks);
    hipLaunchKernelGGL(label_stats_kernel, dim3(blocks, F), dim3(kStatThreads), 0, s, labels, H, W,
                       ws, frame_ints);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    hipLaunchKernelGGL(label_finish_kernel, dim3(F), dim3(256), 0, s, ws, frame_ints, H, W,
                       remap255, expand, obj_cap, ids, rects, areas, boxes, counts);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    if (rle_cap > 0) {
        hipLaunchKernelGGL(label_rle_kernel, dim3(obj_cap, F), dim3(kRleThreads), 0, s, labels, H,
                           W, (const int32_t *)ws, frame_ints, obj_cap, rle_counts, rle_cap, rle_n);
        if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    }
    return VD_OK;
}

}  // namespace vd
