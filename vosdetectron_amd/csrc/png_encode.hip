// Per-frame label maps as 8-bit indexed PNG file images, encoded on the device
// (vd_label_pngs).
//
// Reference: the last step of viz_mask_result (lib/utils/vis.py:152-155): img_saver is
// davis_saver -> image_saver -> io.imwrite_indexed (imdb/vos/davis_db.py:45-47), a
// PIL 'P' image with the DAVIS palette saved as PNG.  Here the file image is formed
// where the label map already is, so that the host copies the few KB of the stream
// instead of the H x W map and runs no zlib.
//
// File layout of one frame (offsets in bytes; n = lengths[f] - kPngFixed):
//     0  signature                         8
//     8  IHDR  length, type, 13, CRC      25
//    33  PLTE  length, type, 768, CRC    780
//   813  IDAT  length, type                8
//   821  zlib header 78 01                 2
//   823  deflate stream                    n
//        Adler-32, IDAT CRC, IEND       4 + 4 + 12
//
// Deflate form: filter type 0 on every row; the rows are cut into strips of kStripRows;
// a strip is one fixed-Huffman block (BTYPE 01) of literals and distance-1 matches
// (run-length coding inside a row), followed -- except for the last strip, which
// carries BFINAL -- by an empty stored block, whose LEN / NLEN words start on a byte
// boundary.  So every strip is a whole number of bytes, and strips are independent.
//
// png_strip_kernel (one wave per strip): per row, the filtered row is staged in LDS
// (all of a lane's loads in flight together); pass 1 finds the run starts with ballots
// (lane c keeps the 64 flags of chunk c), two wave scans give every chunk the last run
// start before it and the first after it; pass 2 gives every byte its run's (length,
// offset) from those, and from them alone decides whether a token starts there and
// which (token_at): no lane waits for another.  A prefix sum of the token bit lengths
// (one ballot per bit of the length) places the codes, which are ORed into an LDS
// image of the strip.  The image is copied to the strip's slot in `out` (the slots are laid out
// at the worst-case strip size, which is what the bound reserves).  The wave also
// forms the strip's part of the Adler-32 sums.
//
// png_frame_kernel (one workgroup per frame): prefix sum of the strip byte lengths,
// moves the strips together in place (towards lower addresses, chunk by chunk: all
// reads of a chunk, barrier, all writes), writes the constant chunks, the Adler-32 and
// the CRC-32s.  A CRC is computed by all threads over equal pieces aligned to the
// message's end; piece t is then multiplied by x^(8 * bytes after it) mod P and the
// products are XORed: crc(a || b) = crc(a) * x^(8|b|) (+) crc(b) for the raw register
// (no inversions); the pre-inversion is an XOR of the first four message bytes with FF,
// the post-inversion one of the result.
#include "common.hpp"
#include "vosdet_internal.hpp"

namespace vd {

static constexpr int kStripRows = 8;
static constexpr int kPngMaxW = 4095;    // W + 1 bytes of a row = at most 64 chunks of 64
static constexpr int kPngMaxH = 16384;   // 2048 strips: the frame kernel's LDS offsets
static constexpr int kPngMaxStrips = kPngMaxH / kStripRows;
static constexpr int kPngMaxF = 65535;   // gridDim.y
static constexpr int kPngHead = 8 + 25 + 780 + 8 + 2;  // bytes before the deflate stream
static constexpr int kPngTail = 4 + 4 + 12;            // Adler-32, IDAT CRC, IEND
static constexpr int kStageLoads = 16;    // row loads a lane keeps in flight
static constexpr int kFrameThreads = 1024;
static constexpr int kMoveBytes = 16;    // bytes a thread moves per chunk
static constexpr int kCrcLoads = 8;      // message bytes a thread loads ahead of its CRC
static constexpr uint32_t kCrcPoly = 0xedb88320u;
static constexpr uint32_t kAdlerMod = 65521u;

struct StripMeta {  // what a strip hands to the frame kernel
    uint32_t len;   // bytes of the strip's deflate piece
    uint32_t a;     // sum of the strip's filtered bytes, mod 65521
    uint32_t b;     // sum of (bytes of the frame after this one, itself included) * byte
    uint32_t pad;
};

// The most bytes a strip of `rows` rows can take: block header (3 bits), 9 bits for
// every filtered byte, end of block (7), stored-block header (3), padding to a byte,
// LEN / NLEN (4 bytes).  A match never costs more than the literals it replaces (at
// most 8 + 5 + 5 bits for at least 3 bytes).
__host__ __device__ inline int64_t strip_cap(int rows, int W) {
    return (9 * (int64_t)rows * (W + 1) + 13 + 7) / 8 + 4;
}

size_t label_png_bound(int H, int W) {
    if (H < 1 || W < 1 || H > kPngMaxH || W > kPngMaxW) return 0;
    const int ns = (H + kStripRows - 1) / kStripRows;
    return (size_t)(kPngHead + kPngTail + (int64_t)(ns - 1) * strip_cap(kStripRows, W) +
                    strip_cap(H - (ns - 1) * kStripRows, W));
}

size_t label_pngs_workspace_bytes(int F, int H, int W) {
    if (F < 1 || F > kPngMaxF || label_png_bound(H, W) == 0) return 0;
    const int ns = (H + kStripRows - 1) / kStripRows;
    return (size_t)F * ns * sizeof(StripMeta);
}

// ---------------------------------------------------------------------------
// tokens
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rev_bits(uint32_t code, int n) { return __brev(code) >> (32 - n); }

// literal v: code and bit count (Huffman codes enter the stream MSB first)
__device__ __forceinline__ uint32_t literal_code(uint32_t v, int &nbits) {
    if (v < 144u) {
        nbits = 8;
        return rev_bits(0x30u + v, 8);
    }
    nbits = 9;
    return rev_bits(0x190u + v - 144u, 9);
}

// match of length L (3..258) at distance 1: length code, extra bits, 5-bit distance code 0
__device__ __forceinline__ uint32_t match_code(int L, int &nbits) {
    const uint32_t x = (uint32_t)(L - 3);
    int e = 0;
    uint32_t idx = x;
    if (L == 258) {
        idx = 28;
    } else if (x >= 8u) {
        e = (31 - __clz((int)x)) - 2;
        idx = 4u * e + 4u + ((x >> e) & 3u);
    }
    const uint32_t extra = (L == 258) ? 0u : (x & ((1u << e) - 1u));
    uint32_t code;
    int n;
    if (idx < 23u) {  // symbols 257..279: 7 bits
        n = 7;
        code = rev_bits(idx + 1u, 7);
    } else {          // 280..285: 8 bits
        n = 8;
        code = rev_bits(0xC0u + idx - 23u, 8);
    }
    nbits = n + e + 5;
    return code | (extra << n);
}

// The token that starts at offset k of a run of R equal bytes (0 bits: none starts
// here).  The run is coded as its first byte, then matches over the other R - 1:
// 258 at a time, except that 259 or 260 left are coded as 256 + (3 or 4) so that no
// tail of 1 or 2 remains; a run of 2 or 3 is all literals.
__device__ __forceinline__ uint32_t token_at(uint32_t v, int k, int R, int &nbits) {
    nbits = 0;
    const int rem = R - 1;
    if (k == 0 || rem <= 2) return literal_code(v, nbits);
    const int j = k - 1, q = rem - j, m = j % 258;
    if (m == 0) {
        if (q >= 3) return match_code(q <= 258 ? q : ((q == 259 || q == 260) ? 256 : 258), nbits);
    } else if (m == 256 && (q == 3 || q == 4)) {
        return match_code(q, nbits);
    }
    return 0u;
}

__global__ __launch_bounds__(VD_WAVE) void png_strip_kernel(
    const uint8_t *__restrict__ labels, int H, int W, uint8_t *__restrict__ out, int64_t cap,
    StripMeta *__restrict__ meta, int img_words) {
    extern __shared__ uint32_t img[];  // the strip's deflate piece, little-endian bit order
    __shared__ uint8_t rowbuf[kPngMaxW + 1];  // the filtered row being coded
    const int s = blockIdx.x, f = blockIdx.y, ns = gridDim.x, lane = threadIdx.x;
    const int y0 = s * kStripRows, rows = min(kStripRows, H - y0);
    const bool last = s == ns - 1;
    const int n = W + 1, nch = (n + 63) / 64;
    for (int i = lane; i < img_words; i += VD_WAVE) img[i] = 0u;
    __syncthreads();

    const int64_t total_raw = (int64_t)H * n;
    uint64_t sum_a = 0, sum_b = 0;
    int64_t cursor = 3;  // bits; the block header is ORed in at the end
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const uint8_t *src = labels + ((int64_t)f * H + y) * W - 1;  // src[p], p >= 1
        // the filtered row into LDS (byte 0 is the filter type, 0): kStageLoads loads in
        // flight per lane, so a row costs a few memory latencies, not one per chunk
        __syncthreads();
        for (int c0 = 0; c0 < nch; c0 += kStageLoads) {
            uint8_t b[kStageLoads];
#pragma unroll
            for (int j = 0; j < kStageLoads; ++j) {
                const int p = (c0 + j) * 64 + lane;
                b[j] = (p >= 1 && p < n) ? src[p] : (uint8_t)0;
            }
#pragma unroll
            for (int j = 0; j < kStageLoads; ++j) {
                const int p = (c0 + j) * 64 + lane;
                if (p < n) rowbuf[p] = b[j];
            }
        }
        __syncthreads();
        // pass 1: run starts
        uint64_t myword = 0;
        for (int c = 0; c < nch; ++c) {
            const int p = c * 64 + lane;
            const bool in = p < n;
            const uint32_t v = in ? rowbuf[p] : 0u, pv = (in && p >= 1) ? rowbuf[p - 1] : 0u;
            const uint64_t bits = ballot(in && (p == 0 || v != pv));
            if (lane == c) myword = bits;
        }
        // lane c: the last run start at or before chunk c's end, the first one after it
        int last_start = myword ? lane * 64 + 63 - __clzll((long long)myword) : -1;
        int first_start = myword ? lane * 64 + __ffsll((unsigned long long)myword) - 1 : n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_up(last_start, o);
            if (lane >= o) last_start = max(last_start, a);
            const int b = __shfl_down(first_start, o);
            if (lane + o < 64) first_start = min(first_start, b);
        }
        const int start_before = __shfl_up(last_start, 1);  // of chunks < lane (lane >= 1)
        int start_after = __shfl_down(first_start, 1);      // of chunks > lane
        if (lane == 63) start_after = n;
        // pass 2: tokens.  c is uniform: the chunk's values come by readlane
        uint32_t row_a = 0, row_pv = 0;  // sum of v and of p * v over this lane's bytes
        for (int c = 0; c < nch; ++c) {
            const int p = c * 64 + lane;
            const bool in = p < n;
            const uint32_t v = in ? rowbuf[p] : 0u;
            const uint64_t bits = readlane64(myword, c);
            const int before = __builtin_amdgcn_readlane(start_before, c);
            const int after = min(__builtin_amdgcn_readlane(start_after, c), n);
            const uint64_t upto = bits & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
            const uint64_t above = (lane == 63) ? 0ull : (bits & ~((2ull << lane) - 1ull));
            const int rs = upto ? c * 64 + 63 - __clzll((long long)upto) : before;
            const int re = above ? c * 64 + __ffsll((unsigned long long)above) - 1 : after;
            int nb = 0;
            uint32_t tok = 0;
            if (in) {
                tok = token_at(v, p - rs, re - rs, nb);
                row_a += v;
                row_pv += (uint32_t)p * v;  // below 64 * 4096 * 255
            }
            // exclusive prefix sum of nb (< 32) over the lanes, one ballot per bit
            int excl = 0, total = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint64_t m = ballot((nb >> k) & 1);
                excl += lane_prefix(m) << k;
                total += __popcll(m) << k;
            }
            if (nb) {
                const int64_t at = cursor + excl;
                const int w = (int)(at >> 5);
                const uint64_t val = (uint64_t)tok << (at & 31);
                if (w < img_words) atomicOr(&img[w], (uint32_t)val);
                if ((uint32_t)(val >> 32) && w + 1 < img_words)
                    atomicOr(&img[w + 1], (uint32_t)(val >> 32));
            }
            cursor += total;
        }
        // Adler: byte p of this row counts (bytes of the frame from it on) times
        sum_a += row_a;
        sum_b += (uint64_t)(total_raw - (int64_t)y * n) * row_a - row_pv;
    }
    cursor += 7;  // end of block: seven zero bits
    if (!last) cursor += 3;  // empty stored block, not final: 0, 00
    int64_t nbytes = (cursor + 7) >> 3;
    __syncthreads();
    if (lane == 0) {
        atomicOr(&img[0], (last ? 1u : 0u) | 2u);  // BFINAL, BTYPE 01
        if (!last) {  // LEN 0000, NLEN FFFF
            const int64_t at = (nbytes + 2) * 8;
            const uint64_t val = (uint64_t)0xffffu << (at & 31);
            const int w = (int)(at >> 5);
            if (w < img_words) atomicOr(&img[w], (uint32_t)val);
            if ((uint32_t)(val >> 32) && w + 1 < img_words)
                atomicOr(&img[w + 1], (uint32_t)(val >> 32));
        }
    }
    if (!last) nbytes += 4;
    __syncthreads();
    const int64_t slot = strip_cap(kStripRows, W);
    nbytes = min(nbytes, min(strip_cap(rows, W), (int64_t)img_words * 4));  // holds by the bound
    uint8_t *dst = out + (int64_t)f * cap + kPngHead + (int64_t)s * slot;
    for (int64_t i = lane; i < nbytes; i += VD_WAVE)
        dst[i] = (uint8_t)(img[i >> 2] >> ((i & 3) * 8));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum_a += shfl_xor64(sum_a, o);
        sum_b += shfl_xor64(sum_b, o);
    }
    if (lane == 0) {
        StripMeta m;
        m.len = (uint32_t)nbytes;
        m.a = (uint32_t)(sum_a % kAdlerMod);
        m.b = (uint32_t)(sum_b % kAdlerMod);
        m.pad = 0u;
        meta[(int64_t)f * ns + s] = m;
    }
}

// ---------------------------------------------------------------------------
// CRC-32
// ---------------------------------------------------------------------------
// a * b mod P, polynomials in the reflected representation (bit 31 = x^0)
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

struct CrcPowers {  // x^(8 * 2^k) mod P
    uint32_t v[32];
};
constexpr CrcPowers crc_powers() {
    CrcPowers t{};
    uint32_t p = 0x40000000u;  // x^1
    for (int i = 0; i < 3; ++i) p = gf_mul(p, p);  // x^8
    for (int k = 0; k < 32; ++k) {
        t.v[k] = p;
        p = gf_mul(p, p);
    }
    return t;
}
__constant__ CrcPowers kCrcPowers = crc_powers();

// CRC-32 (as zlib.crc32) of msg[0, len), len >= 4, by the whole workgroup; every thread
// gets the value.  tab: the 256-entry byte table in LDS; scratch: LDS uint32[16].
// The caller has made msg visible to the workgroup.
__device__ inline uint32_t block_crc32(const uint8_t *msg, int64_t len, const uint32_t *tab,
                                       uint32_t *scratch) {
    const int t = threadIdx.x, T = kFrameThreads;
    const int64_t piece = (len + T - 1) / T;
    const int64_t end = len - (int64_t)(T - 1 - t) * piece;  // pieces are aligned to the end
    const int64_t begin = max(end - piece, (int64_t)0);
    uint32_t crc = 0;
    for (int64_t i0 = begin; i0 < end; i0 += kCrcLoads) {
        uint32_t b[kCrcLoads];  // the loads first: they do not wait for the register
#pragma unroll
        for (int j = 0; j < kCrcLoads; ++j) b[j] = (i0 + j < end) ? msg[i0 + j] : 0u;
#pragma unroll
        for (int j = 0; j < kCrcLoads; ++j) {
            if (i0 + j >= end) break;
            if (i0 + j < 4) b[j] ^= 0xffu;  // the register's initial FFFFFFFF
            crc = tab[(crc ^ b[j]) & 0xffu] ^ (crc >> 8);
        }
    }
    if (crc) {  // times x^(8 * bytes after this piece)
        uint64_t after = (uint64_t)(len - max(end, (int64_t)0));
        for (int k = 0; after; ++k, after >>= 1)
            if (after & 1u) crc = gf_mul(crc, kCrcPowers.v[k]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, o);
    __syncthreads();
    if (lane_id() == 0) scratch[wave_id()] = crc;
    __syncthreads();
    uint32_t r = 0;
    for (int w = 0; w < T / VD_WAVE; ++w) r ^= scratch[w];
    return ~r;
}

__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

__global__ __launch_bounds__(kFrameThreads) void png_frame_kernel(
    int H, int W, const uint8_t *__restrict__ palette, uint8_t *out, int64_t cap,
    const StripMeta *__restrict__ meta, int ns, int32_t *__restrict__ lengths) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t off[kPngMaxStrips + 1];  // first byte of strip s in the joined stream
    __shared__ uint32_t scratch[16];
    __shared__ uint32_t sums[2 * (kFrameThreads / VD_WAVE)];
    const int f = blockIdx.x, t = threadIdx.x;
    uint8_t *o = out + (int64_t)f * cap;
    const StripMeta *fm = meta + (int64_t)f * ns;
    const uint32_t slot = (uint32_t)strip_cap(kStripRows, W);
    if (t < 256) {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
        tab[t] = c;
    }
    // strip offsets: thread t owns strips [t * per, (t + 1) * per)
    const int per = (ns + kFrameThreads - 1) / kFrameThreads;
    const int s0 = min(t * per, ns), s1 = min(s0 + per, ns);
    uint32_t mine = 0, a = 0, b = 0;
    for (int s = s0; s < s1; ++s) {
        mine += min(fm[s].len, slot);
        a += fm[s].a;  // at most 2048 values below 65521
        b += fm[s].b;
    }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, d);
        if (lane_id() >= d) incl += v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a += (uint32_t)__shfl_xor((int)a, d);
        b += (uint32_t)__shfl_xor((int)b, d);
    }
    if (lane_id() == 63) scratch[wave_id()] = incl;
    if (lane_id() == 0) {
        sums[2 * wave_id()] = a;
        sums[2 * wave_id() + 1] = b;
    }
    __syncthreads();
    uint32_t base = 0, n = 0;
    a = b = 0;
    for (int w = 0; w < kFrameThreads / VD_WAVE; ++w) {
        if (w < wave_id()) base += scratch[w];
        n += scratch[w];
        a += sums[2 * w];
        b += sums[2 * w + 1];
    }
    {
        uint32_t at = base + incl - mine;
        for (int s = s0; s < s1; ++s) {
            off[s] = at;
            at += min(fm[s].len, slot);
        }
        if (t == 0) off[ns] = n;
    }
    __syncthreads();

    // join the strips: destination byte d of the stream comes from its strip's slot,
    // which lies at or after d; a chunk's reads all precede its writes, and a later
    // chunk's sources lie after everything an earlier chunk wrote
    uint8_t *data = o + kPngHead;
    const uint32_t chunk = kFrameThreads * kMoveBytes;
    for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t d0 = c0 + (uint32_t)t * kMoveBytes;
        uint8_t v[kMoveBytes];
        if (d0 < n) {
            int lo = 0, hi = ns;  // the strip holding d0: off[lo] <= d0 < off[lo + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= d0) lo = mid; else hi = mid;
            }
            int s = lo;
            int64_t src[kMoveBytes];  // the addresses first, then all loads together
#pragma unroll
            for (int i = 0; i < kMoveBytes; ++i) {
                const uint32_t d = min(d0 + i, n - 1u);
                while (d >= off[s + 1]) ++s;
                src[i] = (int64_t)s * slot + (d - off[s]);
            }
#pragma unroll
            for (int i = 0; i < kMoveBytes; ++i) v[i] = data[src[i]];
        }
        __syncthreads();
        if (d0 < n) {
#pragma unroll
            for (int i = 0; i < kMoveBytes; ++i)
                if (d0 + i < n) data[d0 + i] = v[i];
        }
        __syncthreads();
    }

    // the constant parts, the palette and the Adler-32
    const int64_t total_raw = (int64_t)H * (W + 1);
    for (int i = t; i < 768; i += kFrameThreads) o[41 + i] = palette[i];
    if (t == 0) {
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
        for (int i = 0; i < 8; ++i) o[i] = sig[i];
        put_be32(o + 8, 13u);
        o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
        put_be32(o + 16, (uint32_t)W);
        put_be32(o + 20, (uint32_t)H);
        o[24] = 8; o[25] = 3; o[26] = 0; o[27] = 0; o[28] = 0;  // depth, colour type 3, ...
        put_be32(o + 33, 768u);
        o[37] = 'P'; o[38] = 'L'; o[39] = 'T'; o[40] = 'E';
        put_be32(o + 813, n + 6u);  // zlib header, stream, Adler-32
        o[817] = 'I'; o[818] = 'D'; o[819] = 'A'; o[820] = 'T';
        o[821] = 0x78; o[822] = 0x01;
        const uint32_t A = (1u + a) % kAdlerMod;
        const uint32_t B = (uint32_t)((total_raw % kAdlerMod + b) % kAdlerMod);
        put_be32(data + n, (B << 16) | A);
        uint8_t *e = data + n + 8;  // after the IDAT CRC
        put_be32(e, 0u);
        e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
        put_be32(e + 8, 0xae426082u);
        lengths[f] = (int32_t)(kPngHead + n + kPngTail);
    }
    __syncthreads();
    const uint32_t c_ihdr = block_crc32(o + 12, 17, tab, scratch);
    const uint32_t c_plte = block_crc32(o + 37, 772, tab, scratch);
    const uint32_t c_idat = block_crc32(o + 817, (int64_t)n + 10, tab, scratch);
    if (t == 0) {
        put_be32(o + 29, c_ihdr);
        put_be32(o + 809, c_plte);
        put_be32(data + n + 4, c_idat);
    }
}

int launch_label_pngs(const uint8_t *labels, int F, int H, int W, const uint8_t *palette,
                      uint8_t *out, size_t cap, int32_t *lengths, void *workspace,
                      size_t workspace_bytes, hipStream_t s) {
    const size_t bound = label_png_bound(H, W);
    if (bound == 0 || F > kPngMaxF) return VD_ERR_SHAPE;
    if (cap < bound || cap > ((size_t)1 << 40)) return VD_ERR_ARG;
    if (workspace_bytes < label_pngs_workspace_bytes(F, H, W)) return VD_ERR_WORKSPACE;
    if (!workspace || ((uintptr_t)workspace & 15u)) return VD_ERR_ARG;
    const int ns = (H + kStripRows - 1) / kStripRows;
    StripMeta *meta = (StripMeta *)workspace;
    // the image holds a whole slot, rounded to words, and one word for a code's upper half
    const int img_words = (int)((strip_cap(kStripRows, W) + 3) / 4) + 1;
    hipLaunchKernelGGL(png_strip_kernel, dim3(ns, F), dim3(VD_WAVE), (size_t)img_words * 4, s,
                       labels, H, W, out, (int64_t)cap, meta, img_words);
    if (hipGetLastError() != hipSuccess) return VD_ERR_LAUNCH;
    hipLaunchKernelGGL(png_frame_kernel, dim3(F), dim3(kFrameThreads), 0, s, H, W, palette, out,
                       (int64_t)cap, meta, ns, lengths);
    return hipGetLastError() == hipSuccess ? VD_OK : VD_ERR_LAUNCH;
}

}  // namespace vd
