// fosvos_jpeg_decode: baseline JPEG files -> uint8 frames on the device, byte for byte what util/jpeg_read.py states (and,
// on the inputs of tests/jpeg_read_cases.py, what libjpeg-turbo decodes).  Three launches on the caller's stream:
//
//   k_jpegd_entropy  one wave per restart interval ("segment"; a file without DRI is one).  The wave runs the serial
//                    Huffman decode of jpeg_entropy.h on wave-uniform state (bit buffer, position, predictors); lane k holds
//                    natural-order coefficient k of the current block, and a finished block leaves as ONE 128-byte store.
//                    The file's bytes reach the wave 256 at a time (a dword a lane, every byte bounds-checked against the
//                    segment) and are handed round with v_readlane; the eight Huffman tables of the file are built in LDS
//                    (a 9-bit first-level lookup + the canonical walk for longer codes).
//   k_jpegd_idct     32 blocks a workgroup, thread = (block, row) -> (block, column) -> (block, row) through LDS:
//                    dequantisation, libjpeg's slow-integer inverse DCT in wrap-around 32-bit arithmetic, range limit,
//                    8 bytes a thread into the padded component planes.  A coefficient x quant outside +-32767 counts as 0
//                    and raises the workgroup's flag (status 5).
//   k_jpegd_color    a pixel a thread: h2v2 "fancy" chroma upsampling from the real chroma samples, the 16-bit fixed-point
//                    YCbCr -> RGB rows, BGR interleave (grey: a copy of the luma plane's corner).  Its first workgroup of a
//                    file folds the segment statuses and IDCT flags into the file's status word.
//
// Nothing is written but the file's own coefficient blocks, planes, status words (all inside the workspace), frame and
// status.  The segment table lives in device memory, so the host cannot check its rows: the entropy kernel does, and a row
// that points outside the bytes or the MCU grid decodes nothing and reports status 1.
#include "common.hpp"
#include "jpeg_entropy.h"

using namespace fosvos;
using namespace fosvos_jpegd;

namespace {

constexpr int kSegInts = 5;  // a row of the segment table: file, byte offset, byte length, first MCU, MCU count
constexpr int kIdctBlocks = 32, kIdctThreads = 256, kColorThreads = 256;

struct DecodeLayout {
    Geometry g;
    int plane_w[3], plane_h[3];
    int64_t plane_off[3], plane_bytes;         // per file
    int idct_groups;                           // per file
    size_t off_planes, off_seg_status, off_flags, total;
};

DecodeLayout decode_layout(int N, int H, int W, int comps, bool s420) {
    DecodeLayout L;
    L.g = geometry(H, W, comps, s420 ? 1 : 0);
    int64_t off = 0;
    for (int c = 0; c < 3; ++c) {
        const int f = (L.g.s420 && c == 0) ? 2 : 1;
        L.plane_w[c] = L.g.cols[c] * 8, L.plane_h[c] = f * L.g.mh * 8;
        L.plane_off[c] = off;
        if (c < comps) off += (int64_t)L.plane_w[c] * L.plane_h[c];
    }
    L.plane_bytes = off;
    L.idct_groups = (L.g.blocks + kIdctBlocks - 1) / kIdctBlocks;
    L.off_planes = (size_t)N * L.g.blocks * 128;
    L.off_seg_status = L.off_planes + (size_t)N * (size_t)L.plane_bytes;
    L.off_flags = L.off_seg_status + (size_t)N * L.g.mh * L.g.mw * sizeof(int32_t);
    L.total = L.off_flags + (size_t)N * L.idct_groups * sizeof(int32_t);
    return L;
}

bool decode_shape_ok(int N, int H, int W, int components, int sampling) {
    return N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 65535 && W <= 65535 && (components == 1 || components == 3) &&
           (sampling == 444 || sampling == 420) && !(sampling == 420 && components == 3 && W < 5);
}

// ---------------------------------------------------------------------------------------------- entropy decode
// The segment's bytes, 256 at a time: lane l holds bytes 4l .. 4l+3 of the chunk, zero beyond the segment's end.
struct WaveBytes {
    const uint8_t *p;
    uint32_t len, chunk, word;
    int lane;
    __device__ void load(uint32_t c) {
        chunk = c;
        const uint32_t base = c * 256u + 4u * (uint32_t)lane;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (base + j < len) w |= (uint32_t)p[base + j] << (8 * j);
        word = w;
    }
    __device__ uint32_t get(uint32_t i) {  // i is the same in every lane
        if (i >= len) return 0;
        const uint32_t c = i >> 8;
        if (c != chunk) load(c);
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)word, (int)((i >> 2) & 63u));
        return (w >> (8 * (i & 3u))) & 255u;
    }
};

// The current block: lane k holds natural-order coefficient k and knows that coefficient's zigzag position, so a put is
// one compare and one select - no table is read on the decode's path
struct WaveBlock {
    int16_t *coef;  // the file's blocks
    int lane;
    int position;
    int v;
    __device__ void put(int zigzag, int16_t value) {
        if (position == zigzag) v = value;
    }
    __device__ void store(int index) {
        coef[(size_t)index * 64 + lane] = (int16_t)v;
        v = 0;
    }
    __device__ void zero(int index) {
        v = 0;
        store(index);
    }
};

__global__ __launch_bounds__(64) void k_jpegd_entropy(const uint8_t *__restrict__ bytes, uint32_t n_bytes,
                                                      const int32_t *__restrict__ segments, const FileTables *__restrict__ tables,
                                                      int N, Geometry g, int16_t *__restrict__ coef,
                                                      int32_t *__restrict__ seg_status) {
    __shared__ Huff huff[kSlots];
    __shared__ uint8_t sel[8];
    const int lane = threadIdx.x;
    const int seg = blockIdx.x;
    const int32_t *row = segments + (size_t)seg * kSegInts;
    const int file = (int)FOSVOS_WAVE_UNIFORM(row[0]);
    const int64_t off = (int32_t)FOSVOS_WAVE_UNIFORM(row[1]), len = (int32_t)FOSVOS_WAVE_UNIFORM(row[2]);
    const int64_t first = (int32_t)FOSVOS_WAVE_UNIFORM(row[3]), count = (int32_t)FOSVOS_WAVE_UNIFORM(row[4]);
    if (file < 0 || file >= N || off < 0 || len < 0 || off + len > (int64_t)n_bytes || first < 0 || count < 0 ||
        first + count > (int64_t)g.mh * g.mw) {
        if (lane == 0) seg_status[seg] = kBytes;
        return;
    }
    const FileTables &ft = tables[file];
    if (lane < kSlots) huff_codes(ft.dht[lane], huff[lane]);
    if (lane < 3) sel[lane] = ft.dc_slot[lane], sel[4 + lane] = ft.ac_slot[lane];
    for (int s = 0; s < kSlots; ++s) huff_fill(ft.dht[s], huff[s], lane, 64);
    __syncthreads();
    for (int s = 0; s < kSlots; ++s) huff_lut(huff[s], lane, 64);
    __syncthreads();
    WaveBytes src{bytes + off, (uint32_t)len, 0xFFFFFFFFu, 0u, lane};
    int position = 0;
    for (int k = 0; k < 64; ++k)
        if (zigzag_natural(k) == lane) position = k;
    WaveBlock sink{coef + (size_t)file * g.blocks * 64, lane, position, 0};
    const int status = decode_segment(src, (uint32_t)len, huff, sel, sel + 4, g, (int)first, (int)count, sink);
    if (lane == 0) seg_status[seg] = status;
}

// ---------------------------------------------------------------------------------------------- inverse DCT
// One pass over d[0..7] in wrap-around arithmetic (unsigned: no overflow is undefined), descaled by `shift` bits
__device__ __forceinline__ void idct_pass(const int32_t (&in)[8], int32_t (&out)[8], int shift) {
    typedef uint32_t u;
    const u d0 = in[0], d1 = in[1], d2 = in[2], d3 = in[3], d4 = in[4], d5 = in[5], d6 = in[6], d7 = in[7];
    u z1 = (d2 + d6) * 4433u;
    const u t2 = z1 - d6 * 15137u, t3 = z1 + d2 * 6270u;
    const u t0 = (d0 + d4) << 13, t1 = (d0 - d4) << 13;
    const u e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
    u a0 = d7, a1 = d5, a2 = d3, a3 = d1;
    z1 = a0 + a3;
    u z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const u z5 = (z3 + z4) * 9633u;
    a0 *= 2446u, a1 *= 16819u, a2 *= 25172u, a3 *= 12299u;
    z1 *= (u)-7373, z2 *= (u)-20995;
    z3 = z3 * (u)-16069 + z5, z4 = z4 * (u)-3196 + z5;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    const u o[8] = {e0 + a3, e1 + a2, e2 + a1, e3 + a0, e3 - a0, e2 - a1, e1 - a2, e0 - a3};
    const u half = 1u << (shift - 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = (int32_t)(o[i] + half) >> shift;
}

__device__ __forceinline__ uint32_t range_limit(int32_t v) {
    const int32_t m = v & 1023;
    return m < 128 ? (uint32_t)(m + 128) : m < 512 ? 255u : m < 896 ? 0u : (uint32_t)(m - 896);
}

struct PlaneGeom {
    int w[3];
    int64_t off[3], bytes;
};

__global__ __launch_bounds__(kIdctThreads) void k_jpegd_idct(const int16_t *__restrict__ coef,
                                                            const FileTables *__restrict__ tables, Geometry g, PlaneGeom pg,
                                                            uint8_t *__restrict__ planes, int32_t *__restrict__ flags) {
    __shared__ int32_t xs[kIdctBlocks][8][9];  // a padded row: the column pass strides by 9 words
    const int t = threadIdx.x, bl = t >> 3, i = t & 7;
    const int n = blockIdx.y;
    const int b = blockIdx.x * kIdctBlocks + bl;
    const bool live = b < g.blocks;
    const int c = (g.comps == 3 && live) ? (b >= g.first[2] ? 2 : b >= g.first[1] ? 1 : 0) : 0;
    int bad = 0;
    if (live) {
        // row i of the block: eight coefficients, eight quantisers
        const uint4 raw = *reinterpret_cast<const uint4 *>(coef + ((size_t)n * g.blocks + b) * 64 + i * 8);
        const uint2 qraw = *reinterpret_cast<const uint2 *>(tables[n].quant[c] + i * 8);
        const uint32_t cw[4] = {raw.x, raw.y, raw.z, raw.w};
        const uint32_t qw[2] = {qraw.x, qraw.y};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int32_t cv = (int16_t)(cw[k >> 1] >> (16 * (k & 1)));
            const int32_t q = (int32_t)((qw[k >> 2] >> (8 * (k & 3))) & 255u);
            int32_t x = cv * q;
            if (x > 32767 || x < -32767) bad = 1, x = 0;
            xs[bl][i][k] = x;
        }
    }
    const int any_bad = __syncthreads_or(bad);
    if (t == 0) flags[(size_t)n * gridDim.x + blockIdx.x] = any_bad;
    int32_t d[8], o[8];
    if (live) {  // column i
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = xs[bl][k][i];
        idct_pass(d, o, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) xs[bl][k][i] = o[k];
    }
    __syncthreads();
    if (live) {  // row i
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = xs[bl][i][k];
        idct_pass(d, o, 18);
        uint2 px;
        px.x = range_limit(o[0]) | range_limit(o[1]) << 8 | range_limit(o[2]) << 16 | range_limit(o[3]) << 24;
        px.y = range_limit(o[4]) | range_limit(o[5]) << 8 | range_limit(o[6]) << 16 | range_limit(o[7]) << 24;
        const int local = b - g.first[c];
        const int brow = local / g.cols[c], bcol = local - brow * g.cols[c];
        uint8_t *dst = planes + (size_t)n * pg.bytes + pg.off[c] + (size_t)(brow * 8 + i) * pg.w[c] + (size_t)bcol * 8;
        *reinterpret_cast<uint2 *>(dst) = px;
    }
}

// ---------------------------------------------------------------------------------------------- upsampling and colour
// 3 * near + far of chroma column cx for output row y (jpeg_read.upsample_420)
__device__ __forceinline__ int chroma_s(const uint8_t *__restrict__ plane, int pw, int ch, int y, int cx) {
    const int r = y >> 1;
    int far = (y & 1) ? r + 1 : r - 1;
    far = far < 0 ? 0 : (far > ch - 1 ? ch - 1 : far);
    return 3 * (int)plane[(size_t)r * pw + cx] + (int)plane[(size_t)far * pw + cx];
}
__device__ __forceinline__ int chroma_420(const uint8_t *__restrict__ plane, int pw, int ch, int cw, int y, int x) {
    const int cx = x >> 1;
    const int s = chroma_s(plane, pw, ch, y, cx);
    if (x & 1) {
        const int nb = cx + 1 < cw ? chroma_s(plane, pw, ch, y, cx + 1) : s;
        return (3 * s + nb + 7) >> 4;
    }
    const int nb = cx > 0 ? chroma_s(plane, pw, ch, y, cx - 1) : s;
    return (3 * s + nb + 8) >> 4;
}
__device__ __forceinline__ uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(kColorThreads) void k_jpegd_color(const uint8_t *__restrict__ planes, PlaneGeom pg, int H, int W,
                                                              int comps, int s420, const FileTables *__restrict__ tables,
                                                              const int32_t *__restrict__ seg_status, int n_segments,
                                                              const int32_t *__restrict__ flags, int idct_groups,
                                                              uint8_t *__restrict__ frames, int32_t *__restrict__ status) {
    __shared__ int s_status;
    const int n = blockIdx.y, t = threadIdx.x;
    if (blockIdx.x == 0) {  // the file's status: the smallest non-zero one of its segments, else 5 where an IDCT flag is up
        if (t == 0) s_status = 0x7FFFFFFF;
        __syncthreads();
        int64_t first = tables[n].seg_first, count = tables[n].seg_count;
        first = first < 0 ? 0 : first;
        count = count < 0 ? 0 : count;
        const int64_t end = first + count > (int64_t)n_segments ? (int64_t)n_segments : first + count;
        int mine = 0x7FFFFFFF;
        for (int64_t s = first + t; s < end; s += kColorThreads) {
            const int v = seg_status[s];
            if (v != 0 && v < mine) mine = v;
        }
        for (int k = t; k < idct_groups; k += kColorThreads)
            if (flags[(size_t)n * idct_groups + k] != 0 && kRange < mine) mine = kRange;
        if (mine != 0x7FFFFFFF) atomicMin(&s_status, mine);
        __syncthreads();
        if (t == 0) status[n] = s_status == 0x7FFFFFFF ? 0 : s_status;
    }
    const int64_t p = (int64_t)blockIdx.x * kColorThreads + t;
    if (p >= (int64_t)H * W) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const uint8_t *base = planes + (size_t)n * pg.bytes;
    const int Y = base[pg.off[0] + (size_t)y * pg.w[0] + x];
    if (comps == 1) {
        frames[(size_t)n * H * W + p] = (uint8_t)Y;
        return;
    }
    int cb, cr;
    if (s420) {
        const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
        cb = chroma_420(base + pg.off[1], pg.w[1], ch, cw, y, x);
        cr = chroma_420(base + pg.off[2], pg.w[2], ch, cw, y, x);
    } else {
        cb = base[pg.off[1] + (size_t)y * pg.w[1] + x];
        cr = base[pg.off[2] + (size_t)y * pg.w[2] + x];
    }
    cb -= 128, cr -= 128;
    uint8_t *dst = frames + ((size_t)n * H * W + p) * 3;
    dst[0] = clamp255(Y + ((116130 * cb + 32768) >> 16));
    dst[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    dst[2] = clamp255(Y + ((91881 * cr + 32768) >> 16));
}

}  // namespace

extern "C" size_t fosvos_jpeg_decode_workspace_bytes(int N, int H, int W, int components, int sampling) {
    if (!decode_shape_ok(N, H, W, components, sampling)) return 0;
    return decode_layout(N, H, W, components, sampling == 420).total;
}

extern "C" int fosvos_jpeg_decode(const uint8_t *bytes, size_t n_bytes, const int32_t *segments, int n_segments,
                                  const void *tables, int N, int H, int W, int components, int sampling, uint8_t *frames,
                                  int32_t *status, void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(components == 1 || components == 3, FOSVOS_E_SHAPE, "jpeg_decode: components=%d (1 grey, 3 colour)", components);
    FOSVOS_REQUIRE(sampling == 444 || sampling == 420, FOSVOS_E_ARG, "jpeg_decode: sampling=%d (444 or 420)", sampling);
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 65535 && W <= 65535, FOSVOS_E_SHAPE,
                   "jpeg_decode: N=%d H=%d W=%d (each 1..65535)", N, H, W);
    FOSVOS_REQUIRE(!(sampling == 420 && components == 3 && W < 5), FOSVOS_E_SHAPE,
                   "jpeg_decode: 4:2:0 needs W >= 5, got %d (libjpeg does not smooth narrower chroma rows)", W);
    FOSVOS_REQUIRE(bytes && segments && tables && frames && status && workspace, FOSVOS_E_ARG, "jpeg_decode: null pointer");
    FOSVOS_REQUIRE(n_bytes > 0 && n_bytes <= (size_t)INT32_MAX, FOSVOS_E_ARG, "jpeg_decode: n_bytes=%zu (1..2^31-1)", n_bytes);
    const DecodeLayout L = decode_layout(N, H, W, components, sampling == 420);
    FOSVOS_REQUIRE(n_segments >= N && (int64_t)n_segments <= (int64_t)N * L.g.mh * L.g.mw, FOSVOS_E_ARG,
                   "jpeg_decode: n_segments=%d (between a file and an MCU each: %d..%lld)", n_segments, N,
                   (long long)N * L.g.mh * L.g.mw);
    FOSVOS_REQUIRE(((uintptr_t)segments & 3) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)tables & 7) == 0 &&
                       ((uintptr_t)workspace & 15) == 0,
                   FOSVOS_E_ARG, "jpeg_decode: segments and status must be 4-byte, tables 8-byte, the workspace 16-byte aligned");
    FOSVOS_REQUIRE(workspace_bytes >= L.total, FOSVOS_E_WORKSPACE, "jpeg_decode: workspace %zu B < %zu B", workspace_bytes, L.total);
    FOSVOS_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = reinterpret_cast<uint8_t *>(workspace);
    int16_t *coef = reinterpret_cast<int16_t *>(ws);
    uint8_t *planes = ws + L.off_planes;
    int32_t *seg_status = reinterpret_cast<int32_t *>(ws + L.off_seg_status);
    int32_t *flags = reinterpret_cast<int32_t *>(ws + L.off_flags);
    const FileTables *ft = reinterpret_cast<const FileTables *>(tables);
    PlaneGeom pg;
    for (int c = 0; c < 3; ++c) pg.w[c] = L.plane_w[c], pg.off[c] = L.plane_off[c];
    pg.bytes = L.plane_bytes;

    FOSVOS_PROF("k_jpegd_entropy", stream, 0.0);
    hipLaunchKernelGGL(k_jpegd_entropy, dim3((unsigned)n_segments), dim3(64), 0, st, bytes, (uint32_t)n_bytes, segments, ft, N, L.g,
                       coef, seg_status);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_jpegd_idct", stream, 0.0);
    hipLaunchKernelGGL(k_jpegd_idct, dim3((unsigned)L.idct_groups, (unsigned)N), dim3(kIdctThreads), 0, st, coef, ft, L.g, pg, planes,
                       flags);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_jpegd_color", stream, 0.0);
    const unsigned tiles = (unsigned)(((int64_t)H * W + kColorThreads - 1) / kColorThreads);
    hipLaunchKernelGGL(k_jpegd_color, dim3(tiles, (unsigned)N), dim3(kColorThreads), 0, st, planes, pg, H, W, components, L.g.s420,
                       ft, seg_status, n_segments, flags, L.idct_groups, frames, status);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
