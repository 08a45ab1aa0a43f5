// The front and back end of streaming inference (src/run_webcam.py:81-133, apply_network): a raw uint8 BGR camera frame
// becomes the net's fp32 NCHW input, and the net's logits become the uint8 frame that is shown.  util/frame_overlay.py states
// both in numpy; the boolean modes and the prep are compared with it bit for bit.
//
// fosvos_frame_prep, one launch:
//   k_frame_prep   image[n][c][y][x] = float(frames[n][y][xs][c]) - mean[c], xs = x or (mirror) W-1-x.  3 B read, 12 B written
//                  per pixel; one rounding (the subtraction), so the result is numpy's float32(byte) - float32(mean).
// fosvos_overlay, one launch:
//   k_overlay      mode 0/1: out[n][y][x][:] = frames[n][y][xs][:] with channel `channel` replaced by
//                  trunc(min(byte + (alpha * 255) * p, 255)) in fp64, p = (logit >= 0) or the fp64 sigmoid; mode 2/3: out[n][y][x]
//                  = 0 / 255 or (uint8)(255 p + 0.5).  7 B read, 3 B written per pixel (4 B and 1 B in the mask modes).
//
// Both kernels are byte movers with the same partition.  The pixels form SEGMENTS that are contiguous on both sides: without
// mirror a whole frame (HWC bytes and every CHW plane are flat), with mirror one row (its bytes are read backwards).  A
// thread takes a GROUP of 16 consecutive output pixels of a segment: 48 frame bytes (three 16-byte loads), 16 logits (four),
// and 64-byte runs per output plane or 48 / 16 output bytes.  The groups of a segment start where its fp32 side (the image
// plane, the logits) crosses a 16-byte boundary, so those accesses - most of the bytes - are aligned whatever the base
// pointer and the row length are; the byte side is then wherever it falls, and its 16-byte accesses are declared with the
// alignment they have (1 for bytes, 4 for floats): the compiler picks instructions that are legal for it.  The pixels in
// front of a segment's first group and behind its last full one (fewer than 16 each) go through a scalar loop.
// In a mirrored group the 16 source pixels are the group's mirror image, so the same three loads serve, and the reversal
// is a compile-time permutation of register bytes.
//
// The net at a size of its own (opt-in; util/frame_resample.py states both): frames of [Hf,Wf], net of [Hn,Wn] <= the frame.
// fosvos_frame_prep_scaled, one launch:
//   k_frame_prep_scaled  image[n][c][i][j] = float(double(S) / double(Hf Wf)) - mean[c], S the exact area sum in integers:
//                        S = sum_y sum_x wy[i][y] wx[j][x] byte, w[j][s] = the overlap of [s n_dst, (s+1) n_dst) with
//                        [j n_src, (j+1) n_src).  A workgroup owns 4 output rows times 16 16-byte cells of an image row,
//                        stages the source byte rows under them in LDS and walks them; a thread owns one cell of one plane.
// fosvos_overlay_scaled, one launch:
//   k_overlay_scaled     k_overlay with the logit of an output pixel gathered from the [Hn,Wn] map: bilinear at half-pixel
//                        centres with integer weights, in fp64, as 4 Hf Wf times the logit (its sign is the boolean mask).
//
// Several objects a stream (opt-in; util/object_overlay.py states both): the K logit maps of K per-object nets, pointers by value.
// fosvos_overlay_objects, one launch:
//   k_overlay_objects         k_overlay's partition anchored on map 0; a thread takes its 16 logits from each of the K maps in
//                             turn and keeps (best value, label) per pixel - the rule of fosvos_merge_objects - then blends
//                             every labelled pixel towards its palette colour: b + alpha (col - b) in fp64, rounded half up.
//                             4 K + 3 B read, 3 B written per pixel; no label map in between.
// fosvos_overlay_objects_scaled, one launch:
//   k_overlay_objects_scaled  k_overlay_scaled's thread map; the taps of a pixel are taken once and applied to all K maps,
//                             the rule then runs on the fp64 values.  Mode 0 the overlay, mode 1 the label map.
#include <math.h>

#include "common.hpp"

// the fp64 expressions are the host's, operation for operation
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kStreamThreads = 256;
constexpr int kGroup = 16;  // pixels a thread takes

struct MeanBGR {
    float v[3];
};
// 16 bytes at the alignment the data has, not the one a uint4 / float4 would promise
struct __attribute__((packed)) bytes16 {
    uint32_t w[4];
};
struct __attribute__((packed, aligned(4))) floats4 {
    float v[4];
};

// where thread `gid` works: segment `seg`, output pixels [qa, qb) of it.  `slots` = L / 16 + 2 threads a segment: slot 0 is
// the head [0, k0), slot j >= 1 the group that starts at k0 + 16 (j - 1) (cut at L, possibly empty).
struct Span {
    int64_t seg, qa, qb;
};
__device__ __forceinline__ int64_t segment_of(int64_t gid, int64_t slots) { return gid / slots; }
__device__ __forceinline__ Span span_at(int64_t gid, int64_t seg, int64_t slots, int64_t L, int k0) {
    const int j = (int)(gid - seg * slots);
    Span s;
    s.seg = seg;
    if (j == 0) {
        s.qa = 0;
        s.qb = min((int64_t)k0, L);
    } else {
        s.qa = min(k0 + (int64_t)kGroup * (j - 1), L);
        s.qb = min(s.qa + kGroup, L);
    }
    return s;
}
__device__ __forceinline__ Span span_of(int64_t gid, int64_t seg, int64_t slots, int64_t L, const float *anchor) {
    const int k0 = (int)((16u - ((unsigned)(uintptr_t)anchor & 15u)) & 15u) >> 2;  // floats up to the 16-byte boundary
    return span_at(gid, seg, slots, L, k0);
}

__device__ __forceinline__ void load48(const uint8_t *__restrict__ p, uint32_t (&w)[12]) {
    const bytes16 *__restrict__ v = reinterpret_cast<const bytes16 *>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bytes16 t = v[k];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[4 * k + i] = t.w[i];
    }
}
// byte `i` of a register array (i is a constant after unrolling: one bit-field extract, or none inside a convert)
template <int N>
__device__ __forceinline__ uint32_t byte_at(const uint32_t (&w)[N], int i) {
    return (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
}

// ------------------------------------------------------------------------------------------ frame_prep
// L pixels a segment, R segments a frame (1, or H rows), plane = H * W
template <bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_frame_prep(const uint8_t *__restrict__ frames, float *__restrict__ image,
                                                               int64_t L, int R, int64_t plane, int64_t slots, int64_t total,
                                                               MeanBGR mean) {
    const int64_t gid = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (gid >= total) return;
    const int64_t seg = segment_of(gid, slots);
    const uint8_t *__restrict__ src = frames + seg * 3 * L;
    float *__restrict__ dst = image + (seg / R) * 3 * plane + (seg % R) * L;
    const Span s = span_of(gid, seg, slots, L, dst);
    if (s.qb - s.qa == kGroup) {
        uint32_t w[12];
        load48(src + 3 * (MIRROR ? L - kGroup - s.qa : s.qa), w);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            floats4 *__restrict__ o = reinterpret_cast<floats4 *>(dst + c * plane + s.qa);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                floats4 t;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int px = MIRROR ? kGroup - 1 - (4 * k + i) : 4 * k + i;
                    t.v[i] = (float)byte_at(w, 3 * px + c) - mean.v[c];
                }
                o[k] = t;
            }
        }
    } else {
        for (int64_t q = s.qa; q < s.qb; ++q) {
            const int64_t sp = MIRROR ? L - 1 - q : q;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * plane + q] = (float)src[3 * sp + c] - mean.v[c];
        }
    }
}

// ------------------------------------------------------------------------------------------ frame_prep_scaled
constexpr int kScaleRows = 4;    // output rows a workgroup owns
constexpr int kScaleCells = 16;  // 16-byte cells of an image row a workgroup owns: 64 output columns
constexpr int kScaleThreads = kScaleRows * 3 * kScaleCells;
constexpr int kScaleChunkPx = 1024;      // the most source pixels of a row that are staged at once
constexpr int kScaleStageBytes = 32768;  // the most LDS a workgroup stages in
constexpr int kMaxSide = 8192;           // Hf, Wf: every product of two sides, times 4, stays inside int32

struct ScaleGeom {
    int Hf, Wf, Hn, Wn;
    int pitch, rows;    // the stage: `rows` source rows of `pitch` bytes (a multiple of 16)
    int tiles, strips;  // workgroups along a row, along a column
};
// w[j][s] of util/frame_resample.box_weights
__device__ __forceinline__ int overlap(int s, int j, int n_src, int n_dst) {
    return max(0, min((s + 1) * n_dst, (j + 1) * n_src) - max(s * n_dst, j * n_src));
}

// Thread (row il, plane c, cell q) owns the 16-byte cell m = 16 tile + q of image row (n, c, i0 + il): columns [4m - o, 4m -
// o + 4) cut to [0, Wn), o = the floats the row's start lies behind a 16-byte boundary - so a whole cell is one aligned
// store.  The workgroup walks the source rows under its 4 output rows, `g.rows` at a time, and the source columns under its
// cells, pitch / 3 at a time - the window of an output pixel has no bound (Hn = 1 averages a column), so neither walk may
// be assumed to be one step - and every thread adds the staged part of its windows: S is a sum, any order gives it exactly.
template <bool MIRROR>
__global__ __launch_bounds__(kScaleThreads) void k_frame_prep_scaled(const uint8_t *__restrict__ frames,
                                                                     float *__restrict__ image, ScaleGeom g,
                                                                     int64_t frame_bytes, MeanBGR mean) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    const int Hf = g.Hf, Wf = g.Wf, Hn = g.Hn, Wn = g.Wn;
    const int tile = (int)(blockIdx.x % g.tiles), strip = (int)((blockIdx.x / g.tiles) % g.strips);
    const int64_t n = blockIdx.x / ((unsigned)g.tiles * g.strips);
    const int q = threadIdx.x % kScaleCells, c = (threadIdx.x / kScaleCells) % 3, il = threadIdx.x / (3 * kScaleCells);
    // the workgroup's output rows and columns (whatever o is), and the source rows and columns under them
    const int i0 = strip * kScaleRows, i1 = min(i0 + kScaleRows, Hn);
    const int j0 = max(4 * kScaleCells * tile - 3, 0), j1 = min(4 * kScaleCells * (tile + 1), Wn);
    const int ys0 = i0 * Hf / Hn, ys1 = (i1 * Hf + Hn - 1) / Hn;
    const int xs0 = (MIRROR ? Wn - j1 : j0) * Wf / Wn, xs1 = ((MIRROR ? Wn - j0 : j1) * Wf + Wn - 1) / Wn;
    // the thread's row, cell and windows
    const int i = i0 + il;
    const bool live = i < Hn;
    float *__restrict__ rowp = image + ((n * 3 + c) * Hn + (live ? i : 0)) * Wn;
    const int col0 = 4 * (kScaleCells * tile + q) - (int)(((uintptr_t)rowp >> 2) & 3u);
    const int ylo = live ? i * Hf / Hn : 0, yhi = live ? ((i + 1) * Hf + Hn - 1) / Hn : 0;
    int jj[4], xlo[4], xhi[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int j = col0 + p;
        const bool has = live && j >= 0 && j < Wn;
        jj[p] = has ? (MIRROR ? Wn - 1 - j : j) : 0;
        xlo[p] = has ? jj[p] * Wf / Wn : 0;
        xhi[p] = has ? ((jj[p] + 1) * Wf + Wn - 1) / Wn : 0;
    }
    uint64_t acc[4] = {0, 0, 0, 0};
    const int chunk = g.pitch / 3;
    for (int yb = ys0; yb < ys1; yb += g.rows) {
        const int ye = min(yb + g.rows, ys1);
        for (int xa = xs0; xa < xs1; xa += chunk) {
            const int xb = min(xa + chunk, xs1);
            const int pieces = (3 * (xb - xa) + 15) >> 4;  // 16 pieces <= pitch
            __syncthreads();  // the last stage has been read
            for (int t = threadIdx.x; t < (ye - yb) * pieces; t += kScaleThreads) {
                const int r = t / pieces, k = t - r * pieces;
                const int64_t at = (((n * Hf + yb + r) * Wf) + xa) * 3 + 16 * k;
                uint8_t *d = stage + r * g.pitch + 16 * k;
                if (at + 16 <= frame_bytes) {  // may run into the next row: still the caller's bytes, never used
                    const bytes16 v = *reinterpret_cast<const bytes16 *>(frames + at);
                    *reinterpret_cast<uint4 *>(d) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
                } else {
                    for (int b = 0; b < (int)(frame_bytes - at); ++b) d[b] = frames[at + b];
                }
            }
            __syncthreads();
            for (int y = max(yb, ylo); y < min(ye, yhi); ++y) {
                const uint32_t wy = (uint32_t)overlap(y, i, Hf, Hn);
                const uint8_t *row = stage + (y - yb) * g.pitch + c;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    uint32_t h = 0;  // <= 255 Wf
                    for (int x = max(xlo[p], xa); x < min(xhi[p], xb); ++x)
                        h += (uint32_t)overlap(x, jj[p], Wf, Wn) * row[3 * (x - xa)];
                    acc[p] += (uint64_t)wy * h;  // <= 255 Hf Wf: past 2^32 from 4097 x 4097 on
                }
            }
        }
    }
    if (!live) return;
    const double area = (double)(Hf * Wf);
    const float m = c == 0 ? mean.v[0] : (c == 1 ? mean.v[1] : mean.v[2]);
    float v[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = (float)((double)acc[p] / area) - m;
    if (col0 >= 0 && col0 + 4 <= Wn) {
        *reinterpret_cast<float4 *>(rowp + col0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (col0 + p >= 0 && col0 + p < Wn) rowp[col0 + p] = v[p];
    }
}

// ------------------------------------------------------------------------------------------ overlay
// the new byte of one pixel: `byte` is the frame's value in the overlay's channel (unused in the mask modes); x is the fp32
// logit, or (scaled) the fp64 one - in the boolean modes any positive multiple of it
template <int MODE, typename T>
__device__ __forceinline__ uint32_t level(T x, uint32_t byte, double a255) {
    if (MODE == 2) return x >= T(0) ? 255u : 0u;
    if (MODE == 3) return (uint32_t)(255.0 * sigmoid_f64(x) + 0.5);
    const double p = MODE == 0 ? (x >= T(0) ? 1.0 : 0.0) : sigmoid_f64(x);
    return (uint32_t)fmin((double)byte + a255 * p, 255.0);
}

template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay(const uint8_t *__restrict__ frames,
                                                            const float *__restrict__ logits, uint8_t *__restrict__ out,
                                                            int64_t L, int64_t slots, int64_t total, int channel,
                                                            double a255) {
    constexpr bool kBlend = MODE < 2;
    const int64_t gid = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (gid >= total) return;
    const int64_t seg = segment_of(gid, slots);
    const float *__restrict__ lg = logits + seg * L;
    const Span s = span_of(gid, seg, slots, L, lg);
    const uint8_t *__restrict__ src = kBlend ? frames + seg * 3 * L : nullptr;
    uint8_t *__restrict__ dst = out + seg * (kBlend ? 3 : 1) * L;
    if (s.qb - s.qa == kGroup) {
        float x[kGroup];
        const floats4 *__restrict__ lv = reinterpret_cast<const floats4 *>(lg + s.qa);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const floats4 t = lv[k];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * k + i] = t.v[i];
        }
        if (kBlend) {
            uint32_t w[12], o[12];
            load48(src + 3 * (MIRROR ? L - kGroup - s.qa : s.qa), w);
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = 0;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const int px = MIRROR ? kGroup - 1 - i : i;
                uint32_t b[3] = {byte_at(w, 3 * px), byte_at(w, 3 * px + 1), byte_at(w, 3 * px + 2)};
                const uint32_t v = level<MODE>(x[i], channel == 0 ? b[0] : (channel == 1 ? b[1] : b[2]), a255);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int at = 3 * i + c;
                    o[at >> 2] |= (channel == c ? v : b[c]) << (8 * (at & 3));
                }
            }
            bytes16 *__restrict__ ov = reinterpret_cast<bytes16 *>(dst + 3 * s.qa);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bytes16 t;
#pragma unroll
                for (int i = 0; i < 4; ++i) t.w[i] = o[4 * k + i];
                ov[k] = t;
            }
        } else {
            bytes16 t;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                t.w[k] = level<MODE>(x[4 * k], 0, a255) | (level<MODE>(x[4 * k + 1], 0, a255) << 8) |
                         (level<MODE>(x[4 * k + 2], 0, a255) << 16) | (level<MODE>(x[4 * k + 3], 0, a255) << 24);
            *reinterpret_cast<bytes16 *>(dst + s.qa) = t;
        }
    } else {
        for (int64_t q = s.qa; q < s.qb; ++q) {
            if (kBlend) {
                const int64_t sp = MIRROR ? L - 1 - q : q;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t b = src[3 * sp + c];
                    dst[3 * q + c] = (uint8_t)(channel == c ? level<MODE>(lg[q], b, a255) : b);
                }
            } else {
                dst[q] = (uint8_t)level<MODE>(lg[q], 0, a255);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ overlay_scaled
// Output sample x of an axis with n_src samples in and n_dst out (util/frame_resample.taps): u = (2x+1) n_src + n_dst is the
// numerator moved up by one step, so that it is positive; `at` is its floor less that step (-1: left of the first centre).
struct Walk {
    int at, r;
};
__device__ __forceinline__ Walk walk_from(int x, int n_src, int n_dst) {
    const int u = (2 * x + 1) * n_src + n_dst;
    Walk w;
    w.at = u / (2 * n_dst) - 1;
    w.r = u - (w.at + 1) * (2 * n_dst);
    return w;
}
__device__ __forceinline__ void walk_on(Walk &w, int n_src, int n_dst) {  // x + 1: n_src <= n_dst, one carry at the most
    w.r += 2 * n_src;
    if (w.r >= 2 * n_dst) {
        w.r -= 2 * n_dst;
        ++w.at;
    }
}
struct Tap {
    int i0, i1;
    double w0, w1;
};
__device__ __forceinline__ Tap tap_of(Walk w, int n_src, int n_dst) {
    if (w.at < 0) w.at = 0, w.r = 0;
    if (w.at >= n_src - 1) w.at = n_src - 1, w.r = 0;
    Tap t;
    t.i0 = w.at;
    t.i1 = min(w.at + 1, n_src - 1);
    t.w0 = (double)(2 * n_dst - w.r);
    t.w1 = (double)w.r;
    return t;
}
// 4 Hf Wf times the logit of the output pixel whose column taps are tx, in the host's order
__device__ __forceinline__ double logit_up(const float *__restrict__ a0, const float *__restrict__ a1, const Tap &tx,
                                           const Tap &ty) {
    const double top = (double)a0[tx.i0] * tx.w0 + (double)a0[tx.i1] * tx.w1;
    const double bot = (double)a1[tx.i0] * tx.w0 + (double)a1[tx.i1] * tx.w1;
    return top * ty.w0 + bot * ty.w1;
}

// k_overlay's thread map with rows as the segments; the groups of a row start where the OUTPUT row crosses a 16-byte boundary
// (the logits are gathered, four floats a pixel out of a map that stays in L2, so they have no aligned side to offer).
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_scaled(const uint8_t *__restrict__ frames,
                                                                   const float *__restrict__ logits, uint8_t *__restrict__ out,
                                                                   int Hf, int Wf, int Hn, int Wn, int64_t slots, int64_t total,
                                                                   int channel, double a255) {
    constexpr bool kBlend = MODE < 2;
    constexpr bool kSoft = (MODE & 1) != 0;
    const int64_t gid = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (gid >= total) return;
    const int64_t seg = segment_of(gid, slots), L = Wf;
    const int64_t n = seg / Hf;
    const int y = (int)(seg - n * Hf);
    const uint8_t *__restrict__ src = kBlend ? frames + seg * 3 * L : nullptr;
    uint8_t *__restrict__ dst = out + seg * (kBlend ? 3 : 1) * L;
    // pixels up to the boundary: k0 (or 3 k0, 3 * 11 = 1 mod 16) + the address = 0 mod 16
    const unsigned lead = (16u - ((unsigned)(uintptr_t)dst & 15u)) & 15u;
    const Span s = span_at(gid, seg, slots, L, (int)(kBlend ? (11u * lead) & 15u : lead));
    const Tap ty = tap_of(walk_from(y, Hn, Hf), Hn, Hf);
    const float *__restrict__ a0 = logits + (n * Hn + ty.i0) * Wn;
    const float *__restrict__ a1 = logits + (n * Hn + ty.i1) * Wn;
    const double scale = (double)(4 * Hf * Wf);
    Walk wx = walk_from((int)s.qa, Wn, Wf);
    if (s.qb - s.qa == kGroup) {
        if (kBlend) {
            uint32_t w[12], o[12];
            load48(src + 3 * (MIRROR ? L - kGroup - s.qa : s.qa), w);
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = 0;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const double v = logit_up(a0, a1, tap_of(wx, Wn, Wf), ty);
                walk_on(wx, Wn, Wf);
                const int px = MIRROR ? kGroup - 1 - i : i;
                uint32_t b[3] = {byte_at(w, 3 * px), byte_at(w, 3 * px + 1), byte_at(w, 3 * px + 2)};
                const uint32_t lv =
                    level<MODE>(kSoft ? v / scale : v, channel == 0 ? b[0] : (channel == 1 ? b[1] : b[2]), a255);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int at = 3 * i + c;
                    o[at >> 2] |= (channel == c ? lv : b[c]) << (8 * (at & 3));
                }
            }
            uint4 *__restrict__ ov = reinterpret_cast<uint4 *>(dst + 3 * s.qa);
#pragma unroll
            for (int k = 0; k < 3; ++k) ov[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const double v = logit_up(a0, a1, tap_of(wx, Wn, Wf), ty);
                walk_on(wx, Wn, Wf);
                o[i >> 2] |= level<MODE>(kSoft ? v / scale : v, 0, a255) << (8 * (i & 3));
            }
            *reinterpret_cast<uint4 *>(dst + s.qa) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (int64_t q = s.qa; q < s.qb; ++q) {
            const double v = logit_up(a0, a1, tap_of(wx, Wn, Wf), ty);
            walk_on(wx, Wn, Wf);
            const double x = kSoft ? v / scale : v;
            if (kBlend) {
                const int64_t sp = MIRROR ? L - 1 - q : q;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t b = src[3 * sp + c];
                    dst[3 * q + c] = (uint8_t)(channel == c ? level<MODE>(x, b, a255) : b);
                }
            } else {
                dst[q] = (uint8_t)level<MODE>(x, 0, a255);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ overlay_objects
// Several objects (util/object_overlay.py): the label of a pixel is the merge rule (common.hpp: merge_take) over the K maps,
// its colour entry `label` of the palette, blended into all three channels.
// The palette's entries 1..K as B | G << 8 | R << 16 (entry 0 is never painted), read once per workgroup.  Every thread of
// the workgroup passes here before any of them leaves.
__device__ __forceinline__ void stage_colours(const uint8_t *__restrict__ palette, int K, uint32_t (&cols)[kMaxObjects + 1]) {
    const int k = threadIdx.x;
    if (k <= K)
        cols[k] = k == 0 ? 0u : (uint32_t)palette[3 * k + 2] | ((uint32_t)palette[3 * k + 1] << 8) | ((uint32_t)palette[3 * k] << 16);
    __syncthreads();
}
// the three output bytes (in bits 0..23) of a pixel with the frame's bytes b[3] and the colour `col`, label 0 keeps b
__device__ __forceinline__ uint32_t paint(const uint32_t (&b)[3], uint32_t label, uint32_t col, double alpha) {
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double fb = (double)b[c];
        const double v = fb + alpha * ((double)((col >> (8 * c)) & 0xffu) - fb);
        o |= (label ? (uint32_t)(v + 0.5) : b[c]) << (8 * c);
    }
    return o;
}

// k_overlay's partition; the groups are anchored on map 0, so maps 1..K-1 lie wherever their base pointers put them: all of
// them are loaded as floats4 (alignment 4), which is what they are known to have.
template <bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_objects(const uint8_t *__restrict__ frames, const ObjectLogits maps,
                                                                    int K, const uint8_t *__restrict__ palette,
                                                                    uint8_t *__restrict__ out, int64_t L, int64_t slots,
                                                                    int64_t total, double alpha) {
    __shared__ uint32_t cols[kMaxObjects + 1];
    stage_colours(palette, K, cols);
    const int64_t gid = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (gid >= total) return;
    const int64_t seg = segment_of(gid, slots);
    const Span s = span_of(gid, seg, slots, L, maps.p[0] + seg * L);
    const uint8_t *__restrict__ src = frames + seg * 3 * L;
    uint8_t *__restrict__ dst = out + seg * 3 * L;
    if (s.qb - s.qa == kGroup) {
        float bv[kGroup];
        uint32_t lab[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) bv[i] = -1.f, lab[i] = 0u;
        for (int k = 0; k < K; ++k) {
            const floats4 *__restrict__ lv = reinterpret_cast<const floats4 *>(maps.p[k] + seg * L + s.qa);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const floats4 t = lv[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) merge_take(t.v[i], (uint32_t)k, bv[4 * j + i], lab[4 * j + i]);
            }
        }
        uint32_t w[12], o[12];
        load48(src + 3 * (MIRROR ? L - kGroup - s.qa : s.qa), w);
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = 0;
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const int px = MIRROR ? kGroup - 1 - i : i;
            const uint32_t b[3] = {byte_at(w, 3 * px), byte_at(w, 3 * px + 1), byte_at(w, 3 * px + 2)};
            const uint32_t v = paint(b, lab[i], cols[lab[i]], alpha);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int at = 3 * i + c;
                o[at >> 2] |= ((v >> (8 * c)) & 0xffu) << (8 * (at & 3));
            }
        }
        bytes16 *__restrict__ ov = reinterpret_cast<bytes16 *>(dst + 3 * s.qa);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bytes16 t;
#pragma unroll
            for (int i = 0; i < 4; ++i) t.w[i] = o[4 * k + i];
            ov[k] = t;
        }
    } else {
        for (int64_t q = s.qa; q < s.qb; ++q) {
            float bv = -1.f;
            uint32_t lab = 0u;
            for (int k = 0; k < K; ++k) merge_take(maps.p[k][seg * L + q], (uint32_t)k, bv, lab);
            const int64_t sp = MIRROR ? L - 1 - q : q;
            const uint32_t b[3] = {src[3 * sp], src[3 * sp + 1], src[3 * sp + 2]};
            const uint32_t v = paint(b, lab, cols[lab], alpha);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[3 * q + c] = (uint8_t)(v >> (8 * c));
        }
    }
}

// the label of the output pixel whose taps are tx, ty: the taps are taken once and applied to all K maps (rows at `top` and
// `bot` floats into every map)
__device__ __forceinline__ uint32_t label_up(const ObjectLogits &maps, int K, int64_t top, int64_t bot, const Tap &tx,
                                             const Tap &ty) {
    double bv = -1.0;
    uint32_t lab = 0u;
    for (int k = 0; k < K; ++k) merge_take(logit_up(maps.p[k] + top, maps.p[k] + bot, tx, ty), (uint32_t)k, bv, lab);
    return lab;
}

// k_overlay_scaled's thread map.  MODE 0: the overlay; MODE 1: the label map, one byte a pixel
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_objects_scaled(const uint8_t *__restrict__ frames,
                                                                           const ObjectLogits maps, int K,
                                                                           const uint8_t *__restrict__ palette,
                                                                           uint8_t *__restrict__ out, int Hf, int Wf, int Hn,
                                                                           int Wn, int64_t slots, int64_t total, double alpha) {
    constexpr bool kBlend = MODE == 0;
    __shared__ uint32_t cols[kMaxObjects + 1];
    if (kBlend) stage_colours(palette, K, cols);
    const int64_t gid = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (gid >= total) return;
    const int64_t seg = segment_of(gid, slots), L = Wf;
    const int64_t n = seg / Hf;
    const int y = (int)(seg - n * Hf);
    const uint8_t *__restrict__ src = kBlend ? frames + seg * 3 * L : nullptr;
    uint8_t *__restrict__ dst = out + seg * (kBlend ? 3 : 1) * L;
    const unsigned lead = (16u - ((unsigned)(uintptr_t)dst & 15u)) & 15u;
    const Span s = span_at(gid, seg, slots, L, (int)(kBlend ? (11u * lead) & 15u : lead));
    const Tap ty = tap_of(walk_from(y, Hn, Hf), Hn, Hf);
    const int64_t top = (n * Hn + ty.i0) * Wn, bot = (n * Hn + ty.i1) * Wn;
    Walk wx = walk_from((int)s.qa, Wn, Wf);
    if (s.qb - s.qa == kGroup) {
        if (kBlend) {
            uint32_t w[12], o[12];
            load48(src + 3 * (MIRROR ? L - kGroup - s.qa : s.qa), w);
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = 0;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const uint32_t lab = label_up(maps, K, top, bot, tap_of(wx, Wn, Wf), ty);
                walk_on(wx, Wn, Wf);
                const int px = MIRROR ? kGroup - 1 - i : i;
                const uint32_t b[3] = {byte_at(w, 3 * px), byte_at(w, 3 * px + 1), byte_at(w, 3 * px + 2)};
                const uint32_t v = paint(b, lab, cols[lab], alpha);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int at = 3 * i + c;
                    o[at >> 2] |= ((v >> (8 * c)) & 0xffu) << (8 * (at & 3));
                }
            }
            uint4 *__restrict__ ov = reinterpret_cast<uint4 *>(dst + 3 * s.qa);
#pragma unroll
            for (int k = 0; k < 3; ++k) ov[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
        } else {
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                o[i >> 2] |= label_up(maps, K, top, bot, tap_of(wx, Wn, Wf), ty) << (8 * (i & 3));
                walk_on(wx, Wn, Wf);
            }
            *reinterpret_cast<uint4 *>(dst + s.qa) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (int64_t q = s.qa; q < s.qb; ++q) {
            const uint32_t lab = label_up(maps, K, top, bot, tap_of(wx, Wn, Wf), ty);
            walk_on(wx, Wn, Wf);
            if (kBlend) {
                const int64_t sp = MIRROR ? L - 1 - q : q;
                const uint32_t b[3] = {src[3 * sp], src[3 * sp + 1], src[3 * sp + 2]};
                const uint32_t v = paint(b, lab, cols[lab], alpha);
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[3 * q + c] = (uint8_t)(v >> (8 * c));
            } else {
                dst[q] = (uint8_t)lab;
            }
        }
    }
}

// segments and threads of a launch
struct Partition {
    int64_t L, slots, total;
    int R;
};
inline Partition partition_of(int N, int H, int W, int mirror) {
    Partition p;
    p.R = mirror ? H : 1;
    p.L = mirror ? (int64_t)W : (int64_t)H * W;
    p.slots = p.L / kGroup + 2;
    p.total = (int64_t)N * p.R * p.slots;
    return p;
}
constexpr int64_t kMaxPixels = (int64_t)1 << 36;  // N H W: keeps every count far inside int64 and the grid inside 2^31

template <int MODE>
void launch_overlay(bool mirror, dim3 grid, hipStream_t st, const uint8_t *frames, const float *logits, uint8_t *out,
                    const Partition &p, int channel, double a255) {
    if (mirror)
        hipLaunchKernelGGL((k_overlay<MODE, true>), grid, dim3(kStreamThreads), 0, st, frames, logits, out, p.L, p.slots, p.total,
                           channel, a255);
    else
        hipLaunchKernelGGL((k_overlay<MODE, false>), grid, dim3(kStreamThreads), 0, st, frames, logits, out, p.L, p.slots, p.total,
                           channel, a255);
}
template <int MODE>
void launch_overlay_scaled(bool mirror, dim3 grid, hipStream_t st, const uint8_t *frames, const float *logits, uint8_t *out,
                           int Hf, int Wf, int Hn, int Wn, const Partition &p, int channel, double a255) {
    if (mirror)
        hipLaunchKernelGGL((k_overlay_scaled<MODE, true>), grid, dim3(kStreamThreads), 0, st, frames, logits, out, Hf, Wf, Hn,
                           Wn, p.slots, p.total, channel, a255);
    else
        hipLaunchKernelGGL((k_overlay_scaled<MODE, false>), grid, dim3(kStreamThreads), 0, st, frames, logits, out, Hf, Wf, Hn,
                           Wn, p.slots, p.total, channel, a255);
}
// the sizes of a scaled call: the frame's and the net's
int check_sizes(const char *who, int N, int Hf, int Wf, int Hn, int Wn) {
    FOSVOS_REQUIRE(N > 0 && Hf > 0 && Wf > 0 && Hn > 0 && Wn > 0 && Hf <= kMaxSide && Wf <= kMaxSide &&
                       (int64_t)N * Hf * Wf <= kMaxPixels,
                   FOSVOS_E_SHAPE, "%s: N=%d, frames of %dx%d, a net of %dx%d (sides of 1..%d)", who, N, Hf, Wf, Hn, Wn, kMaxSide);
    FOSVOS_REQUIRE(Hn <= Hf && Wn <= Wf, FOSVOS_E_SHAPE, "%s: the net's size %dx%d exceeds the frame's %dx%d", who, Hn, Wn, Hf,
                   Wf);
    return FOSVOS_OK;
}
}  // namespace

extern "C" int fosvos_frame_prep(const uint8_t *frames, int N, int H, int W, int mirror, const float mean[3], float *image,
                                 int device, void *stream) {
    FOSVOS_REQUIRE(frames && mean && image, FOSVOS_E_ARG, "frame_prep: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)N * H * W <= kMaxPixels, FOSVOS_E_SHAPE, "frame_prep: N=%d H=%d W=%d", N,
                   H, W);
    FOSVOS_REQUIRE(((uintptr_t)image & 3) == 0, FOSVOS_E_ARG, "frame_prep: the image must be 4-byte aligned");
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, H, W, mirror);
    const dim3 grid((unsigned)cdiv(p.total, kStreamThreads));
    const int64_t plane = (int64_t)H * W;
    const MeanBGR m = {{mean[0], mean[1], mean[2]}};
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_frame_prep", stream, 0.0);
    if (mirror)
        hipLaunchKernelGGL(k_frame_prep<true>, grid, dim3(kStreamThreads), 0, st, frames, image, p.L, p.R, plane, p.slots, p.total,
                           m);
    else
        hipLaunchKernelGGL(k_frame_prep<false>, grid, dim3(kStreamThreads), 0, st, frames, image, p.L, p.R, plane, p.slots,
                           p.total, m);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay(const uint8_t *frames, const float *logits, int N, int H, int W, int mirror, int mode, int channel,
                              double alpha, uint8_t *out, int device, void *stream) {
    FOSVOS_REQUIRE(mode >= 0 && mode <= 3, FOSVOS_E_ARG, "overlay: mode %d outside [0, 3]", mode);
    FOSVOS_REQUIRE(logits && out && (frames || mode >= 2), FOSVOS_E_ARG, "overlay: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)N * H * W <= kMaxPixels, FOSVOS_E_SHAPE, "overlay: N=%d H=%d W=%d", N, H, W);
    FOSVOS_REQUIRE(channel >= 0 && channel <= 2, FOSVOS_E_ARG, "overlay: channel %d outside [0, 2]", channel);
    FOSVOS_REQUIRE(alpha >= 0.0 && isfinite(alpha), FOSVOS_E_ARG, "overlay: alpha %g is not a finite number >= 0", alpha);
    FOSVOS_REQUIRE(((uintptr_t)logits & 3) == 0, FOSVOS_E_ARG, "overlay: the logits must be 4-byte aligned");
    FOSVOS_ENTER(device);
    // a mask (modes 2, 3) has nothing to mirror: the logits already are in output order
    const Partition p = partition_of(N, H, W, mode < 2 ? mirror : 0);
    const dim3 grid((unsigned)cdiv(p.total, kStreamThreads));
    const double a255 = alpha * 255.0;
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_overlay", stream, 0.0);
    switch (mode) {
        case 0: launch_overlay<0>(mirror != 0, grid, st, frames, logits, out, p, channel, a255); break;
        case 1: launch_overlay<1>(mirror != 0, grid, st, frames, logits, out, p, channel, a255); break;
        case 2: launch_overlay<2>(false, grid, st, frames, logits, out, p, channel, a255); break;
        default: launch_overlay<3>(false, grid, st, frames, logits, out, p, channel, a255); break;
    }
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_frame_prep_scaled(const uint8_t *frames, int N, int Hf, int Wf, int Hn, int Wn, int mirror,
                                        const float mean[3], float *image, int device, void *stream) {
    FOSVOS_REQUIRE(frames && mean && image, FOSVOS_E_ARG, "frame_prep_scaled: null pointer");
    if (int rc = check_sizes("frame_prep_scaled", N, Hf, Wf, Hn, Wn)) return rc;
    FOSVOS_REQUIRE(((uintptr_t)image & 3) == 0, FOSVOS_E_ARG, "frame_prep_scaled: the image must be 4-byte aligned");
    FOSVOS_ENTER(device);
    ScaleGeom g = {Hf, Wf, Hn, Wn, 0, 0, 0, 0};
    // the source pixels under a workgroup's columns (64, and up to 3 more in front), cut to the chunk; the rows under its rows
    const int64_t under = cdiv((int64_t)(4 * kScaleCells + 3) * Wf, Wn) + 1;
    g.pitch = roundup(3 * (int)std::min<int64_t>(under, kScaleChunkPx), 16);
    g.rows = (int)std::min<int64_t>(cdiv((int64_t)kScaleRows * Hf, Hn) + 1, kScaleStageBytes / g.pitch);
    g.tiles = (int)cdiv(cdiv(Wn + 3, 4), kScaleCells);
    g.strips = (int)cdiv(Hn, kScaleRows);
    const int64_t blocks = (int64_t)N * g.tiles * g.strips;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "frame_prep_scaled: %lld workgroups", (long long)blocks);
    const MeanBGR m = {{mean[0], mean[1], mean[2]}};
    const int64_t frame_bytes = (int64_t)N * Hf * Wf * 3;
    const size_t lds = (size_t)g.pitch * g.rows;
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_frame_prep_scaled", stream, 0.0);
    if (mirror)
        hipLaunchKernelGGL(k_frame_prep_scaled<true>, dim3((unsigned)blocks), dim3(kScaleThreads), lds, st, frames, image, g,
                           frame_bytes, m);
    else
        hipLaunchKernelGGL(k_frame_prep_scaled<false>, dim3((unsigned)blocks), dim3(kScaleThreads), lds, st, frames, image, g,
                           frame_bytes, m);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay_scaled(const uint8_t *frames, const float *logits, int N, int Hf, int Wf, int Hn, int Wn,
                                     int mirror, int mode, int channel, double alpha, uint8_t *out, int device, void *stream) {
    FOSVOS_REQUIRE(mode >= 0 && mode <= 3, FOSVOS_E_ARG, "overlay_scaled: mode %d outside [0, 3]", mode);
    FOSVOS_REQUIRE(logits && out && (frames || mode >= 2), FOSVOS_E_ARG, "overlay_scaled: null pointer");
    if (int rc = check_sizes("overlay_scaled", N, Hf, Wf, Hn, Wn)) return rc;
    FOSVOS_REQUIRE(channel >= 0 && channel <= 2, FOSVOS_E_ARG, "overlay_scaled: channel %d outside [0, 2]", channel);
    FOSVOS_REQUIRE(alpha >= 0.0 && isfinite(alpha), FOSVOS_E_ARG, "overlay_scaled: alpha %g is not a finite number >= 0", alpha);
    FOSVOS_REQUIRE(((uintptr_t)logits & 3) == 0, FOSVOS_E_ARG, "overlay_scaled: the logits must be 4-byte aligned");
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, Hf, Wf, 1);  // rows, in every mode
    const dim3 grid((unsigned)cdiv(p.total, kStreamThreads));
    const double a255 = alpha * 255.0;
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_overlay_scaled", stream, 0.0);
    switch (mode) {
        case 0: launch_overlay_scaled<0>(mirror != 0, grid, st, frames, logits, out, Hf, Wf, Hn, Wn, p, channel, a255); break;
        case 1: launch_overlay_scaled<1>(mirror != 0, grid, st, frames, logits, out, Hf, Wf, Hn, Wn, p, channel, a255); break;
        case 2: launch_overlay_scaled<2>(false, grid, st, frames, logits, out, Hf, Wf, Hn, Wn, p, channel, a255); break;
        default: launch_overlay_scaled<3>(false, grid, st, frames, logits, out, Hf, Wf, Hn, Wn, p, channel, a255); break;
    }
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

namespace {
// the K pointers of a several-objects call, by value
int object_maps(const char *who, const float *const *logits, int K, ObjectLogits &maps) {
    FOSVOS_REQUIRE(K >= 1 && K <= kMaxObjects, FOSVOS_E_ARG, "%s: K=%d outside [1, %d]", who, K, kMaxObjects);
    FOSVOS_REQUIRE(logits, FOSVOS_E_ARG, "%s: null pointer", who);
    for (int k = 0; k < K; ++k) {
        FOSVOS_REQUIRE(logits[k] != nullptr, FOSVOS_E_ARG, "%s: null logit map %d", who, k);
        FOSVOS_REQUIRE(((uintptr_t)logits[k] & 3) == 0, FOSVOS_E_ARG, "%s: logit map %d must be 4-byte aligned", who, k);
        maps.p[k] = logits[k];
    }
    return FOSVOS_OK;
}
}  // namespace

extern "C" int fosvos_overlay_objects(const uint8_t *frames, const float *const *logits, int K, int N, int H, int W, int mirror,
                                      const uint8_t *palette, double alpha, uint8_t *out, int device, void *stream) {
    ObjectLogits maps = {};
    if (int rc = object_maps("overlay_objects", logits, K, maps)) return rc;
    FOSVOS_REQUIRE(frames && palette && out, FOSVOS_E_ARG, "overlay_objects: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)N * H * W <= kMaxPixels, FOSVOS_E_SHAPE, "overlay_objects: N=%d H=%d W=%d",
                   N, H, W);
    FOSVOS_REQUIRE(alpha >= 0.0 && alpha <= 1.0, FOSVOS_E_ARG, "overlay_objects: alpha %g is not a number in [0, 1]", alpha);
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, H, W, mirror);
    const dim3 grid((unsigned)cdiv(p.total, kStreamThreads));
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_overlay_objects", stream, 0.0);
    if (mirror)
        hipLaunchKernelGGL(k_overlay_objects<true>, grid, dim3(kStreamThreads), 0, st, frames, maps, K, palette, out, p.L, p.slots,
                           p.total, alpha);
    else
        hipLaunchKernelGGL(k_overlay_objects<false>, grid, dim3(kStreamThreads), 0, st, frames, maps, K, palette, out, p.L, p.slots,
                           p.total, alpha);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay_objects_scaled(const uint8_t *frames, const float *const *logits, int K, int N, int Hf, int Wf,
                                             int Hn, int Wn, int mirror, int mode, const uint8_t *palette, double alpha,
                                             uint8_t *out, int device, void *stream) {
    FOSVOS_REQUIRE(mode == 0 || mode == 1, FOSVOS_E_ARG, "overlay_objects_scaled: mode %d outside [0, 1]", mode);
    ObjectLogits maps = {};
    if (int rc = object_maps("overlay_objects_scaled", logits, K, maps)) return rc;
    FOSVOS_REQUIRE(out && ((frames && palette) || mode == 1), FOSVOS_E_ARG, "overlay_objects_scaled: null pointer");
    if (int rc = check_sizes("overlay_objects_scaled", N, Hf, Wf, Hn, Wn)) return rc;
    FOSVOS_REQUIRE(mode == 1 || (alpha >= 0.0 && alpha <= 1.0), FOSVOS_E_ARG,
                   "overlay_objects_scaled: alpha %g is not a number in [0, 1]", alpha);
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, Hf, Wf, 1);  // rows, in both modes
    const dim3 grid((unsigned)cdiv(p.total, kStreamThreads)), block(kStreamThreads);
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_overlay_objects_scaled", stream, 0.0);
    if (mode == 1)  // a label map has nothing to mirror: the logits already are in output order
        hipLaunchKernelGGL((k_overlay_objects_scaled<1, false>), grid, block, 0, st, frames, maps, K, palette, out, Hf, Wf, Hn, Wn,
                           p.slots, p.total, alpha);
    else if (mirror)
        hipLaunchKernelGGL((k_overlay_objects_scaled<0, true>), grid, block, 0, st, frames, maps, K, palette, out, Hf, Wf, Hn, Wn,
                           p.slots, p.total, alpha);
    else
        hipLaunchKernelGGL((k_overlay_objects_scaled<0, false>), grid, block, 0, st, frames, maps, K, palette, out, Hf, Wf, Hn, Wn,
                           p.slots, p.total, alpha);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
