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
// Following the object (opt-in; util/frame_roi.py states all three): the net sees a WINDOW (y0, x0, Hw, Ww) of each frame, and the
// windows come from device memory, int32 [N][4], so the host never reads one.  Every kernel sanitises what it loads
// (sane_window): a window that is not valid is the whole frame, so no bound or address depends on an unchecked value.
// fosvos_frame_prep_window, one launch:
//   k_frame_prep_window  k_frame_prep_scaled's body (prep_scaled) on the window of the workgroup's frame: same grid, same stage.
// fosvos_overlay_window, one launch:
//   k_overlay_window     the paint skeleton with the source MapUpWindow: MapUp's value inside the window, -inf outside it.
// fosvos_window_next, two launches:
//   k_window_reset       the frames' boxes and counts in the workspace to their start values.
//   k_window_next        the bounding box of logits >= 0 by __ballot and one atomic min / max per workgroup and bound; the
//                        workgroup that finishes last turns the box into the next window.
//
// Edge-aware upsampling (opt-in; util/guided_upsample.py states it): the coefficient maps of the guided filter (csrc/guided.hip)
// in place of the logits.
// fosvos_overlay_guided, one launch:
//   k_overlay_guided     the paint skeleton with the source PairUp - 4 Hf Wf times abar and bbar, fp64 [N,2,Hn,Wn], interpolated
//                        with k_overlay_scaled's taps - and the paint Guided: v = A I + Bv, I the fp64 sum of the (mirrored)
//                        pixel's own mean-free bytes, then OneChannel / OneByte on v.  It reads the frame in every mode.
//
// Several objects a stream (opt-in; util/object_overlay.py states both): the K logit maps of K per-object nets, pointers by value.
// fosvos_overlay_objects, one launch:
//   k_overlay_objects         a thread takes its 16 logits from each of the K maps in turn and keeps (best value, label) per
//                             pixel - the rule of fosvos_merge_objects - then blends every labelled pixel towards its palette
//                             colour: b + alpha (col - b) in fp64, rounded half up.  4 K + 3 B read, 3 B written per pixel; no
//                             label map in between.
// fosvos_overlay_objects_scaled, one launch:
//   k_overlay_objects_scaled  the same from [Hn,Wn] maps; the taps of a pixel are taken once and applied to all K maps, the
//                             rule then runs on the fp64 values.  Mode 0 the overlay, mode 1 the label map.
//
// The four overlay kernels are one body, paint_pixels<MIRROR, Source, Paint>, behind thin __global__ wrappers.  The body owns
// the partition above, the 48-byte load and its mirror unpack, the packing and the 16-byte stores, and the scalar loop of a
// head or tail.  A SOURCE says where a pixel's value comes from, and with that where the groups are anchored and which store
// goes with the anchor: MapInPlace (one fp32 map, a float) and MapsInPlace (K maps merged in fp32, a label) anchor on their
// first map and store bytes16; MapUp (one map interpolated, a double) and MapsUp (K maps through shared taps, merged in fp64,
// a label) anchor on the output row and store aligned uint4.  A PAINT turns the value and the frame's bytes into the output's:
// OneChannel (level<MODE> in one channel), PaletteBlend (towards the label's colour, all three) or OneByte (a mask or a label,
// no frame read).  k_overlay = MapInPlace + OneChannel | OneByte, k_overlay_scaled = MapUp + the same, k_overlay_objects =
// MapsInPlace + PaletteBlend, k_overlay_objects_scaled = MapsUp + PaletteBlend | OneByte.  k_overlay_window is a fifth wrapper,
// MapUpWindow + OneChannel | OneByte: a source beside MapUp, the paints as they are.  k_overlay_guided is a sixth, PairUp +
// Guided<OneChannel | OneByte>: a source whose value is a pair and a paint that reduces it in front of the paint of the mode.
// Whether the body loads the frame is the paint's compile-time property kReadsFrame, not its byte count: the guided mask
// modes write one byte and read the frame.
#include <limits.h>
#include <math.h>

#include <type_traits>

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
//
// The SOURCE of the walk is a rectangle of the frame: `src` = (y0, x0, Hs, Ws) in the unmirrored frame, the whole frame
// (0, 0, Hf, Wf) for k_frame_prep_scaled, a sanitised window for k_frame_prep_window.  The weights, the windows of the output
// pixels and the area are the rectangle's; only the staging adds its origin, and the frame's own Wf is the row pitch.  The
// stage was sized for the whole frame, and both walks cut their steps to it, so any rectangle inside the frame fits.
struct Rect {
    int y0, x0, H, W;
};
template <bool MIRROR>
__device__ __forceinline__ void prep_scaled(const uint8_t *__restrict__ frames, float *__restrict__ image, const ScaleGeom &g,
                                            const Rect src, int64_t frame_bytes, const MeanBGR &mean, uint8_t *stage) {
    const int Hf = src.H, Wf = src.W, Hn = g.Hn, Wn = g.Wn;  // from here on the source's sides; the frame's are g.Hf, g.Wf
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
                const int64_t at = (((n * g.Hf + src.y0 + yb + r) * g.Wf) + src.x0 + xa) * 3 + 16 * k;
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
template <bool MIRROR>
__global__ __launch_bounds__(kScaleThreads) void k_frame_prep_scaled(const uint8_t *__restrict__ frames,
                                                                     float *__restrict__ image, ScaleGeom g,
                                                                     int64_t frame_bytes, MeanBGR mean) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    prep_scaled<MIRROR>(frames, image, g, Rect{0, 0, g.Hf, g.Wf}, frame_bytes, mean, stage);
}

// ------------------------------------------------------------------------------------------ windows (util/frame_roi.py)
// A window (y0, x0, Hw, Ww) comes from device memory, so nothing about it is known: it is valid when Hn <= Hw <= Hf, Wn <=
// Ww <= Wf, 0 <= y0 <= Hf - Hw and 0 <= x0 <= Wf - Ww, and any other - negative, overflowing - is the whole frame.  The sides
// are compared first, so the two differences are taken of numbers in [0, 8192].  Whatever passes lies inside the frame: every
// loop bound and address behind this function is one the whole-frame launch could have had.
__device__ __forceinline__ Rect sane_window(int y0, int x0, int Hw, int Ww, int Hf, int Wf, int Hn, int Wn) {
    const bool sides = Hw >= Hn && Hw <= Hf && Ww >= Wn && Ww <= Wf;
    const bool ok = sides && y0 >= 0 && x0 >= 0 && y0 <= Hf - (sides ? Hw : Hf) && x0 <= Wf - (sides ? Ww : Wf);
    return ok ? Rect{y0, x0, Hw, Ww} : Rect{0, 0, Hf, Wf};
}
// frame n's window, the same for every lane of the wave that asks: four ordinary loads, then one copy in scalar registers
__device__ __forceinline__ Rect uniform_window(const int32_t *__restrict__ windows, int64_t n, int Hf, int Wf, int Hn, int Wn) {
    const int32_t *__restrict__ w = windows + 4 * n;
    const int y0 = __builtin_amdgcn_readfirstlane(w[0]), x0 = __builtin_amdgcn_readfirstlane(w[1]);
    const int Hw = __builtin_amdgcn_readfirstlane(w[2]), Ww = __builtin_amdgcn_readfirstlane(w[3]);
    return sane_window(y0, x0, Hw, Ww, Hf, Wf, Hn, Wn);
}

// k_frame_prep_scaled on the window of the workgroup's frame.  The window is given in the picture the net sees: with MIRROR
// its columns [x0, x0 + Ww) are the unmirrored frame's [Wf - x0 - Ww, Wf - x0), walked backwards as the whole frame is.
template <bool MIRROR>
__global__ __launch_bounds__(kScaleThreads) void k_frame_prep_window(const uint8_t *__restrict__ frames,
                                                                     const int32_t *__restrict__ windows,
                                                                     float *__restrict__ image, ScaleGeom g,
                                                                     int64_t frame_bytes, MeanBGR mean) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    const int64_t n = blockIdx.x / ((unsigned)g.tiles * g.strips);
    Rect w = uniform_window(windows, n, g.Hf, g.Wf, g.Hn, g.Wn);
    if (MIRROR) w.x0 = g.Wf - w.x0 - w.W;
    prep_scaled<MIRROR>(frames, image, g, w, frame_bytes, mean, stage);
}

// ------------------------------------------------------------------------------------------ the overlays: paints
// A paint turns the value of a pixel and the frame's bytes b[3] into the output bytes o[0..kBytes): 3 repaint the frame, 1
// writes a map of its own.  kReadsFrame says whether the skeleton loads b for it: every paint that repaints the frame, and the
// guided paint in its mask modes too, whose value is made of the pixel's own bytes.
//
// the new byte of one pixel: `byte` is the frame's value in the overlay's channel (unused in the mask modes); x is the fp32
// logit, or (scaled) the fp64 one - in the boolean modes any positive multiple of it
template <int MODE, typename T>
__device__ __forceinline__ uint32_t level(T x, uint32_t byte, double a255) {
    if (MODE == 2) return x >= T(0) ? 255u : 0u;
    if (MODE == 3) return (uint32_t)(255.0 * sigmoid_f64(x) + 0.5);
    const double p = MODE == 0 ? (x >= T(0) ? 1.0 : 0.0) : sigmoid_f64(x);
    return (uint32_t)fmin((double)byte + a255 * p, 255.0);
}
// MODE 0, 1: the level in one channel, the other two as they are
template <int MODE>
struct OneChannel {
    static constexpr int kBytes = 3;
    static constexpr bool kReadsFrame = true;
    int channel;
    double a255;
    template <typename T>
    __device__ __forceinline__ void operator()(T x, const uint32_t (&b)[3], uint32_t (&o)[3]) const {
        const uint32_t b0 = b[0], b1 = b[1], b2 = b[2];  // read before the choice: selects, where a reference would branch
        const uint32_t v = level<MODE>(x, channel == 0 ? b0 : (channel == 1 ? b1 : b2), a255);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = channel == c ? v : b[c];
    }
};
// one byte a pixel: the mask of a logit (MODE 2, 3), or the label of a several-objects source as it is
template <int MODE>
struct OneByte {
    static constexpr int kBytes = 1;
    static constexpr bool kReadsFrame = false;
    template <typename T>
    __device__ __forceinline__ void operator()(T x, const uint32_t (&)[3], uint32_t (&o)[3]) const {
        o[0] = level<MODE>(x, 0u, 0.0);
    }
    __device__ __forceinline__ void operator()(uint32_t label, const uint32_t (&)[3], uint32_t (&o)[3]) const { o[0] = label; }
};
using LabelByte = OneByte<2>;  // no level is taken of a label, so the mode stands for nothing
// Several objects (util/object_overlay.py): a labelled pixel is blended towards entry `label` of the palette in all three
// channels, b + alpha (col - b) in fp64, rounded half up; label 0 keeps b.
// The palette's entries 1..K as B | G << 8 | R << 16 (entry 0 is never painted), read once per workgroup.  Every thread of
// the workgroup passes here before any of them leaves.
__device__ __forceinline__ void stage_colours(const uint8_t *__restrict__ palette, int K, uint32_t (&cols)[kMaxObjects + 1]) {
    const int k = threadIdx.x;
    if (k <= K)
        cols[k] = k == 0 ? 0u : (uint32_t)palette[3 * k + 2] | ((uint32_t)palette[3 * k + 1] << 8) | ((uint32_t)palette[3 * k] << 16);
    __syncthreads();
}
struct PaletteBlend {
    static constexpr int kBytes = 3;
    static constexpr bool kReadsFrame = true;
    const uint32_t *cols;  // what stage_colours staged
    double alpha;
    __device__ __forceinline__ void operator()(uint32_t label, const uint32_t (&b)[3], uint32_t (&o)[3]) const {
        const uint32_t col = cols[label];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double fb = (double)b[c];
            const double v = fb + alpha * ((double)((col >> (8 * c)) & 0xffu) - fb);
            o[c] = label ? (uint32_t)(v + 0.5) : b[c];
        }
    }
};

// ------------------------------------------------------------------------------------------ the overlays: sources
// A source says where a pixel's value comes from.  open() places the thread: it takes the segment, decides where the
// segment's groups start (the anchor) and returns the thread's span; Store is the 16-byte store that goes with that anchor.
// load_group() and take(i), i = 0..15 in turn, serve a full group, at(q), q rising, the pixels of a head or tail.
//
// Maps read in place, at the frames' size: the groups start where the (first) map crosses a 16-byte boundary, so its loads
// are aligned and the output bytes lie wherever they fall (bytes16: alignment 1).  A group's logits are loaded up front.
struct MapInPlace {
    using Store = bytes16;
    const float *__restrict__ logits;
    int64_t L;
    const float *__restrict__ lg;  // the thread's segment
    float x[kGroup];
    __device__ __forceinline__ int64_t length() const { return L; }
    __device__ __forceinline__ Span open(int64_t gid, int64_t seg, int64_t slots, const uint8_t *, int) {
        lg = logits + seg * L;
        return span_of(gid, seg, slots, L, lg);
    }
    __device__ __forceinline__ void load_group(int64_t qa) {
        const floats4 *__restrict__ lv = reinterpret_cast<const floats4 *>(lg + qa);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const floats4 t = lv[k];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[4 * k + i] = t.v[i];
        }
    }
    __device__ __forceinline__ float take(int i) const { return x[i]; }
    __device__ __forceinline__ float at(int64_t q) const { return lg[q]; }
};
// K maps in place, merged by the rule of fosvos_merge_objects (common.hpp: merge_take) in fp32 into a label.  The anchor is
// map 0, so maps 1..K-1 lie wherever their base pointers put them: all of them are loaded as floats4 (alignment 4), which
// is what they are known to have.
struct MapsInPlace {
    using Store = bytes16;
    const ObjectLogits &maps;
    int K;
    int64_t L;
    int64_t first;  // of the thread's segment, in floats into every map
    uint32_t lab[kGroup];
    __device__ __forceinline__ int64_t length() const { return L; }
    __device__ __forceinline__ Span open(int64_t gid, int64_t seg, int64_t slots, const uint8_t *, int) {
        first = seg * L;
        return span_of(gid, seg, slots, L, maps.p[0] + first);
    }
    __device__ __forceinline__ void load_group(int64_t qa) {
        float bv[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) bv[i] = -1.f, lab[i] = 0u;
        for (int k = 0; k < K; ++k) {
            const floats4 *__restrict__ lv = reinterpret_cast<const floats4 *>(maps.p[k] + first + qa);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const floats4 t = lv[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) merge_take(t.v[i], (uint32_t)k, bv[4 * j + i], lab[4 * j + i]);
            }
        }
    }
    __device__ __forceinline__ uint32_t take(int i) const { return lab[i]; }
    __device__ __forceinline__ uint32_t at(int64_t q) const {
        float bv = -1.f;
        uint32_t label = 0u;
        for (int k = 0; k < K; ++k) merge_take(maps.p[k][first + q], (uint32_t)k, bv, label);
        return label;
    }
};

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

// What the interpolated sources share: maps of [Hn,Wn] gathered for frames of [Hf,Wf], bilinear at half-pixel centres with
// integer weights, in fp64.  The segments are the rows; their groups start where the OUTPUT row crosses a 16-byte boundary
// (the logits are gathered, four floats a pixel out of a map that stays in L2, so they have no aligned side to offer), which
// makes every group store an aligned uint4.  The row's taps are taken once, the column taps walk along with the pixels.
__device__ __forceinline__ Span span_of_row(int64_t gid, int64_t seg, int64_t slots, int Wf, const uint8_t *dst, int bytes) {
    // pixels up to the boundary: k0 (or 3 k0, 3 * 11 = 1 mod 16) + the address = 0 mod 16
    const unsigned lead = (16u - ((unsigned)(uintptr_t)dst & 15u)) & 15u;
    return span_at(gid, seg, slots, Wf, (int)(bytes == 3 ? (11u * lead) & 15u : lead));
}
struct RowsUp {
    using Store = uint4;
    int Hf, Wf, Hn, Wn;
    Tap ty;
    Walk wx;
    int64_t top, bot;  // the rows of ty, in floats into a map
    __device__ __forceinline__ int64_t length() const { return Wf; }
    __device__ __forceinline__ Span open(int64_t gid, int64_t seg, int64_t slots, const uint8_t *dst, int bytes) {
        const int64_t n = seg / Hf;
        ty = tap_of(walk_from((int)(seg - n * Hf), Hn, Hf), Hn, Hf);
        top = (n * Hn + ty.i0) * Wn, bot = (n * Hn + ty.i1) * Wn;
        const Span s = span_of_row(gid, seg, slots, Wf, dst, bytes);
        wx = walk_from((int)s.qa, Wn, Wf);
        return s;
    }
    __device__ __forceinline__ void load_group(int64_t) {}
    __device__ __forceinline__ Tap next_tap() {
        const Tap tx = tap_of(wx, Wn, Wf);
        walk_on(wx, Wn, Wf);
        return tx;
    }
};
// one map: the soft modes want the logit itself, the boolean modes only its sign
template <bool SOFT>
struct MapUp : RowsUp {
    const float *__restrict__ logits;
    __device__ __forceinline__ double take(int) {
        const double v = logit_up(logits + top, logits + bot, next_tap(), ty);
        return SOFT ? v / (double)(4 * Hf * Wf) : v;
    }
    __device__ __forceinline__ double at(int64_t) { return take(0); }
};
// K maps: the taps of a pixel are taken once and applied to all K maps, the merge rule then runs on the fp64 values
struct MapsUp : RowsUp {
    const ObjectLogits &maps;
    int K;
    __device__ __forceinline__ uint32_t take(int) {
        const Tap tx = next_tap();
        double bv = -1.0;
        uint32_t label = 0u;
        for (int k = 0; k < K; ++k) merge_take(logit_up(maps.p[k] + top, maps.p[k] + bot, tx, ty), (uint32_t)k, bv, label);
        return label;
    }
    __device__ __forceinline__ uint32_t at(int64_t) { return take(0); }
};
// One map painted into a window of the frame (util/frame_roi.py): the segments, the anchor and the store are RowsUp's, the
// frame's.  Inside the frame's sanitised window a pixel's value is MapUp's with (Hw, Ww) in place of (Hf, Wf) and the pixel
// counted from the window's corner; outside it the value is -inf, which every paint reads as "not object": the boolean test
// fails, and the fp64 sigmoid of -inf is 1 / (1 + inf) = 0.0 exactly, so the frame's byte (or a 0 mask byte) comes out.
// The column walk stands at the window's first column until the pixels reach it and is never read behind its last one.  A
// thread reads its frame's window itself: the threads of a wave may lie in two frames.
template <bool SOFT>
struct MapUpWindow {
    using Store = uint4;
    int Hf, Wf, Hn, Wn;
    const float *__restrict__ logits;
    const int32_t *__restrict__ windows;
    Rect w;
    Tap ty;
    Walk wx;
    int64_t top, bot;
    int x;  // the output column of the next pixel taken
    bool row_in;
    __device__ __forceinline__ int64_t length() const { return Wf; }
    __device__ __forceinline__ Span open(int64_t gid, int64_t seg, int64_t slots, const uint8_t *dst, int bytes) {
        const int64_t n = seg / Hf;
        const int y = (int)(seg - n * Hf);
        const int32_t *__restrict__ wp = windows + 4 * n;
        w = sane_window(wp[0], wp[1], wp[2], wp[3], Hf, Wf, Hn, Wn);
        row_in = y >= w.y0 && y < w.y0 + w.H;
        ty = tap_of(walk_from(row_in ? y - w.y0 : 0, Hn, w.H), Hn, w.H);
        top = (n * Hn + ty.i0) * Wn, bot = (n * Hn + ty.i1) * Wn;
        const Span s = span_of_row(gid, seg, slots, Wf, dst, bytes);
        x = (int)s.qa;
        wx = walk_from(max(x - w.x0, 0), Wn, w.W);
        return s;
    }
    __device__ __forceinline__ void load_group(int64_t) {}
    __device__ __forceinline__ double take(int) {
        const bool in = row_in && x >= w.x0 && x < w.x0 + w.W;
        ++x;
        double v = -INFINITY;
        if (in) {
            const Tap tx = tap_of(wx, Wn, w.W);
            walk_on(wx, Wn, w.W);
            v = logit_up(logits + top, logits + bot, tx, ty);
            if (SOFT) v = v / (double)(4 * w.H * w.W);
        }
        return v;
    }
    __device__ __forceinline__ double at(int64_t) { return take(0); }
};

// Edge-aware upsampling (util/guided_upsample.py): the value of a pixel is the PAIR (A, Bv), 4 Hf Wf times the interpolated
// abar and bbar of the coefficient maps fp64 [N,2,Hn,Wn] (csrc/guided.hip) - RowsUp's segments, anchor, store and taps, applied
// to two fp64 maps.  The paint below reduces the pair with the pixel's own bytes.
struct Pair {
    double a, b;
};
// The pixels of a thread walk along one output row, and Wn <= Wf: the column taps move on by at most one map column a pixel.
// So the thread keeps the two map columns of the last taps - four doubles each: abar and bbar at the rows of ty - and loads
// a column only when a tap reaches one it does not hold: about 4 Wn / Wf loads a pixel in place of 8.  The values are the
// map's either way.
struct Column {
    double at, ab, bt, bb;  // abar at the top and bottom row of ty, bbar likewise
};
struct PairUp : RowsUp {
    const double *__restrict__ coeff;
    const double *__restrict__ ca = nullptr;  // the frame's abar map; bbar lies one plane behind it
    int64_t plane = 0;
    int k0 = -1, k1 = -1;  // the map columns held in c0, c1
    Column c0 = {}, c1 = {};
    __device__ __forceinline__ Span open(int64_t gid, int64_t seg, int64_t slots, const uint8_t *dst, int bytes) {
        const Span s = RowsUp::open(gid, seg, slots, dst, bytes);
        plane = (int64_t)Hn * Wn;
        ca = coeff + (seg / Hf) * 2 * plane;
        top = (int64_t)ty.i0 * Wn, bot = (int64_t)ty.i1 * Wn;  // rows of the frame's own maps
        return s;
    }
    __device__ __forceinline__ Column column(int i) const {
        return Column{ca[top + i], ca[bot + i], ca[plane + top + i], ca[plane + bot + i]};
    }
    __device__ __forceinline__ Pair take(int) {
        const Tap tx = next_tap();
        if (tx.i0 != k0) {  // (first c0 from the old c1, then c1 from the new c0)
            if (tx.i0 == k1)
                c0 = c1;
            else
                c0 = column(tx.i0);
            k0 = tx.i0;
        }
        if (tx.i1 != k1) {
            if (tx.i1 == k0)
                c1 = c0;
            else
                c1 = column(tx.i1);
            k1 = tx.i1;
        }
        Pair v;  // value_up's expressions on the held columns
        v.a = (c0.at * tx.w0 + c1.at * tx.w1) * ty.w0 + (c0.ab * tx.w0 + c1.ab * tx.w1) * ty.w1;
        v.b = (c0.bt * tx.w0 + c1.bt * tx.w1) * ty.w0 + (c0.bb * tx.w0 + c1.bb * tx.w1) * ty.w1;
        return v;
    }
    __device__ __forceinline__ Pair at(int64_t) { return take(0); }
};
// The guided paint: I = (b0 - m0) + (b1 - m1) + (b2 - m2) in fp64, the guide of the (mirrored) frame pixel; v = A I + Bv, which
// is 4 Hf Wf times the refined logit - its sign for the boolean modes, v / scale for the soft ones - and then the paint of
// the mode as it is.  It reads the frame in every mode.
template <int MODE, typename Inner>
struct Guided {
    static constexpr int kBytes = Inner::kBytes;
    static constexpr bool kReadsFrame = true;
    Inner inner;
    double m[3];
    double scale;  // 4 Hf Wf
    __device__ __forceinline__ void operator()(const Pair &p, const uint32_t (&b)[3], uint32_t (&o)[3]) const {
        const double I = (((double)b[0] - m[0]) + ((double)b[1] - m[1])) + ((double)b[2] - m[2]);
        const double v = p.a * I + p.b;
        inner((MODE & 1) ? v / scale : v, b, o);
    }
};

// ------------------------------------------------------------------------------------------ the overlays: the skeleton
__device__ __forceinline__ void store16(bytes16 *__restrict__ p, const uint32_t *o) {
    bytes16 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) t.w[i] = o[i];
    *p = t;
}
__device__ __forceinline__ void store16(uint4 *__restrict__ p, const uint32_t *o) { *p = make_uint4(o[0], o[1], o[2], o[3]); }

// Every overlay kernel is this body: the thread's span of its segment; for a full group the 48 frame bytes, unpacked
// through the mirror permutation, a value and a paint per pixel, the bytes packed into 12 or 4 registers and stored as
// three or one 16-byte runs; for a head or tail the same per pixel, byte by byte.
template <bool MIRROR, typename Source, typename Paint>
__device__ __forceinline__ void paint_pixels(Source from, const Paint paint, const uint8_t *__restrict__ frames,
                                             uint8_t *__restrict__ out, int64_t slots, int64_t total) {
    constexpr int NB = Paint::kBytes;
    constexpr bool FRAME = Paint::kReadsFrame;
    const int64_t gid = (int64_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (gid >= total) return;
    const int64_t seg = segment_of(gid, slots), L = from.length();
    const uint8_t *__restrict__ src = FRAME ? frames + seg * 3 * L : nullptr;
    uint8_t *__restrict__ dst = out + seg * NB * L;
    const Span s = from.open(gid, seg, slots, dst, NB);
    if (__builtin_expect(s.qb - s.qa == kGroup, 1)) {  // nearly every thread: keeps the group's code in the straight line
        from.load_group(s.qa);
        uint32_t w[12], o[4 * NB];
        if constexpr (FRAME) load48(src + 3 * (MIRROR ? L - kGroup - s.qa : s.qa), w);
#pragma unroll
        for (int k = 0; k < 4 * NB; ++k) o[k] = 0;
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            const auto v = from.take(i);
            uint32_t b[3] = {0, 0, 0}, ob[3];
            if constexpr (FRAME) {
                const int px = MIRROR ? kGroup - 1 - i : i;
#pragma unroll
                for (int c = 0; c < 3; ++c) b[c] = byte_at(w, 3 * px + c);
            }
            paint(v, b, ob);
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                const int at = NB * i + c;
                o[at >> 2] |= ob[c] << (8 * (at & 3));
            }
        }
        typename Source::Store *__restrict__ ov = reinterpret_cast<typename Source::Store *>(dst + NB * s.qa);
#pragma unroll
        for (int k = 0; k < NB; ++k) store16(ov + k, o + 4 * k);
    } else {
        for (int64_t q = s.qa; q < s.qb; ++q) {
            const auto v = from.at(q);
            uint32_t b[3] = {0, 0, 0}, ob[3];
            if constexpr (FRAME) {
                const int64_t sp = MIRROR ? L - 1 - q : q;
#pragma unroll
                for (int c = 0; c < 3; ++c) b[c] = src[3 * sp + c];
            }
            paint(v, b, ob);
#pragma unroll
            for (int c = 0; c < NB; ++c) dst[NB * q + c] = (uint8_t)ob[c];
        }
    }
}

// ------------------------------------------------------------------------------------------ the overlays: the kernels
// MODE 0, 1 the overlay, MODE 2, 3 the mask (never mirrored: the logits already are in output order)
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay(const uint8_t *__restrict__ frames,
                                                            const float *__restrict__ logits, uint8_t *__restrict__ out,
                                                            int64_t L, int64_t slots, int64_t total, int channel,
                                                            double a255) {
    if constexpr (MODE < 2)
        paint_pixels<MIRROR>(MapInPlace{logits, L}, OneChannel<MODE>{channel, a255}, frames, out, slots, total);
    else
        paint_pixels<MIRROR>(MapInPlace{logits, L}, OneByte<MODE>{}, frames, out, slots, total);
}
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_scaled(const uint8_t *__restrict__ frames,
                                                                   const float *__restrict__ logits, uint8_t *__restrict__ out,
                                                                   int Hf, int Wf, int Hn, int Wn, int64_t slots, int64_t total,
                                                                   int channel, double a255) {
    const MapUp<(MODE & 1) != 0> from = {{Hf, Wf, Hn, Wn}, logits};
    if constexpr (MODE < 2)
        paint_pixels<MIRROR>(from, OneChannel<MODE>{channel, a255}, frames, out, slots, total);
    else
        paint_pixels<MIRROR>(from, OneByte<MODE>{}, frames, out, slots, total);
}
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_window(const uint8_t *__restrict__ frames,
                                                                   const float *__restrict__ logits,
                                                                   const int32_t *__restrict__ windows, uint8_t *__restrict__ out,
                                                                   int Hf, int Wf, int Hn, int Wn, int64_t slots, int64_t total,
                                                                   int channel, double a255) {
    const MapUpWindow<(MODE & 1) != 0> from = {Hf, Wf, Hn, Wn, logits, windows};
    if constexpr (MODE < 2)
        paint_pixels<MIRROR>(from, OneChannel<MODE>{channel, a255}, frames, out, slots, total);
    else
        paint_pixels<MIRROR>(from, OneByte<MODE>{}, frames, out, slots, total);
}

// every mode mirrors here: the mask modes read the (mirrored) frame too
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_guided(const uint8_t *__restrict__ frames,
                                                                   const double *__restrict__ coeff, uint8_t *__restrict__ out,
                                                                   int Hf, int Wf, int Hn, int Wn, int64_t slots, int64_t total,
                                                                   int channel, double a255, MeanBGR mean) {
    const PairUp from = {{Hf, Wf, Hn, Wn}, coeff};
    const double m0 = (double)mean.v[0], m1 = (double)mean.v[1], m2 = (double)mean.v[2], scale = (double)(4 * Hf * Wf);
    if constexpr (MODE < 2)
        paint_pixels<MIRROR>(from, Guided<MODE, OneChannel<MODE>>{{channel, a255}, {m0, m1, m2}, scale}, frames, out, slots, total);
    else
        paint_pixels<MIRROR>(from, Guided<MODE, OneByte<MODE>>{{}, {m0, m1, m2}, scale}, frames, out, slots, total);
}

// ------------------------------------------------------------------------------------------ window_next
// The window of the next frame from this frame's logits (util/frame_roi.next_window), two launches:
//   k_window_reset  one thread a frame: the frame's box (min row, max row, min column, max column) to (INT_MAX, -1, INT_MAX,
//                   -1) and its count of finished workgroups to 0.
//   k_window_next   a workgroup owns kBoxRows rows of one frame's map, a wave one row at a time, a lane one column of a segment
//                   of 64: __ballot(logit >= 0) of a segment gives its first and last object column, and a non-zero ballot
//                   makes the row an object row - all in scalar registers.  The four waves meet in LDS, and thread 0 puts the
//                   workgroup's four bounds into the frame's box with one agent-scope atomic min / max each (none where the
//                   workgroup saw no object).  Min and max commute: no order of workgroups changes the box.  Thread 0 then
//                   counts its workgroup as finished (acquire-release); the one that counts last - nobody waits for it - has
//                   every bound before it, turns the box into the next window and stores it.  Only that thread reads
//                   `in`, after every logit was read, so `out` may be `in`.
constexpr int kBoxRows = 8;
constexpr int kBoxWords = 5;  // int32 a frame in the workspace: the box and the count
#define WIN_AGENT __HIP_MEMORY_SCOPE_AGENT

__global__ void k_window_reset(int32_t *__restrict__ box, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int32_t *b = box + (int64_t)kBoxWords * n;
    b[0] = INT_MAX, b[1] = -1, b[2] = INT_MAX, b[3] = -1, b[4] = 0;
}

struct NextGeom {
    int Hf, Wf, Hn, Wn, levels, permille, min_pad, strips;
};
// steps 3 to 7 of util/frame_roi.next_window.  Every product stays below 2^27: sides <= 8192, levels <= 64, permille <= 4000
__device__ __forceinline__ Rect window_from_box(int i_min, int i_max, int j_min, int j_max, const Rect w, const NextGeom &g) {
    if (i_max < 0) return Rect{0, 0, g.Hf, g.Wf};
    const int by0 = w.y0 + i_min * w.H / g.Hn, by1 = w.y0 + ((i_max + 1) * w.H + g.Hn - 1) / g.Hn;
    const int bx0 = w.x0 + j_min * w.W / g.Wn, bx1 = w.x0 + ((j_max + 1) * w.W + g.Wn - 1) / g.Wn;
    const int pad = g.min_pad + (g.permille * max(by1 - by0, bx1 - bx0) + 999) / 1000;
    const int need_h = min(g.Hf, by1 - by0 + 2 * pad), need_w = min(g.Wf, bx1 - bx0 + 2 * pad);
    int Hk = g.Hf, Wk = g.Wf;  // level `levels`
    for (int k = 0; k < g.levels; ++k) {
        const int h = g.Hn + (g.Hf - g.Hn) * k / g.levels, ww = g.Wn + (g.Wf - g.Wn) * k / g.levels;
        if (h >= need_h && ww >= need_w) {
            Hk = h, Wk = ww;
            break;
        }
    }
    // floor((a + b - size) / 2) of a sum that may be negative: the arithmetic shift
    const int y0 = min(max((by0 + by1 - Hk) >> 1, 0), g.Hf - Hk), x0 = min(max((bx0 + bx1 - Wk) >> 1, 0), g.Wf - Wk);
    return Rect{y0, x0, Hk, Wk};
}

__global__ __launch_bounds__(kStreamThreads) void k_window_next(const float *__restrict__ logits,
                                                                const int32_t *win_in, int32_t *win_out,
                                                                int32_t *__restrict__ box, NextGeom g) {
    __shared__ int part[kStreamThreads / 64][4];
    const int strip = (int)(blockIdx.x % g.strips);
    const int64_t n = blockIdx.x / g.strips;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *__restrict__ map = logits + n * g.Hn * g.Wn;
    int i_min = INT_MAX, i_max = -1, j_min = INT_MAX, j_max = -1;
    const int i_end = min((strip + 1) * kBoxRows, g.Hn);
    for (int i = strip * kBoxRows + wave; i < i_end; i += kStreamThreads / 64) {
        const float *__restrict__ row = map + (int64_t)i * g.Wn;
        for (int j0 = 0; j0 < g.Wn; j0 += 64) {
            const int j = j0 + lane;
            const unsigned long long m = __ballot(j < g.Wn && row[min(j, g.Wn - 1)] >= 0.f);  // a NaN is not >= 0, -0.0 is
            if (m) {
                i_min = min(i_min, i), i_max = max(i_max, i);
                j_min = min(j_min, j0 + (int)__builtin_ctzll(m)), j_max = max(j_max, j0 + 63 - (int)__builtin_clzll(m));
            }
        }
    }
    if (lane == 0) part[wave][0] = i_min, part[wave][1] = i_max, part[wave][2] = j_min, part[wave][3] = j_max;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kStreamThreads / 64; ++k) {
        i_min = min(i_min, part[k][0]), i_max = max(i_max, part[k][1]);
        j_min = min(j_min, part[k][2]), j_max = max(j_max, part[k][3]);
    }
    int32_t *b = box + (int64_t)kBoxWords * n;
    if (i_max >= 0) {
        __hip_atomic_fetch_min(b + 0, i_min, __ATOMIC_RELAXED, WIN_AGENT);
        __hip_atomic_fetch_max(b + 1, i_max, __ATOMIC_RELAXED, WIN_AGENT);
        __hip_atomic_fetch_min(b + 2, j_min, __ATOMIC_RELAXED, WIN_AGENT);
        __hip_atomic_fetch_max(b + 3, j_max, __ATOMIC_RELAXED, WIN_AGENT);
    }
    // release what this workgroup put into the box, acquire what every workgroup counted before it did
    if (__hip_atomic_fetch_add(b + 4, 1, __ATOMIC_ACQ_REL, WIN_AGENT) != g.strips - 1) return;
    const int32_t *wp = win_in + 4 * n;  // (may be win_out: read here, stored below)
    const Rect w = sane_window(wp[0], wp[1], wp[2], wp[3], g.Hf, g.Wf, g.Hn, g.Wn);
    const Rect next = window_from_box(__hip_atomic_load(b + 0, __ATOMIC_RELAXED, WIN_AGENT),
                                      __hip_atomic_load(b + 1, __ATOMIC_RELAXED, WIN_AGENT),
                                      __hip_atomic_load(b + 2, __ATOMIC_RELAXED, WIN_AGENT),
                                      __hip_atomic_load(b + 3, __ATOMIC_RELAXED, WIN_AGENT), w, g);
    int32_t *o = win_out + 4 * n;
    o[0] = next.y0, o[1] = next.x0, o[2] = next.H, o[3] = next.W;
}

template <bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_objects(const uint8_t *__restrict__ frames, const ObjectLogits maps,
                                                                    int K, const uint8_t *__restrict__ palette,
                                                                    uint8_t *__restrict__ out, int64_t L, int64_t slots,
                                                                    int64_t total, double alpha) {
    __shared__ uint32_t cols[kMaxObjects + 1];
    stage_colours(palette, K, cols);
    paint_pixels<MIRROR>(MapsInPlace{maps, K, L}, PaletteBlend{cols, alpha}, frames, out, slots, total);
}
// MODE 0: the overlay; MODE 1: the label map, one byte a pixel, which needs no colours
template <int MODE, bool MIRROR>
__global__ __launch_bounds__(kStreamThreads) void k_overlay_objects_scaled(const uint8_t *__restrict__ frames,
                                                                           const ObjectLogits maps, int K,
                                                                           const uint8_t *__restrict__ palette,
                                                                           uint8_t *__restrict__ out, int Hf, int Wf, int Hn,
                                                                           int Wn, int64_t slots, int64_t total, double alpha) {
    const MapsUp from = {{Hf, Wf, Hn, Wn}, maps, K};
    if constexpr (MODE == 0) {
        __shared__ uint32_t cols[kMaxObjects + 1];
        stage_colours(palette, K, cols);
        paint_pixels<MIRROR>(from, PaletteBlend{cols, alpha}, frames, out, slots, total);
    } else {
        paint_pixels<MIRROR>(from, LabelByte{}, frames, out, slots, total);
    }
}

// ------------------------------------------------------------------------------------------ host
// segments and threads of a launch
struct Partition {
    int64_t L, slots, total;
    int R;
    dim3 grid;
};
inline Partition partition_of(int N, int H, int W, int mirror) {
    Partition p;
    p.R = mirror ? H : 1;
    p.L = mirror ? (int64_t)W : (int64_t)H * W;
    p.slots = p.L / kGroup + 2;
    p.total = (int64_t)N * p.R * p.slots;
    p.grid = dim3((unsigned)cdiv(p.total, kStreamThreads));
    return p;
}
constexpr int64_t kMaxPixels = (int64_t)1 << 36;  // N H W: keeps every count far inside int64 and the grid inside 2^31

// `mirror` as a template argument: f(std::true_type) or f(std::false_type)
template <typename F>
void with_mirror(int mirror, F &&f) {
    if (mirror)
        f(std::true_type{});
    else
        f(std::false_type{});
}
// the mode of a one-map overlay as well: f(mode, mirror).  A mask (modes 2, 3) has nothing to mirror
template <typename F>
void with_mode(int mode, int mirror, F &&f) {
    switch (mode) {
        case 0: with_mirror(mirror, [&](auto m) { f(std::integral_constant<int, 0>{}, m); }); break;
        case 1: with_mirror(mirror, [&](auto m) { f(std::integral_constant<int, 1>{}, m); }); break;
        case 2: f(std::integral_constant<int, 2>{}, std::false_type{}); break;
        default: f(std::integral_constant<int, 3>{}, std::false_type{}); break;
    }
}

// the same where a mask mirrors as well (the guided paint reads the frame in every mode)
template <typename F>
void with_mode_and_mirror(int mode, int mirror, F &&f) {
    switch (mode) {
        case 0: with_mirror(mirror, [&](auto m) { f(std::integral_constant<int, 0>{}, m); }); break;
        case 1: with_mirror(mirror, [&](auto m) { f(std::integral_constant<int, 1>{}, m); }); break;
        case 2: with_mirror(mirror, [&](auto m) { f(std::integral_constant<int, 2>{}, m); }); break;
        default: with_mirror(mirror, [&](auto m) { f(std::integral_constant<int, 3>{}, m); }); break;
    }
}

// the sizes of a call at the frames' size
int check_frames(const char *who, int N, int H, int W) {
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && (int64_t)N * H * W <= kMaxPixels, FOSVOS_E_SHAPE, "%s: N=%d H=%d W=%d", who, N, H, W);
    return FOSVOS_OK;
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
// a one-map overlay, in front of its sizes: the mode and the pointers (a mask reads no frames) ...
int check_map(const char *who, int mode, const uint8_t *frames, const float *logits, const uint8_t *out) {
    FOSVOS_REQUIRE(mode >= 0 && mode <= 3, FOSVOS_E_ARG, "%s: mode %d outside [0, 3]", who, mode);
    FOSVOS_REQUIRE(logits && out && (frames || mode >= 2), FOSVOS_E_ARG, "%s: null pointer", who);
    return FOSVOS_OK;
}
// ... and behind them: what it paints with
int check_level(const char *who, int channel, double alpha, const float *logits) {
    FOSVOS_REQUIRE(channel >= 0 && channel <= 2, FOSVOS_E_ARG, "%s: channel %d outside [0, 2]", who, channel);
    FOSVOS_REQUIRE(alpha >= 0.0 && isfinite(alpha), FOSVOS_E_ARG, "%s: alpha %g is not a finite number >= 0", who, alpha);
    FOSVOS_REQUIRE(((uintptr_t)logits & 3) == 0, FOSVOS_E_ARG, "%s: the logits must be 4-byte aligned", who);
    return FOSVOS_OK;
}
// a several-objects overlay, in front of its sizes: the K pointers, by value from here on, and the others (a label map,
// `blend` false, reads neither frames nor palette) ...
int check_maps(const char *who, const float *const *logits, int K, ObjectLogits &maps, bool blend, const uint8_t *frames,
               const uint8_t *palette, const uint8_t *out) {
    FOSVOS_REQUIRE(K >= 1 && K <= kMaxObjects, FOSVOS_E_ARG, "%s: K=%d outside [1, %d]", who, K, kMaxObjects);
    FOSVOS_REQUIRE(logits, FOSVOS_E_ARG, "%s: null pointer", who);
    for (int k = 0; k < K; ++k) {
        FOSVOS_REQUIRE(logits[k] != nullptr, FOSVOS_E_ARG, "%s: null logit map %d", who, k);
        FOSVOS_REQUIRE(((uintptr_t)logits[k] & 3) == 0, FOSVOS_E_ARG, "%s: logit map %d must be 4-byte aligned", who, k);
        maps.p[k] = logits[k];
    }
    FOSVOS_REQUIRE(out && ((frames && palette) || !blend), FOSVOS_E_ARG, "%s: null pointer", who);
    return FOSVOS_OK;
}
// ... and behind them: how far it blends
int check_blend(const char *who, bool blend, double alpha) {
    FOSVOS_REQUIRE(!blend || (alpha >= 0.0 && alpha <= 1.0), FOSVOS_E_ARG, "%s: alpha %g is not a number in [0, 1]", who, alpha);
    return FOSVOS_OK;
}
// the windows of a call: int32 [N][4] in device memory, read by the kernels alone
int check_windows(const char *who, const int32_t *windows) {
    FOSVOS_REQUIRE(windows != nullptr, FOSVOS_E_ARG, "%s: null pointer", who);
    FOSVOS_REQUIRE(((uintptr_t)windows & 3) == 0, FOSVOS_E_ARG, "%s: the windows must be 4-byte aligned", who);
    return FOSVOS_OK;
}
// fosvos_frame_prep_scaled (windows == nullptr) and fosvos_frame_prep_window: one geometry, one launch.  The stage is sized
// for the whole frame, the largest source there is, so nothing here depends on what the windows hold.
int prep_scaled_launch(const char *who, const uint8_t *frames, const int32_t *windows, int N, int Hf, int Wf, int Hn, int Wn,
                       int mirror, const float mean[3], float *image, int device, void *stream) {
    FOSVOS_REQUIRE(frames && mean && image, FOSVOS_E_ARG, "%s: null pointer", who);
    if (int rc = check_sizes(who, N, Hf, Wf, Hn, Wn)) return rc;
    FOSVOS_REQUIRE(((uintptr_t)image & 3) == 0, FOSVOS_E_ARG, "%s: the image must be 4-byte aligned", who);
    FOSVOS_ENTER(device);
    ScaleGeom g = {Hf, Wf, Hn, Wn, 0, 0, 0, 0};
    // the source pixels under a workgroup's columns (64, and up to 3 more in front), cut to the chunk; the rows under its rows
    const int64_t under = cdiv((int64_t)(4 * kScaleCells + 3) * Wf, Wn) + 1;
    g.pitch = roundup(3 * (int)std::min<int64_t>(under, kScaleChunkPx), 16);
    g.rows = (int)std::min<int64_t>(cdiv((int64_t)kScaleRows * Hf, Hn) + 1, kScaleStageBytes / g.pitch);
    g.tiles = (int)cdiv(cdiv(Wn + 3, 4), kScaleCells);
    g.strips = (int)cdiv(Hn, kScaleRows);
    const int64_t blocks = (int64_t)N * g.tiles * g.strips;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "%s: %lld workgroups", who, (long long)blocks);
    const MeanBGR m = {{mean[0], mean[1], mean[2]}};
    const int64_t frame_bytes = (int64_t)N * Hf * Wf * 3;
    const size_t lds = (size_t)g.pitch * g.rows;
    FOSVOS_PROF(windows ? "k_frame_prep_window" : "k_frame_prep_scaled", stream, 0.0);
    with_mirror(mirror, [&](auto mi) {
        if (windows)
            hipLaunchKernelGGL(k_frame_prep_window<decltype(mi)::value>, dim3((unsigned)blocks), dim3(kScaleThreads), lds,
                               (hipStream_t)stream, frames, windows, image, g, frame_bytes, m);
        else
            hipLaunchKernelGGL(k_frame_prep_scaled<decltype(mi)::value>, dim3((unsigned)blocks), dim3(kScaleThreads), lds,
                               (hipStream_t)stream, frames, image, g, frame_bytes, m);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
}  // namespace

extern "C" int fosvos_frame_prep(const uint8_t *frames, int N, int H, int W, int mirror, const float mean[3], float *image,
                                 int device, void *stream) {
    FOSVOS_REQUIRE(frames && mean && image, FOSVOS_E_ARG, "frame_prep: null pointer");
    if (int rc = check_frames("frame_prep", N, H, W)) return rc;
    FOSVOS_REQUIRE(((uintptr_t)image & 3) == 0, FOSVOS_E_ARG, "frame_prep: the image must be 4-byte aligned");
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, H, W, mirror);
    const int64_t plane = (int64_t)H * W;
    const MeanBGR m = {{mean[0], mean[1], mean[2]}};
    FOSVOS_PROF("k_frame_prep", stream, 0.0);
    with_mirror(mirror, [&](auto mi) {
        hipLaunchKernelGGL(k_frame_prep<decltype(mi)::value>, p.grid, dim3(kStreamThreads), 0, (hipStream_t)stream, frames, image,
                           p.L, p.R, plane, p.slots, p.total, m);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay(const uint8_t *frames, const float *logits, int N, int H, int W, int mirror, int mode, int channel,
                              double alpha, uint8_t *out, int device, void *stream) {
    if (int rc = check_map("overlay", mode, frames, logits, out)) return rc;
    if (int rc = check_frames("overlay", N, H, W)) return rc;
    if (int rc = check_level("overlay", channel, alpha, logits)) return rc;
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, H, W, mode < 2 ? mirror : 0);
    FOSVOS_PROF("k_overlay", stream, 0.0);
    with_mode(mode, mirror, [&](auto mo, auto mi) {
        hipLaunchKernelGGL((k_overlay<decltype(mo)::value, decltype(mi)::value>), p.grid, dim3(kStreamThreads), 0,
                           (hipStream_t)stream, frames, logits, out, p.L, p.slots, p.total, channel, alpha * 255.0);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_frame_prep_scaled(const uint8_t *frames, int N, int Hf, int Wf, int Hn, int Wn, int mirror,
                                        const float mean[3], float *image, int device, void *stream) {
    return prep_scaled_launch("frame_prep_scaled", frames, nullptr, N, Hf, Wf, Hn, Wn, mirror, mean, image, device, stream);
}

extern "C" int fosvos_frame_prep_window(const uint8_t *frames, const int32_t *windows, int N, int Hf, int Wf, int Hn, int Wn,
                                        int mirror, const float mean[3], float *image, int device, void *stream) {
    if (int rc = check_windows("frame_prep_window", windows)) return rc;
    return prep_scaled_launch("frame_prep_window", frames, windows, N, Hf, Wf, Hn, Wn, mirror, mean, image, device, stream);
}

extern "C" int fosvos_overlay_window(const uint8_t *frames, const float *logits, const int32_t *windows, int N, int Hf, int Wf,
                                     int Hn, int Wn, int mirror, int mode, int channel, double alpha, uint8_t *out, int device,
                                     void *stream) {
    if (int rc = check_map("overlay_window", mode, frames, logits, out)) return rc;
    if (int rc = check_windows("overlay_window", windows)) return rc;
    if (int rc = check_sizes("overlay_window", N, Hf, Wf, Hn, Wn)) return rc;
    if (int rc = check_level("overlay_window", channel, alpha, logits)) return rc;
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, Hf, Wf, 1);  // rows, in every mode: the frame's grid
    FOSVOS_PROF("k_overlay_window", stream, 0.0);
    with_mode(mode, mirror, [&](auto mo, auto mi) {
        hipLaunchKernelGGL((k_overlay_window<decltype(mo)::value, decltype(mi)::value>), p.grid, dim3(kStreamThreads), 0,
                           (hipStream_t)stream, frames, logits, windows, out, Hf, Wf, Hn, Wn, p.slots, p.total, channel,
                           alpha * 255.0);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" size_t fosvos_window_next_workspace_bytes(int N) {
    return N > 0 ? (size_t)N * kBoxWords * sizeof(int32_t) : 0;
}

extern "C" int fosvos_window_next(const float *logits, const int32_t *windows, int N, int Hf, int Wf, int Hn, int Wn, int levels,
                                  int margin_permille, int min_pad, int32_t *out, void *workspace, size_t workspace_bytes,
                                  int device, void *stream) {
    FOSVOS_REQUIRE(logits && out && workspace, FOSVOS_E_ARG, "window_next: null pointer");
    if (int rc = check_windows("window_next", windows)) return rc;
    if (int rc = check_sizes("window_next", N, Hf, Wf, Hn, Wn)) return rc;
    FOSVOS_REQUIRE(levels >= 1 && levels <= 64, FOSVOS_E_ARG, "window_next: levels %d outside [1, 64]", levels);
    FOSVOS_REQUIRE(margin_permille >= 0 && margin_permille <= 4000, FOSVOS_E_ARG, "window_next: margin of %d permille outside [0, 4000]",
                   margin_permille);
    FOSVOS_REQUIRE(min_pad >= 0 && min_pad <= 4095, FOSVOS_E_ARG, "window_next: min_pad %d outside [0, 4095]", min_pad);
    FOSVOS_REQUIRE((((uintptr_t)logits | (uintptr_t)out | (uintptr_t)workspace) & 3) == 0, FOSVOS_E_ARG,
                   "window_next: the logits, the windows and the workspace must be 4-byte aligned");
    FOSVOS_REQUIRE(workspace_bytes >= fosvos_window_next_workspace_bytes(N), FOSVOS_E_ARG, "window_next: workspace of %zu bytes, need %zu",
                   workspace_bytes, fosvos_window_next_workspace_bytes(N));
    const NextGeom g = {Hf, Wf, Hn, Wn, levels, margin_permille, min_pad, (int)cdiv(Hn, kBoxRows)};
    const int64_t blocks = (int64_t)N * g.strips;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "window_next: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    int32_t *box = static_cast<int32_t *>(workspace);
    FOSVOS_PROF("k_window_reset", stream, 0.0);
    hipLaunchKernelGGL(k_window_reset, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, box, N);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_window_next", stream, 0.0);
    hipLaunchKernelGGL(k_window_next, dim3((unsigned)blocks), dim3(kStreamThreads), 0, (hipStream_t)stream, logits, windows, out, box,
                       g);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay_scaled(const uint8_t *frames, const float *logits, int N, int Hf, int Wf, int Hn, int Wn,
                                     int mirror, int mode, int channel, double alpha, uint8_t *out, int device, void *stream) {
    if (int rc = check_map("overlay_scaled", mode, frames, logits, out)) return rc;
    if (int rc = check_sizes("overlay_scaled", N, Hf, Wf, Hn, Wn)) return rc;
    if (int rc = check_level("overlay_scaled", channel, alpha, logits)) return rc;
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, Hf, Wf, 1);  // rows, in every mode
    FOSVOS_PROF("k_overlay_scaled", stream, 0.0);
    with_mode(mode, mirror, [&](auto mo, auto mi) {
        hipLaunchKernelGGL((k_overlay_scaled<decltype(mo)::value, decltype(mi)::value>), p.grid, dim3(kStreamThreads), 0,
                           (hipStream_t)stream, frames, logits, out, Hf, Wf, Hn, Wn, p.slots, p.total, channel, alpha * 255.0);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay_guided(const uint8_t *frames, const double *coeff, int N, int Hf, int Wf, int Hn, int Wn, int mirror,
                                     int mode, int channel, double alpha, const float mean[3], uint8_t *out, int device,
                                     void *stream) {
    FOSVOS_REQUIRE(mode >= 0 && mode <= 3, FOSVOS_E_ARG, "overlay_guided: mode %d outside [0, 3]", mode);
    FOSVOS_REQUIRE(frames && coeff && mean && out, FOSVOS_E_ARG, "overlay_guided: null pointer");  // the frames in every mode
    if (int rc = check_sizes("overlay_guided", N, Hf, Wf, Hn, Wn)) return rc;
    FOSVOS_REQUIRE(channel >= 0 && channel <= 2, FOSVOS_E_ARG, "overlay_guided: channel %d outside [0, 2]", channel);
    FOSVOS_REQUIRE(alpha >= 0.0 && isfinite(alpha), FOSVOS_E_ARG, "overlay_guided: alpha %g is not a finite number >= 0", alpha);
    FOSVOS_REQUIRE(((uintptr_t)coeff & 7) == 0, FOSVOS_E_ARG, "overlay_guided: the coefficients must be 8-byte aligned");
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, Hf, Wf, 1);  // rows, in every mode
    const MeanBGR m = {{mean[0], mean[1], mean[2]}};
    FOSVOS_PROF("k_overlay_guided", stream, 0.0);
    with_mode_and_mirror(mode, mirror, [&](auto mo, auto mi) {
        hipLaunchKernelGGL((k_overlay_guided<decltype(mo)::value, decltype(mi)::value>), p.grid, dim3(kStreamThreads), 0,
                           (hipStream_t)stream, frames, coeff, out, Hf, Wf, Hn, Wn, p.slots, p.total, channel, alpha * 255.0, m);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay_objects(const uint8_t *frames, const float *const *logits, int K, int N, int H, int W, int mirror,
                                      const uint8_t *palette, double alpha, uint8_t *out, int device, void *stream) {
    ObjectLogits maps = {};
    if (int rc = check_maps("overlay_objects", logits, K, maps, true, frames, palette, out)) return rc;
    if (int rc = check_frames("overlay_objects", N, H, W)) return rc;
    if (int rc = check_blend("overlay_objects", true, alpha)) return rc;
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, H, W, mirror);
    FOSVOS_PROF("k_overlay_objects", stream, 0.0);
    with_mirror(mirror, [&](auto mi) {
        hipLaunchKernelGGL(k_overlay_objects<decltype(mi)::value>, p.grid, dim3(kStreamThreads), 0, (hipStream_t)stream, frames,
                           maps, K, palette, out, p.L, p.slots, p.total, alpha);
    });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_overlay_objects_scaled(const uint8_t *frames, const float *const *logits, int K, int N, int Hf, int Wf,
                                             int Hn, int Wn, int mirror, int mode, const uint8_t *palette, double alpha,
                                             uint8_t *out, int device, void *stream) {
    FOSVOS_REQUIRE(mode == 0 || mode == 1, FOSVOS_E_ARG, "overlay_objects_scaled: mode %d outside [0, 1]", mode);
    ObjectLogits maps = {};
    if (int rc = check_maps("overlay_objects_scaled", logits, K, maps, mode == 0, frames, palette, out)) return rc;
    if (int rc = check_sizes("overlay_objects_scaled", N, Hf, Wf, Hn, Wn)) return rc;
    if (int rc = check_blend("overlay_objects_scaled", mode == 0, alpha)) return rc;
    FOSVOS_ENTER(device);
    const Partition p = partition_of(N, Hf, Wf, 1);  // rows, in both modes
    const dim3 block(kStreamThreads);
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_overlay_objects_scaled", stream, 0.0);
    if (mode == 1)  // a label map has nothing to mirror: the logits already are in output order
        hipLaunchKernelGGL((k_overlay_objects_scaled<1, false>), p.grid, block, 0, st, frames, maps, K, palette, out, Hf, Wf, Hn,
                           Wn, p.slots, p.total, alpha);
    else
        with_mirror(mirror, [&](auto mi) {
            hipLaunchKernelGGL((k_overlay_objects_scaled<0, decltype(mi)::value>), p.grid, block, 0, st, frames, maps, K, palette,
                               out, Hf, Wf, Hn, Wn, p.slots, p.total, alpha);
        });
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

