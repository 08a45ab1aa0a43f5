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
__device__ __forceinline__ Span span_of(int64_t gid, int64_t seg, int64_t slots, int64_t L, const float *anchor) {
    const int j = (int)(gid - seg * slots);
    const int k0 = (int)((16u - ((unsigned)(uintptr_t)anchor & 15u)) & 15u) >> 2;  // floats up to the 16-byte boundary
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

// ------------------------------------------------------------------------------------------ overlay
// the new byte of one pixel: `byte` is the frame's value in the overlay's channel (unused in the mask modes)
template <int MODE>
__device__ __forceinline__ uint32_t level(float x, uint32_t byte, double a255) {
    if (MODE == 2) return x >= 0.f ? 255u : 0u;
    if (MODE == 3) return (uint32_t)(255.0 * sigmoid_f64(x) + 0.5);
    const double p = MODE == 0 ? (x >= 0.f ? 1.0 : 0.0) : sigmoid_f64(x);
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
