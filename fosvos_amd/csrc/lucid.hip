// One-shot augmentation that moves the object against its background: one resident uint8 sample (the frame, the frame with the
// object painted out, the mask) -> the [1,3,H,W] image and [1,1,H,W] gt of dataloaders/lucid.py: compose, bit for bit.
//
// The host inverts both 2x3 matrices (np.linalg.inv in fp64) and passes the twelve doubles of destination -> source by value.
// Per output pixel (x, y), with (sx, sy) = ((i00*x + i01*y) + i02, (i10*x + i11*y) + i12) in fp64 under either matrix:
//   gt     the table value of the mask byte at rint (half to even) of the object's (sx, sy), 0 outside: warp.hip's rule.
//   alpha  the four taps of `mask != 0` at floor .. floor + 1 of the object's (sx, sy): the fractions as fp32, weights 1 - f and
//          f, row-outer / column-inner as acc = acc + val * (wy[j] * wx[i]) from +0.0, val = 0 outside the source.  n counts the
//          taps that are inside and on the object: n == 4 makes alpha exactly 1 (n == 0 leaves the sum, which is +0.0).
//   B, Fg  warp.hip's 16-tap bicubic gather of the background under the background's matrix and of the frame under the
//          object's.  B is gathered only where alpha != 1 and Fg only where alpha != 0: away from the object's outline a pixel
//          pays one gather.
//   out    B where alpha == 0, Fg where alpha == 1, else B + alpha * (Fg - B), every operation rounded; then out * gain[c] +
//          bias[c], two roundings.
// flip mirrors the three sources first: source column x is column W-1-x.  fg_on == 0 is no object: alpha = 0 and gt = 0
// everywhere, the mask, the frame and the object's matrix are not read.  Every tap's address is clamped into the frame before
// the load, so no matrix and no mask makes the kernel read outside its operands.
//
// A workgroup of 256 threads owns a tile of 64 x 4 output pixels, one thread a pixel, as k_warp: plain gathers of the
// (L2-resident) sources through the value table in LDS, one coalesced 256-byte store per wave and plane.  ONE launch; no
// workspace, no atomics, nothing waits for another workgroup.
#include <math.h>

#include "common.hpp"

// numpy rounds every product before the add: no multiply-add contraction anywhere in this file
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kLucidTileW = 64, kLucidTileH = 4, kLucidThreads = kLucidTileW * kLucidTileH;
constexpr int kLucidMaxSide = 8192;              // fosvos_hip/limits.py: MAX_FRAME_SIDE
constexpr double kLucidMaxCoord = 1073741824.0;  // 2^30: floor / rint of a source coordinate, and the taps' +-2, fit int32

struct LucidMatrix {
    double i00, i01, i02, i10, i11, i12;  // destination -> source
};

struct LucidArgs {
    LucidMatrix bg, fg;
    float gain[3], bias[3];
};

// custom_transforms._cubic_weights on one fraction, fp32, in numpy's order of operations (a = -0.75)
__device__ __forceinline__ void lucid_cubic_weights(float x, float (&w)[4]) {
    const float a = -0.75f;
    const float t = x + 1.0f;
    w[0] = ((a * t - 5.0f * a) * t + 8.0f * a) * t - 4.0f * a;
    w[1] = ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    const float u = 1.0f - x;
    w[2] = ((a + 2.0f) * u - (a + 3.0f)) * u * u + 1.0f;
    w[3] = 1.0f - w[0] - w[1] - w[2];
}

// warp_affine's bicubic branch for one pixel: the 4 x 4 taps of `src` [H,W,3] at floor - 1 .. floor + 2 of (sx, sy)
__device__ __forceinline__ void lucid_gather(const uint8_t *__restrict__ src, int H, int W, int flip, double sx, double sy,
                                             const float *lut, float (&acc)[3]) {
    const double fx = floor(sx), fy = floor(sy);
    const int bx = (int)fx, by = (int)fy;
    float wx[4], wy[4];
    lucid_cubic_weights((float)(sx - fx), wx);
    lucid_cubic_weights((float)(sy - fy), wy);
    acc[0] = acc[1] = acc[2] = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = by + j - 1;
        const bool row_in = yy >= 0 && yy < H;
        const uint8_t *__restrict__ row = src + (int64_t)min(max(yy, 0), H - 1) * W * 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = bx + i - 1;
            const bool in = row_in && xx >= 0 && xx < W;
            const int xc = min(max(xx, 0), W - 1);
            const uint8_t *__restrict__ p = row + 3 * (flip ? W - 1 - xc : xc);
            const float w = wy[j] * wx[i];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float val = in ? lut[p[ch] * 3 + ch] : 0.0f;
                acc[ch] = acc[ch] + val * w;
            }
        }
    }
}

// grid (ceil(W / 64), ceil(H / 4)), block (64, 4)
__global__ __launch_bounds__(kLucidThreads) void k_lucid(const uint8_t *__restrict__ frame,
                                                         const uint8_t *__restrict__ background,
                                                         const uint8_t *__restrict__ mask, int H, int W, int flip, int fg_on,
                                                         LucidArgs a, const float *__restrict__ img_lut,
                                                         const float *__restrict__ gt_lut, float *__restrict__ image,
                                                         float *__restrict__ gt) {
    __shared__ float lut[256 * 3];  // [256][3]: u8 - mean of each channel
    const int tid = threadIdx.y * kLucidTileW + threadIdx.x;
    for (int i = tid; i < 256 * 3; i += kLucidThreads) lut[i] = img_lut[i];
    __syncthreads();
    const int x = blockIdx.x * kLucidTileW + threadIdx.x, y = blockIdx.y * kLucidTileH + threadIdx.y;
    if (x >= W || y >= H) return;
    const int64_t px = (int64_t)y * W + x, plane = (int64_t)H * W;
    float alpha = 0.0f, g = 0.0f;
    double sx = 0.0, sy = 0.0;
    if (fg_on) {
        sx = (a.fg.i00 * (double)x + a.fg.i01 * (double)y) + a.fg.i02;
        sy = (a.fg.i10 * (double)x + a.fg.i11 * (double)y) + a.fg.i12;
        // the gt: nearest, half to even
        const int xi = (int)rint(sx), yi = (int)rint(sy);
        if (xi >= 0 && xi < W && yi >= 0 && yi < H) g = gt_lut[mask[(int64_t)yi * W + (flip ? W - 1 - xi : xi)]];
        // alpha: four taps of `mask != 0`
        const double fx = floor(sx), fy = floor(sy);
        const int bx = (int)fx, by = (int)fy;
        const float rx = (float)(sx - fx), ry = (float)(sy - fy);
        const float wx[2] = {1.0f - rx, rx}, wy[2] = {1.0f - ry, ry};
        int n = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int yy = by + j;
            const bool row_in = yy >= 0 && yy < H;
            const uint8_t *__restrict__ row = mask + (int64_t)min(max(yy, 0), H - 1) * W;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xx = bx + i;
                const int xc = min(max(xx, 0), W - 1);
                const bool on = row_in && xx >= 0 && xx < W && row[flip ? W - 1 - xc : xc] != 0;
                alpha = alpha + (on ? 1.0f : 0.0f) * (wy[j] * wx[i]);
                n += on ? 1 : 0;
            }
        }
        if (n == 4) alpha = 1.0f;
    }
    gt[px] = g;
    float b[3] = {0.0f, 0.0f, 0.0f}, f[3] = {0.0f, 0.0f, 0.0f};
    if (alpha != 1.0f) {
        const double bsx = (a.bg.i00 * (double)x + a.bg.i01 * (double)y) + a.bg.i02;
        const double bsy = (a.bg.i10 * (double)x + a.bg.i11 * (double)y) + a.bg.i12;
        lucid_gather(background, H, W, flip, bsx, bsy, lut, b);
    }
    if (alpha != 0.0f) lucid_gather(frame, H, W, flip, sx, sy, lut, f);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v = b[ch];
        if (alpha == 1.0f) {
            v = f[ch];
        } else if (alpha != 0.0f) {
            v = b[ch] + alpha * (f[ch] - b[ch]);
        }
        image[ch * plane + px] = v * a.gain[ch] + a.bias[ch];
    }
}

// a coordinate is affine in (x, y): bounded over the frame by its values at the four corners
inline int lucid_check_matrix(const char *which, const LucidMatrix &m, int H, int W) {
    FOSVOS_REQUIRE(isfinite(m.i00) && isfinite(m.i01) && isfinite(m.i02) && isfinite(m.i10) && isfinite(m.i11) && isfinite(m.i12),
                   FOSVOS_E_ARG, "lucid_sample: non-finite coefficient in the %s matrix [[%g, %g, %g], [%g, %g, %g]]", which,
                   m.i00, m.i01, m.i02, m.i10, m.i11, m.i12);
    for (int c = 0; c < 4; ++c) {
        const double x = (c & 1) ? W - 1 : 0, y = (c & 2) ? H - 1 : 0;
        const double sx = (m.i00 * x + m.i01 * y) + m.i02, sy = (m.i10 * x + m.i11 * y) + m.i12;
        FOSVOS_REQUIRE(fabs(sx) <= kLucidMaxCoord && fabs(sy) <= kLucidMaxCoord, FOSVOS_E_ARG,
                       "lucid_sample: output corner (%d, %d) maps to source (%g, %g) under the %s matrix, beyond +-2^30", (int)x,
                       (int)y, sx, sy, which);
    }
    return FOSVOS_OK;
}
}  // namespace

extern "C" int fosvos_lucid_sample(const uint8_t *frame, const uint8_t *background, const uint8_t *mask, int H, int W, int flip,
                                   double b00, double b01, double b02, double b10, double b11, double b12, double f00,
                                   double f01, double f02, double f10, double f11, double f12, int fg_on, float gain0,
                                   float gain1, float gain2, float bias0, float bias1, float bias2, const float *img_lut,
                                   const float *gt_lut, float *image, float *gt, int device, void *stream) {
    FOSVOS_REQUIRE(frame && background && mask && img_lut && gt_lut && image && gt, FOSVOS_E_ARG, "lucid_sample: null pointer");
    FOSVOS_REQUIRE(H > 0 && W > 0 && H <= kLucidMaxSide && W <= kLucidMaxSide, FOSVOS_E_SHAPE,
                   "lucid_sample: H=%d W=%d (1 <= H, W <= %d)", H, W, kLucidMaxSide);
    LucidArgs a = {{b00, b01, b02, b10, b11, b12}, {f00, f01, f02, f10, f11, f12}, {gain0, gain1, gain2}, {bias0, bias1, bias2}};
    if (!fg_on) a.fg = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};  // not read
    int rc = lucid_check_matrix("background", a.bg, H, W);
    if (rc != FOSVOS_OK) return rc;
    rc = lucid_check_matrix("object", a.fg, H, W);
    if (rc != FOSVOS_OK) return rc;
    FOSVOS_REQUIRE(isfinite(gain0) && isfinite(gain1) && isfinite(gain2) && isfinite(bias0) && isfinite(bias1) && isfinite(bias2),
                   FOSVOS_E_ARG, "lucid_sample: non-finite gain or bias: gains (%g, %g, %g), biases (%g, %g, %g)", gain0, gain1,
                   gain2, bias0, bias1, bias2);
    FOSVOS_ENTER(device);
    const dim3 grid((unsigned)cdiv(W, kLucidTileW), (unsigned)cdiv(H, kLucidTileH)), block(kLucidTileW, kLucidTileH);
    FOSVOS_PROF("k_lucid", stream, 0.0);
    hipLaunchKernelGGL(k_lucid, grid, block, 0, (hipStream_t)stream, frame, background, mask, H, W, flip ? 1 : 0, fg_on ? 1 : 0, a,
                       img_lut, gt_lut, image, gt);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
