// Rotation and zoom of the training sample on the device: one resident uint8 DAVIS sample -> the [1,3,H,W] image and
// [1,1,H,W] gt that RandomHorizontalFlip + ScaleNRotate + ToTensor yield for it, bit for bit the numpy restatement in
// dataloaders/custom_transforms.py (warp_affine: cv2.warpAffine with constant-0 borders, bicubic for the frame, nearest for
// the mask).
//
// The host inverts the 2x3 matrix (np.linalg.inv in fp64) and passes the six doubles of destination -> source by value.
// Per output pixel (x, y): sx = (i00*x + i01*y) + i02 and sy likewise in fp64; the mask takes rint of both (half to even)
// and the lookup-table value of the byte there, 0 outside; the frame takes floor of both, the two fractions as fp32,
// interpolateCubic's weights (A = -0.75) in fp32 in numpy's order of operations, and the 16 taps row-outer / column-inner as
// out = out + val * (wy[j] * wx[i]) from +0.0, every product rounded before its add, val = 0 for a tap outside the source.
// flip mirrors the source first: source column x is frame column W-1-x.  Every tap's address is clamped into the frame before
// the load, so no matrix makes the kernel read outside its operands.
//
// A workgroup of 256 threads owns a tile of 64 x 4 output pixels, one thread a pixel: plain gathers of the (L2-resident)
// frame through the value table in LDS, and one coalesced 256-byte store per wave and plane.
//
// renormalize (the reference's ScaleNRotate: `if min < 0: tmp -= min`, `if max > 1: tmp /= max`): the warp launch also
// writes the (min, max) of its tile's image values to the workspace, one pair per workgroup, and a second launch has every
// workgroup reduce ALL pairs (min and max: no order to agree on, no atomics, nobody waits for anybody) and rewrite its share
// of the image.  The max of the shifted array is fl(mx - mn) (rounding is monotone), so the second pass needs no third.
#include <math.h>

#include "common.hpp"

// numpy rounds every product before the add: no multiply-add contraction anywhere in this file
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kWarpTileW = 64, kWarpTileH = 4, kWarpThreads = kWarpTileW * kWarpTileH;
constexpr int kWarpMaxSide = 8192;            // fosvos_hip/limits.py: MAX_FRAME_SIDE
constexpr double kWarpMaxCoord = 1073741824.0;  // 2^30: floor / rint of a source coordinate, and the taps' +-2, fit int32
constexpr int kRenormThreads = 256, kRenormMaxBlocks = 1024;

struct WarpMatrix {
    double i00, i01, i02, i10, i11, i12;  // destination -> source
};

// custom_transforms._cubic_weights on one fraction, fp32, in numpy's order of operations (a = -0.75)
__device__ __forceinline__ void cubic_weights(float x, float (&w)[4]) {
    const float a = -0.75f;
    const float t = x + 1.0f;
    w[0] = ((a * t - 5.0f * a) * t + 8.0f * a) * t - 4.0f * a;
    w[1] = ((a + 2.0f) * x - (a + 3.0f)) * x * x + 1.0f;
    const float u = 1.0f - x;
    w[2] = ((a + 2.0f) * u - (a + 3.0f)) * u * u + 1.0f;
    w[3] = 1.0f - w[0] - w[1] - w[2];
}

// (min, max) over the workgroup's 256 threads; `wave`: 8 floats of LDS.  Every thread returns the result.
__device__ __forceinline__ void block_minmax(float &mn, float &mx, float *wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if ((tid & 63) == 0) {
        wave[(tid >> 6) * 2] = mn;
        wave[(tid >> 6) * 2 + 1] = mx;
    }
    __syncthreads();
    mn = fminf(fminf(wave[0], wave[2]), fminf(wave[4], wave[6]));
    mx = fmaxf(fmaxf(wave[1], wave[3]), fmaxf(wave[5], wave[7]));
}

// grid (ceil(W / 64), ceil(H / 4)), block (64, 4).  kPairs: also write this tile's (min, max) to pairs[2 * block].
template <bool kPairs>
__global__ __launch_bounds__(kWarpThreads) void k_warp(const uint8_t *__restrict__ frame, const uint8_t *__restrict__ mask,
                                                       int H, int W, int flip, WarpMatrix m,
                                                       const float *__restrict__ img_lut, const float *__restrict__ gt_lut,
                                                       float *__restrict__ image, float *__restrict__ gt,
                                                       float *__restrict__ pairs) {
    __shared__ float lut[256 * 3];  // [256][3]: u8 - mean of each channel
    __shared__ float wave[8];
    const int tid = threadIdx.y * kWarpTileW + threadIdx.x;
    for (int i = tid; i < 256 * 3; i += kWarpThreads) lut[i] = img_lut[i];
    __syncthreads();
    const int x = blockIdx.x * kWarpTileW + threadIdx.x, y = blockIdx.y * kWarpTileH + threadIdx.y;
    const bool live = x < W && y < H;
    float mn = INFINITY, mx = -INFINITY;
    if (live) {
        const double sx = (m.i00 * (double)x + m.i01 * (double)y) + m.i02;
        const double sy = (m.i10 * (double)x + m.i11 * (double)y) + m.i12;
        const int64_t px = (int64_t)y * W + x, plane = (int64_t)H * W;
        // the mask: nearest, half to even
        const int xi = (int)rint(sx), yi = (int)rint(sy);
        float g = 0.0f;
        if (xi >= 0 && xi < W && yi >= 0 && yi < H) g = gt_lut[mask[(int64_t)yi * W + (flip ? W - 1 - xi : xi)]];
        gt[px] = g;
        // the frame: bicubic over the 4 x 4 taps at floor - 1 .. floor + 2
        const double fx = floor(sx), fy = floor(sy);
        const int bx = (int)fx, by = (int)fy;
        float wx[4], wy[4];
        cubic_weights((float)(sx - fx), wx);
        cubic_weights((float)(sy - fy), wy);
        float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = by + j - 1;
            const bool row_in = yy >= 0 && yy < H;
            const uint8_t *__restrict__ row = frame + (int64_t)min(max(yy, 0), H - 1) * W * 3;
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
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            image[ch * plane + px] = acc[ch];
            mn = fminf(mn, acc[ch]);
            mx = fmaxf(mx, acc[ch]);
        }
    }
    if constexpr (kPairs) {
        block_minmax(mn, mx, wave);  // (every tile holds at least one live pixel: the pair is finite)
        if (tid == 0) {
            const int64_t b = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
            pairs[2 * b] = mn;
            pairs[2 * b + 1] = mx;
        }
    }
}

// every workgroup reduces all n_pairs (min, max) pairs, then rewrites its share of the n image values
__global__ __launch_bounds__(kRenormThreads) void k_warp_renorm(float *__restrict__ image, int64_t n,
                                                                const float *__restrict__ pairs, int n_pairs) {
    __shared__ float wave[8];
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < n_pairs; i += kRenormThreads) {
        mn = fminf(mn, pairs[2 * i]);
        mx = fmaxf(mx, pairs[2 * i + 1]);
    }
    block_minmax(mn, mx, wave);
    const bool shift = mn < 0.0f;
    const float mx2 = shift ? mx - mn : mx;
    const bool div = mx2 > 1.0f;
    if (!shift && !div) return;
    for (int64_t i = (int64_t)blockIdx.x * kRenormThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRenormThreads) {
        float v = image[i];
        if (shift) v = v - mn;
        if (div) v = v / mx2;
        image[i] = v;
    }
}

inline int64_t warp_tiles(int H, int W) { return cdiv(W, kWarpTileW) * cdiv(H, kWarpTileH); }
}  // namespace

extern "C" size_t fosvos_warp_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || H > kWarpMaxSide || W > kWarpMaxSide) return 0;
    return (size_t)warp_tiles(H, W) * 2 * sizeof(float);
}

extern "C" int fosvos_warp_sample(const uint8_t *frame, const uint8_t *mask, int H, int W, int flip, double i00, double i01,
                                  double i02, double i10, double i11, double i12, const float *img_lut, const float *gt_lut,
                                  float *image, float *gt, int renormalize, void *workspace, size_t workspace_bytes,
                                  int device, void *stream) {
    FOSVOS_REQUIRE(frame && mask && img_lut && gt_lut && image && gt, FOSVOS_E_ARG, "warp_sample: null pointer");
    FOSVOS_REQUIRE(H > 0 && W > 0 && H <= kWarpMaxSide && W <= kWarpMaxSide, FOSVOS_E_SHAPE,
                   "warp_sample: H=%d W=%d (1 <= H, W <= %d)", H, W, kWarpMaxSide);
    const WarpMatrix m = {i00, i01, i02, i10, i11, i12};
    FOSVOS_REQUIRE(isfinite(i00) && isfinite(i01) && isfinite(i02) && isfinite(i10) && isfinite(i11) && isfinite(i12),
                   FOSVOS_E_ARG, "warp_sample: non-finite coefficient in [[%g, %g, %g], [%g, %g, %g]]", i00, i01, i02, i10,
                   i11, i12);
    // a coordinate is affine in (x, y): bounded over the frame by its values at the four corners
    for (int c = 0; c < 4; ++c) {
        const double x = (c & 1) ? W - 1 : 0, y = (c & 2) ? H - 1 : 0;
        const double sx = (m.i00 * x + m.i01 * y) + m.i02, sy = (m.i10 * x + m.i11 * y) + m.i12;
        FOSVOS_REQUIRE(fabs(sx) <= kWarpMaxCoord && fabs(sy) <= kWarpMaxCoord, FOSVOS_E_ARG,
                       "warp_sample: output corner (%d, %d) maps to source (%g, %g), beyond +-2^30", (int)x, (int)y, sx, sy);
    }
    const size_t need = renormalize ? fosvos_warp_workspace_bytes(H, W) : 0;
    FOSVOS_REQUIRE(!renormalize || (workspace != nullptr && workspace_bytes >= need), FOSVOS_E_WORKSPACE,
                   "warp_sample: renormalize needs a workspace of %zu bytes (fosvos_warp_workspace_bytes), got %zu", need,
                   workspace ? workspace_bytes : (size_t)0);
    FOSVOS_REQUIRE(!renormalize || ((uintptr_t)workspace & 3) == 0, FOSVOS_E_ARG,
                   "warp_sample: the workspace must be 4-byte aligned");
    FOSVOS_ENTER(device);
    const dim3 grid((unsigned)cdiv(W, kWarpTileW), (unsigned)cdiv(H, kWarpTileH)), block(kWarpTileW, kWarpTileH);
    if (!renormalize) {
        FOSVOS_PROF("k_warp", stream, 0.0);
        hipLaunchKernelGGL(k_warp<false>, grid, block, 0, (hipStream_t)stream, frame, mask, H, W, flip ? 1 : 0, m, img_lut,
                           gt_lut, image, gt, (float *)nullptr);
        FOSVOS_LAUNCH_CHECK();
        return FOSVOS_OK;
    }
    FOSVOS_PROF("k_warp_pairs", stream, 0.0);
    hipLaunchKernelGGL(k_warp<true>, grid, block, 0, (hipStream_t)stream, frame, mask, H, W, flip ? 1 : 0, m, img_lut, gt_lut,
                       image, gt, (float *)workspace);
    FOSVOS_LAUNCH_CHECK();
    const int64_t n = 3 * (int64_t)H * W;
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, kRenormThreads * 8), kRenormMaxBlocks);
    FOSVOS_PROF("k_warp_renorm", stream, 0.0);
    hipLaunchKernelGGL(k_warp_renorm, dim3(blocks), dim3(kRenormThreads), 0, (hipStream_t)stream, image, n,
                       (const float *)workspace, (int)warp_tiles(H, W));
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
