// Training-sample augmentation on the device: one resident uint8 DAVIS sample -> the [1,3,oh,ow] image and [1,1,oh,ow] gt
// the reference's training pipeline yields for it (src/util/io_helper.py:62-70: RandomHorizontalFlip, Resize, ToTensor
// behind DAVIS2016.make_img_gt_pair), bit for bit the numpy restatement in dataloaders/custom_transforms.py.
//
// The host builds every table (custom_transforms.resize_plan): per output column and per output row the four clipped
// source indices and four fp32 weights of cv2's bicubic kernel, plus the nearest-neighbour indices of the mask.  The value
// conversions are lookup tables too (u8 - mean per channel, u8 / max(label) per frame), so the only arithmetic here is the
// resampling's own: per output value ((((0 + a0*w0) + a1*w1) + a2*w2) + a3*w3) in fp32, every product rounded before its
// add (numpy's `out += a[idx] * w`), the horizontal pass in fp32 first and the vertical pass over its results second.
//
// Memory-bound (a 480x854 sample: 1.6 MB in, 6.6 MB out).  A block owns one output row: it stages the four source rows its
// vertical taps name in LDS with 16-byte loads (the frame's rows are 3*W bytes, not 16-byte aligned: each row keeps its
// global misalignment in LDS so that the aligned middle moves as whole vectors), and its threads walk the row's output
// columns, so every output plane is written with coalesced stores.
#include "common.hpp"

// numpy rounds every product before the add: no multiply-add contraction anywhere in this file
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kAugThreads = 256;
constexpr int kAugMaxW = 4096;  // four staged rows of 3*W bytes + the 3 KB value table stay under 64 KB of LDS

__host__ __device__ inline int aug_row_stride(int W) { return (3 * W + 15 + 15) / 16 * 16; }

__device__ __forceinline__ int clamp_idx(int v, int hi) { return min(max(v, 0), hi); }

// lds[mis + j] = src[j] for j < len, mis = src % 16 (lds is 16-byte aligned)
__device__ __forceinline__ void stage_row(const uint8_t *__restrict__ src, int len, uint8_t *__restrict__ lds) {
    const int mis = (int)((uintptr_t)src & 15);
    const int head = min((16 - mis) & 15, len);
    const int nvec = (len - head) >> 4;
    for (int i = threadIdx.x; i < head; i += kAugThreads) lds[mis + i] = src[i];
    const uint4 *__restrict__ v = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d = reinterpret_cast<uint4 *>(lds + mis + head);  // mis + head is 0 or 16
    for (int i = threadIdx.x; i < nvec; i += kAugThreads) d[i] = v[i];
    for (int i = head + (nvec << 4) + threadIdx.x; i < len; i += kAugThreads) lds[mis + i] = src[i];
}

// grid (1, OH): block y = output row y.  col_taps == nullptr: plain copy (scale 1, OH == H, OW == W).
__global__ __launch_bounds__(kAugThreads) void k_augment(
    const uint8_t *__restrict__ frame, const uint8_t *__restrict__ mask, int H, int W, int flip,
    const int4 *__restrict__ col_taps, const float4 *__restrict__ col_w, const int32_t *__restrict__ row_taps,
    const float *__restrict__ row_w, const int32_t *__restrict__ col_near, const int32_t *__restrict__ row_near, int OH,
    int OW, const float *__restrict__ img_lut, const float *__restrict__ gt_lut, float *__restrict__ image,
    float *__restrict__ gt) {
    extern __shared__ __align__(16) uint8_t aug_smem[];
    float *lut = reinterpret_cast<float *>(aug_smem);  // [256][3]: u8 - mean of each channel
    uint8_t *rows = aug_smem + 256 * 3 * sizeof(float);
    const int row_stride = aug_row_stride(W);
    const int y = blockIdx.y, len = 3 * W;
    const bool cubic = col_taps != nullptr;
    for (int i = threadIdx.x; i < 256 * 3; i += kAugThreads) lut[i] = img_lut[i];
    int mis[4];
    float wy[4];
    if (cubic) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t *src = frame + (int64_t)clamp_idx(row_taps[y * 4 + k], H - 1) * len;
            mis[k] = (int)((uintptr_t)src & 15);
            wy[k] = row_w[y * 4 + k];
            stage_row(src, len, rows + k * row_stride);
        }
    } else {
        const uint8_t *src = frame + (int64_t)y * len;
        mis[0] = (int)((uintptr_t)src & 15);
        stage_row(src, len, rows);
    }
    __syncthreads();
    const int64_t plane = (int64_t)OH * OW, out_row = (int64_t)y * OW;
    const uint8_t *__restrict__ mrow = mask + (int64_t)(cubic ? clamp_idx(row_near[y], H - 1) : y) * W;
    for (int x = threadIdx.x; x < OW; x += kAugThreads) {
        int nx;
        if (cubic) {
            const int4 ti = col_taps[x];
            const float4 tw = col_w[x];
            int c[4] = {ti.x, ti.y, ti.z, ti.w};
            const float wx[4] = {tw.x, tw.y, tw.z, tw.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = clamp_idx(c[j], W - 1);
                c[j] = 3 * (flip ? W - 1 - c[j] : c[j]);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint8_t *rk = rows + k * row_stride + mis[k] + ch;
                    float h = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) h = h + lut[rk[c[j]] * 3 + ch] * wx[j];
                    acc = acc + h * wy[k];
                }
                image[ch * plane + out_row + x] = acc;
            }
            nx = clamp_idx(col_near[x], W - 1);
        } else {
            const uint8_t *px = rows + mis[0] + 3 * (flip ? W - 1 - x : x);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) image[ch * plane + out_row + x] = lut[px[ch] * 3 + ch];
            nx = x;
        }
        gt[out_row + x] = gt_lut[mrow[flip ? W - 1 - nx : nx]];
    }
}
}  // namespace

extern "C" int fosvos_augment_sample(const uint8_t *frame, const uint8_t *mask, int H, int W, int flip,
                                     const int32_t *col_taps, const float *col_w, const int32_t *row_taps,
                                     const float *row_w, const int32_t *col_near, const int32_t *row_near, int OH, int OW,
                                     const float *img_lut, const float *gt_lut, float *image, float *gt, int device,
                                     void *stream) {
    FOSVOS_REQUIRE(frame && mask && img_lut && gt_lut && image && gt, FOSVOS_E_ARG, "augment_sample: null pointer");
    FOSVOS_REQUIRE(H > 0 && W > 0 && W <= kAugMaxW && OH > 0 && OH <= 65535 && OW > 0, FOSVOS_E_SHAPE,
                   "augment_sample: H=%d W=%d (W <= %d) -> OH=%d OW=%d", H, W, kAugMaxW, OH, OW);
    const int n_tables = (col_taps != nullptr) + (col_w != nullptr) + (row_taps != nullptr) + (row_w != nullptr) +
                         (col_near != nullptr) + (row_near != nullptr);
    FOSVOS_REQUIRE(n_tables == 0 || n_tables == 6, FOSVOS_E_ARG,
                   "augment_sample: give all six resampling tables, or none for a plain copy (%d given)", n_tables);
    FOSVOS_REQUIRE(n_tables == 6 || (OH == H && OW == W), FOSVOS_E_SHAPE,
                   "augment_sample: a copy keeps the size (%dx%d -> %dx%d)", H, W, OH, OW);
    FOSVOS_REQUIRE((((uintptr_t)col_taps | (uintptr_t)col_w) & 15) == 0, FOSVOS_E_ARG,
                   "augment_sample: the column tables must be 16-byte aligned");
    FOSVOS_ENTER(device);
    const size_t lds = 256 * 3 * sizeof(float) + 4 * (size_t)aug_row_stride(W);
    FOSVOS_PROF("k_augment", stream, 0.0);
    hipLaunchKernelGGL(k_augment, dim3(1, (unsigned)OH), dim3(kAugThreads), lds, (hipStream_t)stream, frame, mask, H, W,
                       flip ? 1 : 0, reinterpret_cast<const int4 *>(col_taps), reinterpret_cast<const float4 *>(col_w),
                       row_taps, row_w, col_near, row_near, OH, OW, img_lut, gt_lut, image, gt);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
