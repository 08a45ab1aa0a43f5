// Measuring how the picture moved between two frames and moving a mask along with it (opt-in): full-search block matching on
// the frames' luma and a per-block warp.  util/block_motion.py states the arithmetic in numpy - all of it in integers - and
// every output here is compared with it bit for bit.
//
// fosvos_motion_luma: k_motion_luma, one thread a pixel: the frame's bytes taken back from the net's input as crf.hip takes
//   them (t = (f64(v) + f64(mean[c])) + 0.5, clamped to 0..255, a NaN is 0), Y = (29 g0 + 150 g1 + 77 g2 + 128) >> 8.
// fosvos_motion_warp: k_motion_warp, one thread a pixel: out = mask[y + dy, x + dx] != 0 with the block's (dy, dx); the source
//   index is tested against the frame BEFORE the read, so no field can reach outside the mask.
// fosvos_motion_estimate: ONE launch of k_motion_estimate<block> for all N pairs.  A workgroup of 256 threads (four waves)
//   owns a TILE of 16 rows x 64 columns of one pair: four blocks of 16 or sixteen of 8.  (480 x 854 gives 420 workgroups a
//   pair; a 32 x 64 tile would leave a single pair with fewer workgroups than the chip has CUs.)
//   stage    the current tile (16 x 64 bytes, 1 KB) and the previous frame's tile with a halo of `search` rows above and below
//            and of `search` rounded up to a multiple of 4 columns left and right - up to 48 x 96 bytes, 4.7 KB - as packed
//            words: thread t makes words t, t + 256, ... from four byte loads (a row of a byte plane starts at any address)
//            and ONE word store; a byte outside the frame is staged as 0 without a read.
//   match    wave v takes blocks v, v + 4, ... of the tile.  It holds the block's current pixels in registers (block * block / 4
//            words, the same in every lane: LDS broadcasts), and its lanes share out the candidates: lane l takes candidates
//            l, l + 64, ... of the (2 search + 1)^2 in raster order (dy outside, dx inside), so neighbouring lanes read
//            neighbouring bytes of one staged row.  A candidate that would take the block outside the frame is skipped, not
//            clamped.  Per row of the block a lane reads block / 4 + 1 staged words, takes the block / 4 words that start at
//            its byte with v_alignbyte_b32 and sums |cur - prev| four bytes an instruction with v_sad_u8.  In a ragged block
//            the rows below the frame are not visited and the bytes right of it are masked out of both operands.
//   winner   a lane keeps the smallest key (score << 22 | (dy^2 + dx^2) << 12 | (dy + 16) << 6 | (dx + 16)) of its
//            candidates as one 64-bit integer; six wave shuffles take the block's minimum; lane 0 writes the field and the
//            unbiased SAD.  One wave owns a block's every candidate, so there is nothing to combine across waves.
//   No atomics, no global scratch, no workgroup waits for another.
#include <math.h>

#include "common.hpp"

using namespace fosvos;

namespace {
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTileH = 16, kTileW = 64;
constexpr int kMaxSearch = 16, kMaxZeroBias = 255;
constexpr int kMaxSide = 8192;
constexpr int kCurWords = kTileW / 4;                            // 16 words a row of the current tile
constexpr int kPrevRows = kTileH + 2 * kMaxSearch;               // 48
constexpr int kPrevWords = (kTileW + 2 * kMaxSearch) / 4;        // 24 words a staged row at the widest halo
constexpr int kPrevStride = kPrevWords + 1;                      // ... and one more: the word behind an aligned read
constexpr int kKeyDyShift = 6, kKeyD2Shift = 12, kKeyScoreShift = 22;

struct MotionGeom {
    int H, W;
    int tiles_x, tiles_y;
    int search, halo_x;  // halo_x: search rounded up to a multiple of 4
    int zero_bias;
    int Hb, Wb;
};
struct Lds {
    uint32_t cur[kTileH * kCurWords];
    uint32_t prev[kPrevRows * kPrevStride + 3];
};

__device__ __forceinline__ uint32_t level(float v, double mean) {
    const double t = ((double)v + mean) + 0.5;
    return t >= 0.0 ? (t < 256.0 ? (uint32_t)(int)floor(t) : 255u) : 0u;  // a NaN compares false: 0
}

__global__ __launch_bounds__(kThreads) void k_motion_luma(const float *__restrict__ image, uint8_t *__restrict__ out,
                                                         int64_t plane, int64_t total, double m0, double m1, double m2) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t n = i / plane, px = i - n * plane;
    const float *__restrict__ im = image + n * 3 * plane + px;
    const uint32_t y = 29u * level(im[0], m0) + 150u * level(im[plane], m1) + 77u * level(im[2 * plane], m2) + 128u;
    out[i] = (uint8_t)(y >> 8);
}

__global__ __launch_bounds__(kThreads) void k_motion_warp(const uint8_t *__restrict__ mask, const int8_t *__restrict__ field,
                                                         uint8_t *__restrict__ out, int H, int W, int block, int Hb, int Wb,
                                                         int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t plane = (int64_t)H * W;
    const int64_t n = i / plane, px = i - n * plane;
    const int y = (int)(px / W), x = (int)(px - (int64_t)y * W);
    const int8_t *__restrict__ d = field + ((n * Hb + y / block) * Wb + x / block) * 2;
    const int sy = y + (int)d[0], sx = x + (int)d[1];  // |d| <= 128 and y, x < 8192: no overflow
    uint8_t v = 0;
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = mask[n * plane + (int64_t)sy * W + sx] != 0;
    out[i] = v;
}

// one staged word: the four bytes (y, x .. x + 3) of a byte plane, 0 outside the frame
__device__ __forceinline__ uint32_t stage_word(const uint8_t *__restrict__ plane, int y, int x, int H, int W) {
    if (y < 0 || y >= H) return 0u;
    const uint8_t *__restrict__ row = plane + (int64_t)y * W;
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (x + b >= 0 && x + b < W) w |= (uint32_t)row[x + b] << (8 * b);
    return w;
}

// SAD of one candidate over the block's rows.  kMask: the block is narrower than B (its right part lies outside the frame).
template <int B, bool kMask>
__device__ __forceinline__ uint32_t block_sad(const uint32_t (&cur)[B][B / 4], const uint32_t *__restrict__ prow, int shift,
                                              int rows, const uint32_t (&mask)[B / 4]) {
    uint32_t sad = 0;
#pragma unroll
    for (int r = 0; r < B; ++r) {
        if (r < rows) {
            uint32_t w[B / 4 + 1];
#pragma unroll
            for (int k = 0; k <= B / 4; ++k) w[k] = prow[r * kPrevStride + k];
#pragma unroll
            for (int k = 0; k < B / 4; ++k) {
                uint32_t p = __builtin_amdgcn_alignbyte(w[k + 1], w[k], (uint32_t)shift);
                if (kMask) p &= mask[k];
                sad = __builtin_amdgcn_sad_u8(cur[r][k], p, sad);
            }
        }
    }
    return sad;
}

template <int B>
__global__ __launch_bounds__(kThreads) void k_motion_estimate(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ cur,
                                                             int8_t *__restrict__ field, int32_t *__restrict__ cost,
                                                             MotionGeom g) {
    __shared__ Lds lds;
    const int x0 = (int)(blockIdx.x % g.tiles_x) * kTileW;
    const int y0 = (int)((blockIdx.x / g.tiles_x) % g.tiles_y) * kTileH;
    const int64_t n = blockIdx.x / ((unsigned)g.tiles_x * g.tiles_y);
    const int64_t plane = (int64_t)g.H * g.W;
    const uint8_t *__restrict__ pv = prev + n * plane;
    const uint8_t *__restrict__ cu = cur + n * plane;
    const int s = g.search, hx = g.halo_x;

    for (int idx = threadIdx.x; idx < kTileH * kCurWords; idx += kThreads) {
        const int sy = idx / kCurWords, sw = idx - sy * kCurWords;
        lds.cur[idx] = stage_word(cu, y0 + sy, x0 + 4 * sw, g.H, g.W);
    }
    const int prow_words = (kTileW + 2 * hx) / 4, prows = kTileH + 2 * s;
    for (int idx = threadIdx.x; idx < prows * prow_words; idx += kThreads) {
        const int sy = idx / prow_words, sw = idx - sy * prow_words;
        lds.prev[sy * kPrevStride + sw] = stage_word(pv, y0 - s + sy, x0 - hx + 4 * sw, g.H, g.W);
    }
    // the word behind each staged row (read, never used, by a candidate whose bytes start at a word) and the tail
    for (int idx = threadIdx.x; idx < prows; idx += kThreads) lds.prev[idx * kPrevStride + prow_words] = 0u;
    __syncthreads();

    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    constexpr int kBlocksX = kTileW / B, kBlocks = (kTileH / B) * kBlocksX;
    const int side = 2 * s + 1, ncand = side * side;
    for (int b = wave; b < kBlocks; b += kWaves) {
        const int ly = (b / kBlocksX) * B, lx = (b % kBlocksX) * B;  // the block's corner in the tile
        const int by0 = y0 + ly, bx0 = x0 + lx;
        if (by0 >= g.H || bx0 >= g.W) continue;  // the same in every lane of the wave
        const int rows = min(B, g.H - by0), cols = min(B, g.W - bx0);
        const int by1 = by0 + rows, bx1 = bx0 + cols;
        uint32_t c[B][B / 4], mask[B / 4];
#pragma unroll
        for (int k = 0; k < B / 4; ++k) {
            const int left = cols - 4 * k;  // the word's bytes inside the frame
            mask[k] = left >= 4 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
        }
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int k = 0; k < B / 4; ++k) c[r][k] = lds.cur[(ly + r) * kCurWords + lx / 4 + k];  // 0 outside the frame
        const uint32_t bias = ((uint32_t)g.zero_bias * (uint32_t)(rows * cols)) >> 4;
        uint64_t best = ~(uint64_t)0;
        for (int cand = lane; cand < ncand; cand += 64) {
            const int dy = cand / side - s, dx = cand - (cand / side) * side - s;
            if (by0 + dy < 0 || by1 + dy > g.H || bx0 + dx < 0 || bx1 + dx > g.W) continue;  // skipped, not clamped
            const int xb = lx + hx + dx;  // the candidate's first byte in a staged row: 0 <= xb, xb + B <= 64 + 2 hx
            const uint32_t *__restrict__ prow = lds.prev + (ly + s + dy) * kPrevStride + (xb >> 2);
            const uint32_t sad = cols == B ? block_sad<B, false>(c, prow, xb & 3, rows, mask)
                                           : block_sad<B, true>(c, prow, xb & 3, rows, mask);
            const uint32_t score = sad + ((dy | dx) != 0 ? bias : 0u);
            const uint64_t key = ((uint64_t)score << kKeyScoreShift) | ((uint64_t)(dy * dy + dx * dx) << kKeyD2Shift) |
                                 ((uint64_t)(dy + kMaxSearch) << kKeyDyShift) | (uint64_t)(dx + kMaxSearch);
            best = key < best ? key : best;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint64_t other = __shfl_xor((unsigned long long)best, off, 64);
            best = other < best ? other : best;
        }
        if (lane == 0) {  // (0, 0) is always a candidate: best is a key
            const int dy = (int)((best >> kKeyDyShift) & 63u) - kMaxSearch, dx = (int)(best & 63u) - kMaxSearch;
            const uint32_t score = (uint32_t)(best >> kKeyScoreShift);
            const int64_t at = (n * g.Hb + by0 / B) * g.Wb + bx0 / B;
            field[2 * at] = (int8_t)dy;
            field[2 * at + 1] = (int8_t)dx;
            cost[at] = (int32_t)(score - ((dy | dx) != 0 ? bias : 0u));
        }
    }
}
}  // namespace

extern "C" int fosvos_motion_luma(const float *image, const float mean[3], int N, int H, int W, uint8_t *out, int device,
                                  void *stream) {
    FOSVOS_REQUIRE(image && mean && out, FOSVOS_E_ARG, "motion_luma: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, FOSVOS_E_SHAPE,
                   "motion_luma: N=%d, frames of %dx%d (sides of 1..%d)", N, H, W, kMaxSide);
    FOSVOS_REQUIRE(((uintptr_t)image & 3) == 0, FOSVOS_E_ARG, "motion_luma: the image must be 4-byte aligned");
    const int64_t plane = (int64_t)H * W, total = (int64_t)N * plane;
    const int64_t blocks = cdiv(total, kThreads);
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "motion_luma: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    FOSVOS_PROF("k_motion_luma", stream, 8.0 * (double)total);
    hipLaunchKernelGGL(k_motion_luma, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, image, out, plane, total,
                       (double)mean[0], (double)mean[1], (double)mean[2]);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_motion_estimate(const uint8_t *prev, const uint8_t *cur, int N, int H, int W, int block, int search,
                                      int zero_bias, int8_t *field, int32_t *cost, int device, void *stream) {
    FOSVOS_REQUIRE(prev && cur && field && cost, FOSVOS_E_ARG, "motion_estimate: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, FOSVOS_E_SHAPE,
                   "motion_estimate: N=%d, planes of %dx%d (sides of 1..%d)", N, H, W, kMaxSide);
    FOSVOS_REQUIRE(block == 8 || block == 16, FOSVOS_E_ARG, "motion_estimate: block %d is neither 8 nor 16", block);
    FOSVOS_REQUIRE(search >= 1 && search <= kMaxSearch, FOSVOS_E_ARG, "motion_estimate: search %d outside [1, %d]", search,
                   kMaxSearch);
    FOSVOS_REQUIRE(zero_bias >= 0 && zero_bias <= kMaxZeroBias, FOSVOS_E_ARG, "motion_estimate: zero_bias %d outside [0, %d]",
                   zero_bias, kMaxZeroBias);
    FOSVOS_REQUIRE(((uintptr_t)cost & 3) == 0, FOSVOS_E_ARG, "motion_estimate: cost must be 4-byte aligned");
    MotionGeom g = {H, W, (int)cdiv(W, kTileW), (int)cdiv(H, kTileH), search, roundup(search, 4), zero_bias,
                    (int)cdiv(H, block), (int)cdiv(W, block)};
    const int64_t blocks = (int64_t)N * g.tiles_x * g.tiles_y;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "motion_estimate: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    const double cands = (2.0 * search + 1) * (2.0 * search + 1);
    FOSVOS_PROF("k_motion_estimate", stream, 2.0 * cands * (double)N * H * W);
    if (block == 8)
        hipLaunchKernelGGL(k_motion_estimate<8>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, prev, cur, field,
                           cost, g);
    else
        hipLaunchKernelGGL(k_motion_estimate<16>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, prev, cur,
                           field, cost, g);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_motion_warp(const uint8_t *mask, const int8_t *field, int N, int H, int W, int block, uint8_t *out,
                                  int device, void *stream) {
    FOSVOS_REQUIRE(mask && field && out, FOSVOS_E_ARG, "motion_warp: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, FOSVOS_E_SHAPE,
                   "motion_warp: N=%d, masks of %dx%d (sides of 1..%d)", N, H, W, kMaxSide);
    FOSVOS_REQUIRE(block == 8 || block == 16, FOSVOS_E_ARG, "motion_warp: block %d is neither 8 nor 16", block);
    const int64_t total = (int64_t)N * H * W;
    // a gather: an output pixel of one thread is another thread's source
    FOSVOS_REQUIRE(out + total <= mask || mask + total <= out, FOSVOS_E_ARG, "motion_warp: out must not overlap the mask");
    const int64_t blocks = cdiv(total, kThreads);
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "motion_warp: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    FOSVOS_PROF("k_motion_warp", stream, 0.0);
    hipLaunchKernelGGL(k_motion_warp, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, mask, field, out, H, W, block,
                       (int)cdiv(H, block), (int)cdiv(W, block), total);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
