// Scoring a segmented sequence on the device: the PNG bytes of the probability map and the integer counts behind the two
// DAVIS 2016 measures, region similarity J (mask IoU) and contour accuracy F (boundary F-measure).  The reference has no
// evaluation code (src/eval/README.md points at an outside toolkit); the definitions are the ones util/davis_measures.py
// states in numpy, and the byte stretch is util/experiment_helper.bytescale in fp64.
//
// fosvos_prob_bytes, three launches:
//   k_minmax_init  the frame's {min, max} record <- {+inf, -inf}
//   k_minmax       one pass over the logits: per-workgroup min / max, one pair of integer atomics each (a float orders like
//                  its bits read as a signed integer when the sign is clear and like MINUS its bits read as an unsigned
//                  one when it is set, so the record holds real floats all along; min / max are order-free)
//   k_prob_map     one pass: p = 1 / (1 + exp(-x)) in fp64, stretched to the frame's own [p(min), p(max)], rounded half up
// Memory-bound: 4 B read twice and 1 B written per pixel.
//
// fosvos_jf_counts, two launches, all integer:
//   k_jf_pack      a wave reads 64 consecutive logits (one 256-B line) and 64 ground-truth bytes; __ballot(x >= 0) and
//                  __ballot(gt != 0) ARE the two 64-pixel words of the bit planes A and B ([N][H][ceil(W/64)] uint64 each, bit
//                  i of word c = pixel 64c+i, bits past column W-1 zero).  Its first 6N threads zero the counters.
//   k_jf_count     a workgroup owns a tile of 16 rows x 8 words (512 pixels).  It builds the boundary maps of A and B for the
//                  tile and its halo (r rows above and below, one word left and right: r <= 63 keeps the disk's reach inside
//                  the neighbouring word) in LDS from the planes (XORs of a word with itself shifted by one bit, carrying
//                  the neighbour word's edge bit, and with the row below), then every thread dilates ONE word of both maps:
//                  the disk is a union of horizontal spans, one per dy in [-r, r] of half-width floor(sqrt(r*r - dy*dy)), so
//                  the dilation is an OR over 2r+1 rows of the row's word spread left and right by that half-width
//                  (doubling shift-ORs on the 128-bit pair {neighbour, word}).  Counts are popcounts of ANDed words, summed
//                  over the wave, the workgroup and - with integer atomics, so in any order - the frame.
// After the pack pass everything works on data 32 times smaller than the logits (a 480x854 plane is 53 KB), which stays in L2;
// LDS per workgroup: 2 * (16 + 2r) * 10 words + the span table = 5.6 KB at r = 8, 23.2 KB at r = 63.
//
// Several objects a sequence (util/object_merge.py states both in numpy):
// fosvos_merge_objects, one launch:
//   k_merge_objects   the K logit maps of the K per-object nets (pointers by value in the kernel's arguments) -> one label
//                     byte a pixel: 0 where no logit is >= 0, else 1 + the lowest k holding the largest such logit.  A thread
//                     takes 4 consecutive pixels (K float4 loads, one dword store) where size and alignment allow, else 1.
//                     Memory-bound: 4K B read and 1 B written per pixel.
// fosvos_jf_counts_labels, two launches:
//   k_jf_pack_labels  a wave reads 64 predicted and 64 ground-truth label bytes; for k = 1..K __ballot(pred == k) and
//                     __ballot(gt == k) are the words of object k's planes, laid out [N][K][H][Wp]: to k_jf_count, which runs
//                     unchanged, these are N * K frames.  Its threads zero the 6 N K counters.
#include "common.hpp"

// the fp64 expressions are the host's, operation for operation
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
typedef unsigned long long u64;

constexpr int kEvalThreads = 256;
constexpr int kMaxRadius = 63;

// ------------------------------------------------------------------------------------------ prob_bytes
__global__ void k_minmax_init(float *__restrict__ minmax, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        minmax[2 * i] = __int_as_float(0x7f800000);
        minmax[2 * i + 1] = __int_as_float((int)0xff800000u);
    }
}

__device__ __forceinline__ void atomic_min_f32(float *p, float v) {
    if (__float_as_int(v) >= 0) atomicMin(reinterpret_cast<int *>(p), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned *>(p), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float *p, float v) {
    if (__float_as_int(v) >= 0) atomicMax(reinterpret_cast<int *>(p), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned *>(p), __float_as_uint(v));
}

// grid (blocks, N).  vec: the frames are 16-byte aligned and hw % 4 == 0
__global__ __launch_bounds__(kEvalThreads) void k_minmax(const float *__restrict__ x, int64_t hw, int vec,
                                                         float *__restrict__ minmax) {
    x += (int64_t)blockIdx.y * hw;
    float lo = __int_as_float(0x7f800000), hi = -lo;
    const int64_t t = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x, nt = (int64_t)gridDim.x * kEvalThreads;
    if (vec) {
        const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
        for (int64_t i = t; i < (hw >> 2); i += nt) {
            const float4 v = x4[i];
            lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
            hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
        }
    } else {
        for (int64_t i = t; i < hw; i += nt) {
            lo = fminf(lo, x[i]);
            hi = fmaxf(hi, x[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    // (a thread that saw no pixel still holds +-inf, which changes nothing)
    __shared__ float s_lo[kEvalThreads / 64], s_hi[kEvalThreads / 64];
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // one pair of atomics per workgroup: they all meet on one address
        atomic_min_f32(minmax + 2 * blockIdx.y, fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3])));
        atomic_max_f32(minmax + 2 * blockIdx.y + 1, fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3])));
    }
}

__device__ __forceinline__ unsigned prob_byte(float x, double cmin, double k) {
    const double scaled = (sigmoid_f64(x) - cmin) * k;
    return (unsigned)(fmin(fmax(scaled, 0.0), 255.0) + 0.5);
}

__global__ __launch_bounds__(kEvalThreads) void k_prob_map(const float *__restrict__ x, int64_t hw, int vec,
                                                           const float *__restrict__ minmax, uint8_t *__restrict__ out) {
    x += (int64_t)blockIdx.y * hw;
    out += (int64_t)blockIdx.y * hw;
    const double cmin = sigmoid_f64(minmax[2 * blockIdx.y]), cmax = sigmoid_f64(minmax[2 * blockIdx.y + 1]);
    double cscale = cmax - cmin;
    if (cscale == 0.0) cscale = 1.0;
    const double k = 255.0 / cscale;
    const int64_t t = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x, nt = (int64_t)gridDim.x * kEvalThreads;
    if (vec) {
        const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(x);
        uint32_t *__restrict__ o4 = reinterpret_cast<uint32_t *>(out);
        for (int64_t i = t; i < (hw >> 2); i += nt) {
            const float4 v = x4[i];
            o4[i] = prob_byte(v.x, cmin, k) | (prob_byte(v.y, cmin, k) << 8) | (prob_byte(v.z, cmin, k) << 16) |
                    (prob_byte(v.w, cmin, k) << 24);
        }
    } else {
        for (int64_t i = t; i < hw; i += nt) out[i] = (uint8_t)prob_byte(x[i], cmin, k);
    }
}

// ------------------------------------------------------------------------------------------ jf_counts
constexpr int kPackWordsPerWave = 4;
constexpr int kJfTileRows = 16, kJfTileWords = 8, kJfThreads = kJfTileRows * kJfTileWords;
constexpr int kJfLdsWords = kJfTileWords + 2;  // one halo word on either side

__host__ __device__ inline int jf_words(int W) { return (W + 63) / 64; }
inline size_t jf_lds_bytes(int r) {
    return (size_t)2 * (kJfTileRows + 2 * r) * kJfLdsWords * sizeof(u64) + (2 * kMaxRadius + 1) * sizeof(int);
}

// one wave packs kPackWordsPerWave consecutive words (of rows of W pixels each, Wp words a row)
__global__ __launch_bounds__(kEvalThreads) void k_jf_pack(const float *__restrict__ logits,
                                                          const uint8_t *__restrict__ gt, int W, int Wp,
                                                          int64_t n_words, u64 *__restrict__ plane_a,
                                                          u64 *__restrict__ plane_b, int32_t *__restrict__ counts,
                                                          int n_counts) {
    const int64_t gtid = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
    if (gtid < n_counts) counts[gtid] = 0;
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (gtid >> 6) * kPackWordsPerWave;
    float v[kPackWordsPerWave];
    uint8_t g[kPackWordsPerWave];
#pragma unroll
    for (int j = 0; j < kPackWordsPerWave; ++j) {
        const int64_t w = w0 + j, row = w / Wp;  // row counts through all frames
        const int x = (int)(w - row * Wp) * 64 + lane;
        const bool in = w < n_words && x < W;
        v[j] = in ? logits[row * W + x] : -1.f;
        g[j] = in ? gt[row * W + x] : (uint8_t)0;
    }
#pragma unroll
    for (int j = 0; j < kPackWordsPerWave; ++j) {
        const u64 a = __ballot(v[j] >= 0.f), b = __ballot(g[j] != 0);
        if (lane == 0 && w0 + j < n_words) {
            plane_a[w0 + j] = a;
            plane_b[w0 + j] = b;
        }
    }
}

// the boundary-map word (y, c) of a plane: S != right neighbour, != the pixel below, != the one below right; the last row
// compares to the right only, the last column downwards only, the corner is 0
__device__ __forceinline__ u64 bmap_word(const u64 *__restrict__ plane, int y, int c, int H, int W, int Wp) {
    const u64 *row = plane + (int64_t)y * Wp;
    const u64 s = row[c], sn = (c + 1 < Wp) ? row[c + 1] : 0;
    const int nb = W - 1 - 64 * c;  // columns of this word left of the image's last one
    const u64 not_last = nb >= 64 ? ~0ull : (nb <= 0 ? 0ull : ((1ull << nb) - 1));
    const u64 right = s ^ ((s >> 1) | (sn << 63));
    if (y >= H - 1) return right & not_last;
    const u64 d = row[Wp + c], dn = (c + 1 < Wp) ? row[Wp + c + 1] : 0;
    return ((right | (s ^ ((d >> 1) | (dn << 63)))) & not_last) | (s ^ d);
}

// OR of (hi:lo) shifted up by 0..h bits (h <= 63), its high word: `m` spread towards higher columns, fed by `below`
__device__ __forceinline__ u64 spread_up(u64 below, u64 m, int h) {
    u64 lo = below, hi = m;
    for (int cover = 0; cover < h;) {
        const int s = min(cover + 1, h - cover);
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
        cover += s;
    }
    return hi;
}
__device__ __forceinline__ u64 spread_down(u64 m, u64 above, int h) {
    u64 lo = m, hi = above;
    for (int cover = 0; cover < h;) {
        const int s = min(cover + 1, h - cover);
        lo |= (lo >> s) | (hi << (64 - s));
        hi |= hi >> s;
        cover += s;
    }
    return lo;
}

// grid (ceil(Wp / 8), ceil(H / 16), N)
__global__ __launch_bounds__(kJfThreads) void k_jf_count(const u64 *__restrict__ plane_a, const u64 *__restrict__ plane_b,
                                                         int H, int W, int Wp, int r, int32_t *__restrict__ counts) {
    extern __shared__ __align__(16) uint8_t jf_smem[];
    const int rows_l = kJfTileRows + 2 * r;
    u64 *ba = reinterpret_cast<u64 *>(jf_smem), *bb = ba + rows_l * kJfLdsWords;
    int *half = reinterpret_cast<int *>(bb + rows_l * kJfLdsWords);  // [2r+1]: the disk's half-width at each dy
    __shared__ int s_cnt[6];
    const int64_t plane = (int64_t)H * Wp;
    plane_a += blockIdx.z * plane;
    plane_b += blockIdx.z * plane;
    const int y0 = blockIdx.y * kJfTileRows, c0 = blockIdx.x * kJfTileWords;
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    for (int i = threadIdx.x; i <= 2 * r; i += kJfThreads) {
        const int dy = i - r, rem = r * r - dy * dy;
        int h = 0;
        while ((h + 1) * (h + 1) <= rem) ++h;
        half[i] = h;
    }
    for (int i = threadIdx.x; i < rows_l * kJfLdsWords; i += kJfThreads) {
        const int ly = i / kJfLdsWords, lc = i - ly * kJfLdsWords;
        const int y = y0 - r + ly, c = c0 - 1 + lc;
        const bool in = y >= 0 && y < H && c >= 0 && c < Wp;
        ba[i] = in ? bmap_word(plane_a, y, c, H, W, Wp) : 0;
        bb[i] = in ? bmap_word(plane_b, y, c, H, W, Wp) : 0;
    }
    __syncthreads();
    const int ty = threadIdx.x / kJfTileWords, tc = threadIdx.x % kJfTileWords;
    const int y = y0 + ty, c = c0 + tc;
    u64 dil_a = 0, dil_b = 0;
    for (int i = 0; i <= 2 * r; ++i) {
        const int h = half[i];
        const u64 *ra = ba + (ty + i) * kJfLdsWords + tc, *rb = bb + (ty + i) * kJfLdsWords + tc;
        dil_a |= spread_up(ra[0], ra[1], h) | spread_down(ra[1], ra[2], h);
        dil_b |= spread_up(rb[0], rb[1], h) | spread_down(rb[1], rb[2], h);
    }
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    if (y < H && c < Wp) {
        const u64 a = plane_a[(int64_t)y * Wp + c], b = plane_b[(int64_t)y * Wp + c];
        const u64 ea = ba[(ty + r) * kJfLdsWords + tc + 1], eb = bb[(ty + r) * kJfLdsWords + tc + 1];
        cnt[0] = __popcll(a & b);
        cnt[1] = __popcll(a | b);
        cnt[2] = __popcll(ea);
        cnt[3] = __popcll(eb);
        cnt[4] = __popcll(ea & dil_b);
        cnt[5] = __popcll(eb & dil_a);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int v = cnt[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_cnt[threadIdx.x]) atomicAdd(&counts[blockIdx.z * 6 + threadIdx.x], s_cnt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------ several objects
// (ObjectLogits and the merge rule of one pixel, merge_take: common.hpp)
// grid (blocks, N).  vec: every map and the labels are 16-byte / 4-byte aligned and hw % 4 == 0
__global__ __launch_bounds__(kEvalThreads) void k_merge_objects(const ObjectLogits maps, int K, int64_t hw, int vec,
                                                                uint8_t *__restrict__ out) {
    const int64_t frame = (int64_t)blockIdx.y * hw;
    out += frame;
    const int64_t t = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x, nt = (int64_t)gridDim.x * kEvalThreads;
    if (vec) {
        uint32_t *__restrict__ o4 = reinterpret_cast<uint32_t *>(out);
        for (int64_t i = t; i < (hw >> 2); i += nt) {
            float bv[4] = {-1.f, -1.f, -1.f, -1.f};
            uint32_t b[4] = {0u, 0u, 0u, 0u};
            for (int k = 0; k < K; ++k) {
                const float4 v = reinterpret_cast<const float4 *>(maps.p[k] + frame)[i];
                merge_take(v.x, (uint32_t)k, bv[0], b[0]);
                merge_take(v.y, (uint32_t)k, bv[1], b[1]);
                merge_take(v.z, (uint32_t)k, bv[2], b[2]);
                merge_take(v.w, (uint32_t)k, bv[3], b[3]);
            }
            o4[i] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        }
    } else {
        for (int64_t i = t; i < hw; i += nt) {
            float bv = -1.f;
            uint32_t b = 0u;
            for (int k = 0; k < K; ++k) merge_take(maps.p[k][frame + i], (uint32_t)k, bv, b);
            out[i] = (uint8_t)b;
        }
    }
}

// one wave packs kPackWordsPerWave consecutive words of the label maps into the planes of all K objects; lane k - 1 keeps
// and writes object k's two words
__global__ __launch_bounds__(kEvalThreads) void k_jf_pack_labels(const uint8_t *__restrict__ pred,
                                                                 const uint8_t *__restrict__ gt, int H, int W, int Wp, int K,
                                                                 int64_t n_words, u64 *__restrict__ plane_a,
                                                                 u64 *__restrict__ plane_b, int32_t *__restrict__ counts,
                                                                 int n_counts) {
    const int64_t gtid = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
    for (int64_t i = gtid; i < n_counts; i += (int64_t)gridDim.x * kEvalThreads) counts[i] = 0;
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (gtid >> 6) * kPackWordsPerWave;
    uint8_t p[kPackWordsPerWave], g[kPackWordsPerWave];
#pragma unroll
    for (int j = 0; j < kPackWordsPerWave; ++j) {
        const int64_t w = w0 + j, row = w / Wp;  // row counts through all frames
        const int x = (int)(w - row * Wp) * 64 + lane;
        const bool in = w < n_words && x < W;
        p[j] = in ? pred[row * W + x] : (uint8_t)0;
        g[j] = in ? gt[row * W + x] : (uint8_t)0;
    }
#pragma unroll
    for (int j = 0; j < kPackWordsPerWave; ++j) {
        u64 a = 0, b = 0;
        for (int k = 1; k <= K; ++k) {
            const u64 ak = __ballot(p[j] == k), bk = __ballot(g[j] == k);
            a = lane == k - 1 ? ak : a;
            b = lane == k - 1 ? bk : b;
        }
        const int64_t w = w0 + j, row = w / Wp, n = row / H;
        if (lane < K && w < n_words) {
            // word (y, c) of frame n -> plane n * K + lane
            const int64_t at = ((n * K + lane) * H + (row - n * H)) * Wp + (w - row * Wp);
            plane_a[at] = a;
            plane_b[at] = b;
        }
    }
}
}  // namespace

extern "C" int fosvos_prob_bytes(const float *logits, int N, int H, int W, float *minmax, uint8_t *out, int device,
                                 void *stream) {
    FOSVOS_REQUIRE(logits && minmax && out, FOSVOS_E_ARG, "prob_bytes: null pointer");
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, FOSVOS_E_SHAPE, "prob_bytes: N=%d (<= 65535) H=%d W=%d", N, H, W);
    FOSVOS_ENTER(device);
    const int64_t hw = (int64_t)H * W;
    const int vec = (hw % 4 == 0) && ((((uintptr_t)logits | (uintptr_t)out) & 15) == 0);
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(vec ? hw / 4 : hw, kEvalThreads), 2048);
    hipStream_t st = (hipStream_t)stream;
    FOSVOS_PROF("k_minmax_init", stream, 0.0);
    hipLaunchKernelGGL(k_minmax_init, dim3((unsigned)cdiv(N, 64)), dim3(64), 0, st, minmax, N);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_minmax", stream, 0.0);
    // at most 128 workgroups a frame: every one of them ends in two atomics on the frame's record, and same-address atomics
    // run one after the other (measured at 5x480x854: with a pair per wave of 401 workgroups a frame the op took 38.6 us a
    // frame, with a pair per workgroup of 128 it takes 5.1)
    hipLaunchKernelGGL(k_minmax, dim3(std::min(blocks, 128u), (unsigned)N), dim3(kEvalThreads), 0, st, logits, hw, vec, minmax);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_prob_map", stream, 0.0);
    hipLaunchKernelGGL(k_prob_map, dim3(blocks, (unsigned)N), dim3(kEvalThreads), 0, st, logits, hw, vec, minmax, out);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" size_t fosvos_jf_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)2 * N * H * jf_words(W) * sizeof(u64);
}

extern "C" int fosvos_jf_counts(const float *logits, const uint8_t *gt, int N, int H, int W, int radius, int32_t *counts,
                                void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(logits && gt && counts && workspace, FOSVOS_E_ARG, "jf_counts: null pointer");
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX &&
                       cdiv(H, kJfTileRows) <= 65535 && (int64_t)N * H * W <= ((int64_t)1 << 40),
                   FOSVOS_E_SHAPE, "jf_counts: N=%d (<= 65535) H=%d W=%d", N, H, W);
    FOSVOS_REQUIRE(radius >= 1 && radius <= kMaxRadius, FOSVOS_E_ARG, "jf_counts: radius %d outside [1, %d]", radius,
                   kMaxRadius);
    FOSVOS_REQUIRE(((uintptr_t)workspace & 7) == 0, FOSVOS_E_ARG, "jf_counts: the workspace must be 8-byte aligned");
    const size_t need = fosvos_jf_workspace_bytes(N, H, W);
    FOSVOS_REQUIRE(workspace_bytes >= need, FOSVOS_E_WORKSPACE, "jf_counts: workspace %zu B < %zu B", workspace_bytes, need);
    FOSVOS_ENTER(device);
    const int Wp = jf_words(W);
    const int64_t n_words = (int64_t)N * H * Wp;
    u64 *plane_a = reinterpret_cast<u64 *>(workspace), *plane_b = plane_a + n_words;
    hipStream_t st = (hipStream_t)stream;
    // (16 threads a word, so the 6N counters always find a thread to zero them)
    const int64_t pack_blocks = cdiv(n_words, (kEvalThreads / 64) * kPackWordsPerWave);
    FOSVOS_PROF("k_jf_pack", stream, 0.0);
    hipLaunchKernelGGL(k_jf_pack, dim3((unsigned)pack_blocks), dim3(kEvalThreads), 0, st, logits, gt, W, Wp, n_words, plane_a,
                       plane_b, counts, 6 * N);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_jf_count", stream, 0.0);
    hipLaunchKernelGGL(k_jf_count, dim3((unsigned)cdiv(Wp, kJfTileWords), (unsigned)cdiv(H, kJfTileRows), (unsigned)N),
                       dim3(kJfThreads), jf_lds_bytes(radius), st, plane_a, plane_b, H, W, Wp, radius, counts);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_merge_objects(const float *const *logits, int K, int N, int H, int W, uint8_t *labels, int device,
                                    void *stream) {
    FOSVOS_REQUIRE(K >= 1 && K <= kMaxObjects, FOSVOS_E_ARG, "merge_objects: K=%d outside [1, %d]", K, kMaxObjects);
    FOSVOS_REQUIRE(logits && labels, FOSVOS_E_ARG, "merge_objects: null pointer");
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, FOSVOS_E_SHAPE, "merge_objects: N=%d (<= 65535) H=%d W=%d", N, H, W);
    ObjectLogits maps = {};
    uintptr_t align = (uintptr_t)labels & 3;
    for (int k = 0; k < K; ++k) {
        FOSVOS_REQUIRE(logits[k] != nullptr, FOSVOS_E_ARG, "merge_objects: null logit map %d", k);
        maps.p[k] = logits[k];
        align |= (uintptr_t)logits[k] & 15;
    }
    FOSVOS_ENTER(device);
    const int64_t hw = (int64_t)H * W;
    const int vec = (hw % 4 == 0) && align == 0;
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(vec ? hw / 4 : hw, kEvalThreads), 2048);
    FOSVOS_PROF("k_merge_objects", stream, 0.0);
    hipLaunchKernelGGL(k_merge_objects, dim3(blocks, (unsigned)N), dim3(kEvalThreads), 0, (hipStream_t)stream, maps, K, hw, vec,
                       labels);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" size_t fosvos_jf_labels_workspace_bytes(int N, int K, int H, int W) {
    if (N <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)2 * N * K * H * jf_words(W) * sizeof(u64);
}

extern "C" int fosvos_jf_counts_labels(const uint8_t *pred, const uint8_t *gt, int N, int K, int H, int W, int radius,
                                       int32_t *counts, void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(pred && gt && counts && workspace, FOSVOS_E_ARG, "jf_counts_labels: null pointer");
    FOSVOS_REQUIRE(K >= 1 && K <= kMaxObjects, FOSVOS_E_ARG, "jf_counts_labels: K=%d outside [1, %d]", K, kMaxObjects);
    FOSVOS_REQUIRE(N > 0 && (int64_t)N * K <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= INT32_MAX &&
                       cdiv(H, kJfTileRows) <= 65535 && (int64_t)N * K * H * W <= ((int64_t)1 << 40),
                   FOSVOS_E_SHAPE, "jf_counts_labels: N=%d K=%d (N K <= 65535) H=%d W=%d", N, K, H, W);
    FOSVOS_REQUIRE(radius >= 1 && radius <= kMaxRadius, FOSVOS_E_ARG, "jf_counts_labels: radius %d outside [1, %d]", radius,
                   kMaxRadius);
    FOSVOS_REQUIRE(((uintptr_t)workspace & 7) == 0, FOSVOS_E_ARG, "jf_counts_labels: the workspace must be 8-byte aligned");
    const size_t need = fosvos_jf_labels_workspace_bytes(N, K, H, W);
    FOSVOS_REQUIRE(workspace_bytes >= need, FOSVOS_E_WORKSPACE, "jf_counts_labels: workspace %zu B < %zu B", workspace_bytes,
                   need);
    FOSVOS_ENTER(device);
    const int Wp = jf_words(W);
    const int64_t n_words = (int64_t)N * H * Wp;  // of one label map
    u64 *plane_a = reinterpret_cast<u64 *>(workspace), *plane_b = plane_a + n_words * K;
    hipStream_t st = (hipStream_t)stream;
    const int64_t pack_blocks = cdiv(n_words, (kEvalThreads / 64) * kPackWordsPerWave);
    FOSVOS_PROF("k_jf_pack_labels", stream, 0.0);
    hipLaunchKernelGGL(k_jf_pack_labels, dim3((unsigned)pack_blocks), dim3(kEvalThreads), 0, st, pred, gt, H, W, Wp, K, n_words,
                       plane_a, plane_b, counts, 6 * N * K);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_jf_count", stream, 0.0);
    hipLaunchKernelGGL(k_jf_count, dim3((unsigned)cdiv(Wp, kJfTileWords), (unsigned)cdiv(H, kJfTileRows), (unsigned)(N * K)),
                       dim3(kJfThreads), jf_lds_bytes(radius), st, plane_a, plane_b, H, W, Wp, radius, counts);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
