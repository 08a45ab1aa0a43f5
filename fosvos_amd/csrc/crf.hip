// Refining the test pass's logits with a local CRF on the frame's colours (opt-in): mean-field inference over a window of
// radius r with an appearance and a smoothness kernel.  util/mask_crf.py states the arithmetic in numpy; the output is compared
// with it bit for bit, so every fp64 operation here is one IEEE operation of that file, in its order, and nothing is
// contracted.  There is no transcendental: every exp and tanh is a table [RGB | A | B | D] the host made (mask_crf.tables).
//
// fosvos_crf_refine: `iterations` launches of ONE kernel body, k_crf_iterate; a launch is a mean-field iteration.
//   launch t   reads z^{t-1} - the clipped logit u in the first launch, else an fp64 map of the workspace - and writes z^t to
//              the workspace's other map; the last launch writes float32(z^T) to `out`.  A workgroup reads the halo of z^{t-1}
//              that other workgroups of launch t-1 wrote, which is why an iteration is a launch: no workgroup waits for another
//              and there are no atomics.
// A workgroup of 256 threads owns a TILE of 16 rows x 64 columns of one frame's map:
//   stage      the tables' [RGB | A | B] (256 + 2 (2r+1)^2 doubles, 4 KB at r = 5) and, for the tile and a halo of r on every
//              side - up to 26 x 74 pixels -, the guide as ONE packed word a pixel (level of plane 0 | plane 1 << 8 | plane 2 <<
//              16; 7.5 KB) and the belief of z^{t-1} as fp64 (15 KB), computed while staging; D, which only this phase reads,
//              twice a staged pixel, comes through the cache.  Thread t takes staged elements t, t + 256, ...: consecutive
//              threads, consecutive columns.  27 KB static: five workgroups share a CU's LDS.
//   window     thread t owns column t % 64 of rows t / 64, + 4, + 8, + 12: four pixels whose 16 running sums stay in registers.
//              It walks the offsets in the definition's order (dy outside, dx inside, ascending) once for all four pixels;
//              consecutive lanes read consecutive LDS words.  A neighbour outside the map is skipped: a staged element outside
//              the map is never read and is not written either.
//   finish     ma = Na / Da, ms = Ns / Ds (0.0 where the denominator is not positive), z = (u + wa ma) + ws ms.
// Da and Ds do not depend on t; they are summed again in every launch (keeping them would cost two more fp64 maps of traffic and
// save 2 of 9 fp64 operations a neighbour: not measured, not built).
#include <math.h>

#include "common.hpp"

// the fp64 expressions are the host's, operation for operation
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kTileH = 16, kTileW = 64;
constexpr int kCrfThreads = 256;
constexpr int kMaxRadius = 5, kMaxIterations = 10;
constexpr int kStageH = kTileH + 2 * kMaxRadius, kStageW = kTileW + 2 * kMaxRadius;  // 26 x 74
constexpr int kRowsPerThread = kTileH * kTileW / kCrfThreads;                        // 4
constexpr int kMaxSide = 8192;
constexpr int kLevels = 256;                                                         // RGB[0..255]
constexpr int kMaxWindow = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);              // 121
constexpr int kBeliefSteps = 2048;                                                   // D[0..2048]
constexpr double kBeliefLimit = 16.0, kBeliefPerUnit = 64.0;

struct CrfGeom {
    int H, W, r;
    int tiles_x, tiles_y;
    int first, last;  // the launch reads the logits as z^0; it writes `out`
};
struct CrfParams {
    double clip, wa, ws;
    double mean[3];
};
struct Lds {
    double s[kStageH * kStageW];      // the belief of z^{t-1}; element (sy, sx) is map pixel (y0 - r + sy, x0 - r + sx)
    uint32_t g[kStageH * kStageW];    // the guide's three levels, packed
    double tab[kLevels + 2 * kMaxWindow];  // [RGB | A | B]
};

__device__ __forceinline__ double unary(float logit, double clip) {
    const double v = (double)logit;
    const double p = v >= -clip ? v : -clip;  // a NaN compares false: -clip
    return p <= clip ? p : clip;
}
__device__ __forceinline__ uint32_t guide_level(float v, double mean) {
    const double t = ((double)v + mean) + 0.5;
    return t >= 0.0 ? (t < 256.0 ? (uint32_t)(int)floor(t) : 255u) : 0u;  // a NaN compares false: 0
}
__device__ __forceinline__ double belief(double z, const double *__restrict__ D) {
    double zc = z < -kBeliefLimit ? -kBeliefLimit : z;
    zc = zc > kBeliefLimit ? kBeliefLimit : zc;
    const double p = (zc + kBeliefLimit) * kBeliefPerUnit;
    // 0 <= p <= 2048 for every finite z; the clamp from below keeps the index inside D whatever the tables held
    const int i = max(0, min((int)floor(p), kBeliefSteps - 1));
    const double f = p - (double)i;
    const double d0 = D[i], d1 = D[i + 1];
    return d0 + f * (d1 - d0);
}
__device__ __forceinline__ int level_gap(uint32_t a, uint32_t b, int shift) {
    const int d = (int)((a >> shift) & 255u) - (int)((b >> shift) & 255u);
    return d < 0 ? -d : d;
}

__global__ __launch_bounds__(kCrfThreads) void k_crf_iterate(const float *__restrict__ image, const float *__restrict__ logits,
                                                            const double *__restrict__ tables, const double *__restrict__ zin,
                                                            double *__restrict__ zout, float *__restrict__ out, CrfGeom g,
                                                            CrfParams p) {
    __shared__ Lds lds;
    const int r = g.r, kk = 2 * r + 1;
    const int x0 = (int)(blockIdx.x % g.tiles_x) * kTileW;
    const int y0 = (int)((blockIdx.x / g.tiles_x) % g.tiles_y) * kTileH;
    const int64_t n = blockIdx.x / ((unsigned)g.tiles_x * g.tiles_y);
    const int64_t plane = (int64_t)g.H * g.W;
    const float *__restrict__ im = image + n * 3 * plane;
    const float *__restrict__ lg = logits + n * plane;
    const double *__restrict__ D = tables + kLevels + 2 * kk * kk;

    for (int idx = threadIdx.x; idx < kLevels + 2 * kk * kk; idx += kCrfThreads) lds.tab[idx] = tables[idx];
    const int cw = kTileW + 2 * r, staged = (kTileH + 2 * r) * cw;
    for (int idx = threadIdx.x; idx < staged; idx += kCrfThreads) {
        const int sy = idx / cw, sx = idx - sy * cw;
        const int y = y0 - r + sy, x = x0 - r + sx;
        if (y < 0 || y >= g.H || x < 0 || x >= g.W) continue;
        const int64_t px = (int64_t)y * g.W + x;
        const int at = sy * kStageW + sx;
        lds.g[at] = guide_level(im[px], p.mean[0]) | (guide_level(im[plane + px], p.mean[1]) << 8) |
                    (guide_level(im[2 * plane + px], p.mean[2]) << 16);
        lds.s[at] = belief(g.first ? unary(lg[px], p.clip) : zin[n * plane + px], D);
    }
    __syncthreads();

    const double *__restrict__ rgb = lds.tab;
    const double *__restrict__ ta = lds.tab + kLevels;
    const double *__restrict__ tb = ta + kk * kk;
    const int tx = threadIdx.x % kTileW, x = x0 + tx;
    const int ty0 = threadIdx.x / kTileW;
    bool ok[kRowsPerThread];
    uint32_t gc[kRowsPerThread];
    double na[kRowsPerThread], da[kRowsPerThread], ns[kRowsPerThread], ds[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int ty = ty0 + (kCrfThreads / kTileW) * k;
        ok[k] = y0 + ty < g.H && x < g.W;
        gc[k] = ok[k] ? lds.g[(ty + r) * kStageW + tx + r] : 0u;
        na[k] = da[k] = ns[k] = ds[k] = 0.0;
    }
    for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
            const int xx = x + dx;
            if ((dy == 0 && dx == 0) || xx < 0 || xx >= g.W) continue;
            const double wa = ta[(dy + r) * kk + dx + r], wb = tb[(dy + r) * kk + dx + r];
#pragma unroll
            for (int k = 0; k < kRowsPerThread; ++k) {
                const int ty = ty0 + (kCrfThreads / kTileW) * k;
                const int yy = y0 + ty + dy;
                if (!ok[k] || yy < 0 || yy >= g.H) continue;
                const int at = (ty + r + dy) * kStageW + tx + r + dx;
                const uint32_t gj = lds.g[at];
                const double sj = lds.s[at];
                const double a = wa * ((rgb[level_gap(gc[k], gj, 0)] * rgb[level_gap(gc[k], gj, 8)]) * rgb[level_gap(gc[k], gj, 16)]);
                na[k] = na[k] + a * sj;
                da[k] = da[k] + a;
                ns[k] = ns[k] + wb * sj;
                ds[k] = ds[k] + wb;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        if (!ok[k]) continue;
        const int y = y0 + ty0 + (kCrfThreads / kTileW) * k;
        const int64_t px = (int64_t)y * g.W + x;
        const double ma = da[k] > 0.0 ? na[k] / da[k] : 0.0;
        const double ms = ds[k] > 0.0 ? ns[k] / ds[k] : 0.0;
        const double z = (unary(lg[px], p.clip) + p.wa * ma) + p.ws * ms;
        if (g.last)
            out[n * plane + px] = (float)z;
        else
            zout[n * plane + px] = z;
    }
}
// ------------------------------------------------------------------------------------------ the joint CRF over K + 1 labels
// fosvos_crf_labels (util/label_crf.py states it): the same launch structure, tile, thread map and window walk, with K + 1
// beliefs a pixel - a soft-max over the labels, piecewise linear on the table E - in the place of one.  z^t is K + 1 fp64 maps
// a frame, [N, K+1, H, W], in either half of the workspace by turns.  The beliefs of a staged pixel do not all fit in LDS, so a
// workgroup walks the labels in CHUNKS of kLabelChunk: per chunk it stages the chunk's beliefs (for which it reads all K + 1
// values of z^{t-1} of the staged pixel, twice: the largest, then the sum of the e's), walks the window - the weight `a` of a
// neighbour is computed once and applied to every label of the chunk - and finishes the chunk's labels.  The guide and [RGB | A
// | B] are staged once.  Recomputed per chunk: a staged pixel's largest z and S, and a neighbour's `a`, Da and Ds (the same
// operations on the same operands: the same bits).  4 x 15 KB + 7.5 KB + 4 KB = 71.5 KB static: two workgroups share a CU's LDS.
constexpr int kLabelChunk = 4;
constexpr int kExpSteps = 2048;  // E[0..2048]
constexpr double kExpLimit = 32.0, kExpPerUnit = 64.0;

struct LabelGeom {
    int H, W, r, K;
    int tiles_x, tiles_y;
    int first, last;  // the launch reads the logits as z^0; it writes the labels and the scores
};
struct LabelLds {
    double q[kLabelChunk][kStageH * kStageW];  // the beliefs of the chunk's labels; the element order of Lds::s
    uint32_t g[kStageH * kStageW];
    double tab[kLevels + 2 * kMaxWindow];
};

__device__ __forceinline__ double exp_gap(double m, double z, const double *__restrict__ E) {
    const double gap = m - z;
    const double d = gap < kExpLimit ? gap : kExpLimit;
    const double p = d * kExpPerUnit;
    // 0 <= p <= 2048 for finite z <= m; the clamps keep the index inside E whatever the workspace or the tables held
    const int i = max(0, min((int)floor(p), kExpSteps - 1));
    const double f = p - (double)i;
    const double e0 = E[i], e1 = E[i + 1];
    return e0 + f * (e1 - e0);
}

__global__ __launch_bounds__(kCrfThreads) void k_crf_labels_iterate(const float *__restrict__ image, const ObjectLogits maps,
                                                                   const double *__restrict__ tables,
                                                                   const double *__restrict__ zin, double *__restrict__ zout,
                                                                   uint8_t *__restrict__ labels, float *__restrict__ scores,
                                                                   LabelGeom g, CrfParams p) {
    __shared__ LabelLds lds;
    const int r = g.r, kk = 2 * r + 1, L = g.K + 1;
    const int x0 = (int)(blockIdx.x % g.tiles_x) * kTileW;
    const int y0 = (int)((blockIdx.x / g.tiles_x) % g.tiles_y) * kTileH;
    const int64_t n = blockIdx.x / ((unsigned)g.tiles_x * g.tiles_y);
    const int64_t plane = (int64_t)g.H * g.W;
    const float *__restrict__ im = image + n * 3 * plane;
    const double *__restrict__ E = tables + kLevels + 2 * kk * kk;
    const int64_t frame = n * plane;         // of a net's logits and of the labels
    const int64_t zframe = n * L * plane;    // of z and of the scores

    for (int idx = threadIdx.x; idx < kLevels + 2 * kk * kk; idx += kCrfThreads) lds.tab[idx] = tables[idx];
    const int cw = kTileW + 2 * r, staged = (kTileH + 2 * r) * cw;
    for (int idx = threadIdx.x; idx < staged; idx += kCrfThreads) {
        const int sy = idx / cw, sx = idx - sy * cw;
        const int y = y0 - r + sy, x = x0 - r + sx;
        if (y < 0 || y >= g.H || x < 0 || x >= g.W) continue;
        const int64_t px = (int64_t)y * g.W + x;
        lds.g[sy * kStageW + sx] = guide_level(im[px], p.mean[0]) | (guide_level(im[plane + px], p.mean[1]) << 8) |
                                   (guide_level(im[2 * plane + px], p.mean[2]) << 16);
    }

    const double *__restrict__ rgb = lds.tab;
    const double *__restrict__ ta = lds.tab + kLevels;
    const double *__restrict__ tb = ta + kk * kk;
    const int tx = threadIdx.x % kTileW, x = x0 + tx;
    const int ty0 = threadIdx.x / kTileW;
    bool ok[kRowsPerThread];
    double bestv[kRowsPerThread];
    uint32_t best[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        ok[k] = y0 + ty0 + (kCrfThreads / kTileW) * k < g.H && x < g.W;
        bestv[k] = -INFINITY;  // label 0 takes the first comparison: every z is finite
        best[k] = 0u;
    }

    for (int c0 = 0; c0 < L; c0 += kLabelChunk) {
        const int nl = min(kLabelChunk, L - c0);
        __syncthreads();  // the guide is staged; the window of the chunk before has read its beliefs
        for (int idx = threadIdx.x; idx < staged; idx += kCrfThreads) {
            const int sy = idx / cw, sx = idx - sy * cw;
            const int y = y0 - r + sy, x = x0 - r + sx;
            if (y < 0 || y >= g.H || x < 0 || x >= g.W) continue;
            const int64_t px = (int64_t)y * g.W + x;
            double m = g.first ? 0.0 : zin[zframe + px];
            for (int l = 1; l < L; ++l) {
                const double v = g.first ? unary(maps.p[l - 1][frame + px], p.clip) : zin[zframe + l * plane + px];
                m = v > m ? v : m;
            }
            double S = 0.0, e[kLabelChunk];
#pragma unroll
            for (int c = 0; c < kLabelChunk; ++c) e[c] = 0.0;
            for (int l = 0; l < L; ++l) {
                const double v =
                    g.first ? (l == 0 ? 0.0 : unary(maps.p[l - 1][frame + px], p.clip)) : zin[zframe + l * plane + px];
                const double ev = exp_gap(m, v, E);
                S = S + ev;
#pragma unroll
                for (int c = 0; c < kLabelChunk; ++c) e[c] = l == c0 + c ? ev : e[c];
            }
#pragma unroll
            for (int c = 0; c < kLabelChunk; ++c)
                if (c < nl) lds.q[c][sy * kStageW + sx] = e[c] / S;
        }
        __syncthreads();

        uint32_t gc[kRowsPerThread];
        double da[kRowsPerThread], ds[kRowsPerThread], na[kRowsPerThread][kLabelChunk], ns[kRowsPerThread][kLabelChunk];
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            const int ty = ty0 + (kCrfThreads / kTileW) * k;
            gc[k] = ok[k] ? lds.g[(ty + r) * kStageW + tx + r] : 0u;
            da[k] = ds[k] = 0.0;
#pragma unroll
            for (int c = 0; c < kLabelChunk; ++c) na[k][c] = ns[k][c] = 0.0;
        }
        for (int dy = -r; dy <= r; ++dy) {
            for (int dx = -r; dx <= r; ++dx) {
                const int xx = x + dx;
                if ((dy == 0 && dx == 0) || xx < 0 || xx >= g.W) continue;
                const double wa = ta[(dy + r) * kk + dx + r], wb = tb[(dy + r) * kk + dx + r];
#pragma unroll
                for (int k = 0; k < kRowsPerThread; ++k) {
                    const int ty = ty0 + (kCrfThreads / kTileW) * k;
                    const int yy = y0 + ty + dy;
                    if (!ok[k] || yy < 0 || yy >= g.H) continue;
                    const int at = (ty + r + dy) * kStageW + tx + r + dx;
                    const uint32_t gj = lds.g[at];
                    const double a =
                        wa * ((rgb[level_gap(gc[k], gj, 0)] * rgb[level_gap(gc[k], gj, 8)]) * rgb[level_gap(gc[k], gj, 16)]);
                    da[k] = da[k] + a;
                    ds[k] = ds[k] + wb;
#pragma unroll
                    for (int c = 0; c < kLabelChunk; ++c) {
                        if (c < nl) {
                            const double qj = lds.q[c][at];
                            na[k][c] = na[k][c] + a * qj;
                            ns[k][c] = ns[k][c] + wb * qj;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            if (!ok[k]) continue;
            const int y = y0 + ty0 + (kCrfThreads / kTileW) * k;
            const int64_t px = (int64_t)y * g.W + x;
#pragma unroll
            for (int c = 0; c < kLabelChunk; ++c) {
                if (c >= nl) continue;
                const int l = c0 + c;
                const double ma = da[k] > 0.0 ? na[k][c] / da[k] : 0.0;
                const double ms = ds[k] > 0.0 ? ns[k][c] / ds[k] : 0.0;
                const double u = l == 0 ? 0.0 : unary(maps.p[l - 1][frame + px], p.clip);
                const double z = (u + p.wa * ma) + p.ws * ms;
                if (!g.last) {
                    zout[zframe + l * plane + px] = z;
                    continue;
                }
                if (scores) scores[zframe + l * plane + px] = (float)z;
                // an object beats the background on a tie, the lowest object wins among equal objects
                const bool take = best[k] == 0u ? z >= bestv[k] : z > bestv[k];
                bestv[k] = take ? z : bestv[k];
                best[k] = take ? (uint32_t)l : best[k];
            }
        }
    }
    if (g.last) {
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            if (!ok[k]) continue;
            const int y = y0 + ty0 + (kCrfThreads / kTileW) * k;
            labels[frame + (int64_t)y * g.W + x] = (uint8_t)best[k];
        }
    }
}
}  // namespace

extern "C" size_t fosvos_crf_labels_workspace_bytes(int N, int K, int H, int W) {
    if (N <= 0 || K < 1 || K > kMaxObjects || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide) return 0;
    return (size_t)N * 2 * (K + 1) * H * W * sizeof(double);
}

extern "C" int fosvos_crf_labels(const float *image, const float *const *logits, int K, const double *tables, int N, int H, int W,
                                 int iterations, int radius, double weight_appearance, double weight_smooth, double clip,
                                 const float mean[3], uint8_t *labels, float *scores, void *workspace, size_t workspace_bytes,
                                 int device, void *stream) {
    FOSVOS_REQUIRE(K >= 1 && K <= kMaxObjects, FOSVOS_E_ARG, "crf_labels: K=%d outside [1, %d]", K, kMaxObjects);
    FOSVOS_REQUIRE(image && logits && tables && mean && labels && workspace, FOSVOS_E_ARG, "crf_labels: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, FOSVOS_E_SHAPE,
                   "crf_labels: N=%d, maps of %dx%d (sides of 1..%d)", N, H, W, kMaxSide);
    FOSVOS_REQUIRE(iterations >= 1 && iterations <= kMaxIterations, FOSVOS_E_ARG, "crf_labels: %d iterations outside [1, %d]",
                   iterations, kMaxIterations);
    FOSVOS_REQUIRE(radius >= 1 && radius <= kMaxRadius, FOSVOS_E_ARG, "crf_labels: radius %d outside [1, %d]", radius, kMaxRadius);
    FOSVOS_REQUIRE(weight_appearance >= 0.0 && weight_appearance <= 100.0 && weight_smooth >= 0.0 && weight_smooth <= 100.0,
                   FOSVOS_E_ARG, "crf_labels: weights %g and %g outside [0, 100]", weight_appearance, weight_smooth);
    FOSVOS_REQUIRE(clip > 0.0 && clip <= 1e4, FOSVOS_E_ARG, "crf_labels: clip %g outside (0, 1e4]", clip);
    ObjectLogits maps = {};
    uintptr_t align = (uintptr_t)image | (uintptr_t)scores;
    for (int k = 0; k < K; ++k) {
        FOSVOS_REQUIRE(logits[k] != nullptr, FOSVOS_E_ARG, "crf_labels: null logit map %d", k);
        maps.p[k] = logits[k];
        align |= (uintptr_t)logits[k];
    }
    FOSVOS_REQUIRE((align & 3) == 0, FOSVOS_E_ARG, "crf_labels: the image, the logits and the scores must be 4-byte aligned");
    FOSVOS_REQUIRE((((uintptr_t)tables | (uintptr_t)workspace) & 7) == 0, FOSVOS_E_ARG,
                   "crf_labels: the tables and the workspace must be 8-byte aligned");
    FOSVOS_REQUIRE(workspace_bytes >= fosvos_crf_labels_workspace_bytes(N, K, H, W), FOSVOS_E_ARG,
                   "crf_labels: workspace of %zu bytes, need %zu", workspace_bytes, fosvos_crf_labels_workspace_bytes(N, K, H, W));
    LabelGeom g = {H, W, radius, K, (int)cdiv(W, kTileW), (int)cdiv(H, kTileH), 0, 0};
    const int64_t blocks = (int64_t)N * g.tiles_x * g.tiles_y;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "crf_labels: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    CrfParams p = {clip, weight_appearance, weight_smooth, {(double)mean[0], (double)mean[1], (double)mean[2]}};
    const size_t half = (size_t)N * (K + 1) * H * W;
    double *sets[2] = {static_cast<double *>(workspace), static_cast<double *>(workspace) + half};
    const int chunks = (int)cdiv(K + 1, kLabelChunk);
    for (int t = 1; t <= iterations; ++t) {
        g.first = t == 1;
        g.last = t == iterations;
        // launch t reads the set launch t - 1 wrote and writes the other one
        const double *zin = g.first ? nullptr : sets[t & 1];
        double *zout = g.last ? nullptr : sets[(t + 1) & 1];
        FOSVOS_PROF("k_crf_labels_iterate", stream,
                    (5.0 * chunks + 4.0 * (K + 1)) * ((2 * radius + 1) * (2 * radius + 1) - 1) * (double)N * H * W);
        hipLaunchKernelGGL(k_crf_labels_iterate, dim3((unsigned)blocks), dim3(kCrfThreads), 0, (hipStream_t)stream, image, maps,
                           tables, zin, zout, labels, scores, g, p);
        FOSVOS_LAUNCH_CHECK();
    }
    return FOSVOS_OK;
}

extern "C" size_t fosvos_crf_refine_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide) return 0;
    return (size_t)N * 2 * H * W * sizeof(double);
}

extern "C" int fosvos_crf_refine(const float *image, const float *logits, const double *tables, int N, int H, int W, int iterations,
                                 int radius, double weight_appearance, double weight_smooth, double clip, const float mean[3],
                                 float *out, void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(image && logits && tables && mean && out && workspace, FOSVOS_E_ARG, "crf_refine: null pointer");
    FOSVOS_REQUIRE(N > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide, FOSVOS_E_SHAPE,
                   "crf_refine: N=%d, maps of %dx%d (sides of 1..%d)", N, H, W, kMaxSide);
    FOSVOS_REQUIRE(iterations >= 1 && iterations <= kMaxIterations, FOSVOS_E_ARG, "crf_refine: %d iterations outside [1, %d]",
                   iterations, kMaxIterations);
    FOSVOS_REQUIRE(radius >= 1 && radius <= kMaxRadius, FOSVOS_E_ARG, "crf_refine: radius %d outside [1, %d]", radius, kMaxRadius);
    FOSVOS_REQUIRE(weight_appearance >= 0.0 && weight_appearance <= 100.0 && weight_smooth >= 0.0 && weight_smooth <= 100.0,
                   FOSVOS_E_ARG, "crf_refine: weights %g and %g outside [0, 100]", weight_appearance, weight_smooth);
    FOSVOS_REQUIRE(clip > 0.0 && clip <= 1e4, FOSVOS_E_ARG, "crf_refine: clip %g outside (0, 1e4]", clip);
    FOSVOS_REQUIRE((((uintptr_t)image | (uintptr_t)logits | (uintptr_t)out) & 3) == 0, FOSVOS_E_ARG,
                   "crf_refine: the image, the logits and out must be 4-byte aligned");
    FOSVOS_REQUIRE((((uintptr_t)tables | (uintptr_t)workspace) & 7) == 0, FOSVOS_E_ARG,
                   "crf_refine: the tables and the workspace must be 8-byte aligned");
    FOSVOS_REQUIRE(workspace_bytes >= fosvos_crf_refine_workspace_bytes(N, H, W), FOSVOS_E_ARG,
                   "crf_refine: workspace of %zu bytes, need %zu", workspace_bytes, fosvos_crf_refine_workspace_bytes(N, H, W));
    CrfGeom g = {H, W, radius, (int)cdiv(W, kTileW), (int)cdiv(H, kTileH), 0, 0};
    const int64_t blocks = (int64_t)N * g.tiles_x * g.tiles_y;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "crf_refine: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    CrfParams p = {clip, weight_appearance, weight_smooth, {(double)mean[0], (double)mean[1], (double)mean[2]}};
    double *maps[2] = {static_cast<double *>(workspace), static_cast<double *>(workspace) + (size_t)N * H * W};
    for (int t = 1; t <= iterations; ++t) {
        g.first = t == 1;
        g.last = t == iterations;
        // launch t reads the map launch t - 1 wrote and writes the other one
        const double *zin = g.first ? nullptr : maps[t & 1];
        double *zout = g.last ? nullptr : maps[(t + 1) & 1];
        FOSVOS_PROF("k_crf_iterate", stream, 9.0 * ((2 * radius + 1) * (2 * radius + 1) - 1) * (double)N * H * W);
        hipLaunchKernelGGL(k_crf_iterate, dim3((unsigned)blocks), dim3(kCrfThreads), 0, (hipStream_t)stream, image, logits, tables,
                           zin, zout, out, g, p);
        FOSVOS_LAUNCH_CHECK();
    }
    return FOSVOS_OK;
}
