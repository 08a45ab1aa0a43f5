// Edge-aware upsampling of the stream's logits (opt-in): the coefficient maps of the guided filter at the net's size.
// util/guided_upsample.py states the arithmetic in numpy; both maps are compared with it bit for bit, so every fp64
// operation here is one IEEE operation of that file, in its order, and nothing is contracted.
//
// fosvos_guided_coefficients, two launches:
//   k_guided_fit     g = image[0] + image[1] + image[2] and p = the clipped logit in fp64; the box sums B(g), B(p), B(g p),
//                    B(g g) over the window of radius r cut to the map; a = (n Sgp - Sg Sp) / ((n Sgg - Sg Sg) + (eps n) n),
//                    b = (Sp - a Sg) / n, n the window's pixel count from its indices.  [a, b] go to the workspace, fp64 [N,2,Hn,Wn].
//   k_guided_smooth  abar = B(a) / n, bbar = B(b) / n into coeff, fp64 [N,2,Hn,Wn].
//
// Both kernels are one body.  A workgroup of 256 threads owns a TILE of 16 rows x 64 columns of one frame's map:
//   stage       the two source maps of the tile and a halo of r on every side, as fp64, into LDS: up to 32 x 80 values a map
//               (40 KB).  Thread t takes staged elements t, t + 256, ...: consecutive threads, consecutive columns.
//   vertical    V[m][row][col], the sum over the window's rows, ascending from 0.0, for the 16 rows and all 64 + 2r staged columns
//               of TWO maps (20 KB).  Thread t takes (row, col) pairs t, t + 256, ...
//   horizontal  S[m] of a pixel, the sum of V[m] over the window's columns, ascending from 0.0.  Thread t owns column t % 64 of
//               rows t / 64, t / 64 + 4, + 8, + 12: four pixels, whose sums stay in registers.
// The fit runs vertical + horizontal twice over the same stage - first (g, p), then the products (g p, g g), formed as they
// are read - so LDS stays at 60 KB static, under the 64 KB a launch gets without asking, and two workgroups share a CU.  The
// loops run over the window cut to the map: a staged element outside the map is never read and is not written either.
// No workgroup waits for another and there are no atomics; the smooth launch reads the halo of a and b that other workgroups
// of the fit launch wrote, which is why they are two launches.  fp64 adds: 2 r + 1 terms a sum, 4 + 2 sums a pixel and
// phase - about 30 M at 480 x 854 and r = 4, microseconds of the fp64 rate; the launches are the cost.
#include <math.h>

#include "common.hpp"

// the fp64 expressions are the host's, operation for operation
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kTileH = 16, kTileW = 64;
constexpr int kGuidedThreads = 256;
constexpr int kMaxRadius = 8;
constexpr int kStageH = kTileH + 2 * kMaxRadius, kStageW = kTileW + 2 * kMaxRadius;  // 32 x 80
constexpr int kRowsPerThread = kTileH * kTileW / kGuidedThreads;                     // 4
constexpr int kMaxSide = 8192;                                                       // as the stream's scaled entries

struct GuidedGeom {
    int Hn, Wn, r;
    int tiles_x, tiles_y;
};
struct Tile {
    int64_t n;   // frame
    int y0, x0;  // first row and column of the tile
};
__device__ __forceinline__ Tile tile_of(const GuidedGeom &g) {
    Tile t;
    t.x0 = (int)(blockIdx.x % g.tiles_x) * kTileW;
    t.y0 = (int)((blockIdx.x / g.tiles_x) % g.tiles_y) * kTileH;
    t.n = blockIdx.x / ((unsigned)g.tiles_x * g.tiles_y);
    return t;
}

struct Lds {
    double s[2][kStageH * kStageW];  // the two staged maps; element (sy, sx) is map pixel (y0 - r + sy, x0 - r + sx)
    double v[2][kTileH * kStageW];   // their vertical sums; element (ty, sx) is map pixel (y0 + ty, x0 - r + sx)
};

// vertical + horizontal of two maps: PRODUCTS false, the staged maps themselves; true, s0 s1 and s0 s0.  out[k][m] is
// the box sum of map m at the thread's k-th pixel (left as it is where that pixel is outside the map).  Ends behind a barrier:
// lds.v may be written again.
template <bool PRODUCTS>
__device__ __forceinline__ void box_sums(Lds &lds, const GuidedGeom &g, const Tile &t, double (&out)[kRowsPerThread][2]) {
    const int r = g.r, cw = kTileW + 2 * r;
    for (int idx = threadIdx.x; idx < kTileH * cw; idx += kGuidedThreads) {
        const int ty = idx / cw, sx = idx - ty * cw;
        const int y = t.y0 + ty, x = t.x0 - r + sx;
        if (y >= g.Hn || x < 0 || x >= g.Wn) continue;
        const int ya = max(0, y - r), yb = min(g.Hn - 1, y + r);
        double u0 = 0.0, u1 = 0.0;
        for (int yy = ya; yy <= yb; ++yy) {
            const int at = (yy - (t.y0 - r)) * kStageW + sx;
            const double s0 = lds.s[0][at], s1 = lds.s[1][at];
            u0 = u0 + (PRODUCTS ? s0 * s1 : s0);
            u1 = u1 + (PRODUCTS ? s0 * s0 : s1);
        }
        lds.v[0][ty * kStageW + sx] = u0;
        lds.v[1][ty * kStageW + sx] = u1;
    }
    __syncthreads();
    const int tx = threadIdx.x % kTileW, x = t.x0 + tx;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int ty = threadIdx.x / kTileW + (kGuidedThreads / kTileW) * k;
        if (t.y0 + ty >= g.Hn || x >= g.Wn) continue;
        const int xa = max(0, x - r), xb = min(g.Wn - 1, x + r);
        double u0 = 0.0, u1 = 0.0;
        for (int xx = xa; xx <= xb; ++xx) {
            const int at = ty * kStageW + (xx - (t.x0 - r));
            u0 = u0 + lds.v[0][at];
            u1 = u1 + lds.v[1][at];
        }
        out[k][0] = u0, out[k][1] = u1;
    }
    __syncthreads();
}
// n of pixel (y, x): the product of the window's two extents
__device__ __forceinline__ double window_count(int y, int x, const GuidedGeom &g) {
    const int ny = min(g.Hn - 1, y + g.r) - max(0, y - g.r) + 1, nx = min(g.Wn - 1, x + g.r) - max(0, x - g.r) + 1;
    return (double)(ny * nx);
}
// the staged element idx of the loop every thread runs: its place in the stage, and whether it is a pixel of the map
__device__ __forceinline__ bool staged_pixel(int idx, const GuidedGeom &g, const Tile &t, int &at, int &y, int &x) {
    const int cw = kTileW + 2 * g.r;
    const int sy = idx / cw, sx = idx - sy * cw;
    y = t.y0 - g.r + sy, x = t.x0 - g.r + sx;
    at = sy * kStageW + sx;
    return y >= 0 && y < g.Hn && x >= 0 && x < g.Wn;
}

__global__ __launch_bounds__(kGuidedThreads) void k_guided_fit(const float *__restrict__ image, const float *__restrict__ logits,
                                                               double *__restrict__ ab, GuidedGeom g, double eps, double clip) {
    __shared__ Lds lds;
    const Tile t = tile_of(g);
    const int64_t plane = (int64_t)g.Hn * g.Wn;
    const float *__restrict__ im = image + t.n * 3 * plane;
    const float *__restrict__ lg = logits + t.n * plane;
    const int staged = (kTileH + 2 * g.r) * (kTileW + 2 * g.r);
    for (int idx = threadIdx.x; idx < staged; idx += kGuidedThreads) {
        int at, y, x;
        if (!staged_pixel(idx, g, t, at, y, x)) continue;
        const int64_t px = (int64_t)y * g.Wn + x;
        lds.s[0][at] = ((double)im[px] + (double)im[plane + px]) + (double)im[2 * plane + px];
        const double v = (double)lg[px];
        const double p = v >= -clip ? v : -clip;  // a NaN compares false: -clip
        lds.s[1][at] = p <= clip ? p : clip;
    }
    __syncthreads();
    double s[kRowsPerThread][2], q[kRowsPerThread][2];
    box_sums<false>(lds, g, t, s);  // Sg, Sp
    box_sums<true>(lds, g, t, q);   // Sgp, Sgg
    const int tx = threadIdx.x % kTileW, x = t.x0 + tx;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int y = t.y0 + threadIdx.x / kTileW + (kGuidedThreads / kTileW) * k;
        if (y >= g.Hn || x >= g.Wn) continue;
        const double n = window_count(y, x, g);
        const double sg = s[k][0], sp = s[k][1], sgp = q[k][0], sgg = q[k][1];
        const double num = n * sgp - sg * sp;
        const double den = (n * sgg - sg * sg) + (eps * n) * n;
        const double a = num / den;
        const double b = (sp - a * sg) / n;
        const int64_t px = (int64_t)y * g.Wn + x;
        ab[t.n * 2 * plane + px] = a;
        ab[(t.n * 2 + 1) * plane + px] = b;
    }
}

__global__ __launch_bounds__(kGuidedThreads) void k_guided_smooth(const double *__restrict__ ab, double *__restrict__ coeff,
                                                                  GuidedGeom g) {
    __shared__ Lds lds;
    const Tile t = tile_of(g);
    const int64_t plane = (int64_t)g.Hn * g.Wn;
    const double *__restrict__ src = ab + t.n * 2 * plane;
    const int staged = (kTileH + 2 * g.r) * (kTileW + 2 * g.r);
    for (int idx = threadIdx.x; idx < staged; idx += kGuidedThreads) {
        int at, y, x;
        if (!staged_pixel(idx, g, t, at, y, x)) continue;
        const int64_t px = (int64_t)y * g.Wn + x;
        lds.s[0][at] = src[px];
        lds.s[1][at] = src[plane + px];
    }
    __syncthreads();
    double s[kRowsPerThread][2];
    box_sums<false>(lds, g, t, s);
    const int tx = threadIdx.x % kTileW, x = t.x0 + tx;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int y = t.y0 + threadIdx.x / kTileW + (kGuidedThreads / kTileW) * k;
        if (y >= g.Hn || x >= g.Wn) continue;
        const double n = window_count(y, x, g);
        const int64_t px = (int64_t)y * g.Wn + x;
        coeff[t.n * 2 * plane + px] = s[k][0] / n;
        coeff[(t.n * 2 + 1) * plane + px] = s[k][1] / n;
    }
}
}  // namespace

extern "C" size_t fosvos_guided_coefficients_workspace_bytes(int N, int Hn, int Wn) {
    if (N <= 0 || Hn <= 0 || Wn <= 0 || Hn > kMaxSide || Wn > kMaxSide) return 0;
    return (size_t)N * 2 * Hn * Wn * sizeof(double);
}

extern "C" int fosvos_guided_coefficients(const float *image, const float *logits, int N, int Hn, int Wn, int radius, double eps,
                                          double clip, double *coeff, void *workspace, size_t workspace_bytes, int device,
                                          void *stream) {
    FOSVOS_REQUIRE(image && logits && coeff && workspace, FOSVOS_E_ARG, "guided_coefficients: null pointer");
    FOSVOS_REQUIRE(N > 0 && Hn > 0 && Wn > 0 && Hn <= kMaxSide && Wn <= kMaxSide, FOSVOS_E_SHAPE,
                   "guided_coefficients: N=%d, maps of %dx%d (sides of 1..%d)", N, Hn, Wn, kMaxSide);
    FOSVOS_REQUIRE(radius >= 1 && radius <= kMaxRadius, FOSVOS_E_ARG, "guided_coefficients: radius %d outside [1, %d]", radius,
                   kMaxRadius);
    FOSVOS_REQUIRE(eps >= 1e-3 && eps <= 1e9, FOSVOS_E_ARG, "guided_coefficients: eps %g outside [1e-3, 1e9]", eps);
    FOSVOS_REQUIRE(clip > 0.0 && clip <= 1e4, FOSVOS_E_ARG, "guided_coefficients: clip %g outside (0, 1e4]", clip);
    FOSVOS_REQUIRE((((uintptr_t)image | (uintptr_t)logits) & 3) == 0, FOSVOS_E_ARG,
                   "guided_coefficients: the image and the logits must be 4-byte aligned");
    FOSVOS_REQUIRE((((uintptr_t)coeff | (uintptr_t)workspace) & 7) == 0, FOSVOS_E_ARG,
                   "guided_coefficients: the coefficients and the workspace must be 8-byte aligned");
    FOSVOS_REQUIRE(workspace_bytes >= fosvos_guided_coefficients_workspace_bytes(N, Hn, Wn), FOSVOS_E_ARG,
                   "guided_coefficients: workspace of %zu bytes, need %zu", workspace_bytes,
                   fosvos_guided_coefficients_workspace_bytes(N, Hn, Wn));
    GuidedGeom g = {Hn, Wn, radius, (int)cdiv(Wn, kTileW), (int)cdiv(Hn, kTileH)};
    const int64_t blocks = (int64_t)N * g.tiles_x * g.tiles_y;
    FOSVOS_REQUIRE(blocks < ((int64_t)1 << 31), FOSVOS_E_SHAPE, "guided_coefficients: %lld workgroups", (long long)blocks);
    FOSVOS_ENTER(device);
    double *ab = static_cast<double *>(workspace);
    FOSVOS_PROF("k_guided_fit", stream, 0.0);
    hipLaunchKernelGGL(k_guided_fit, dim3((unsigned)blocks), dim3(kGuidedThreads), 0, (hipStream_t)stream, image, logits, ab, g, eps,
                       clip);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_guided_smooth", stream, 0.0);
    hipLaunchKernelGGL(k_guided_smooth, dim3((unsigned)blocks), dim3(kGuidedThreads), 0, (hipStream_t)stream, ab, coeff, g);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
