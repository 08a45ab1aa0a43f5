// Test-time ensemble of the test pass (opt-in): the net sees the frame mirrored and at a few other sizes, and its answers are
// averaged back on the frame's grid.  util/test_ensemble.py states both entries in numpy; every output is compared with it
// bit for bit.
//
// fosvos_ensemble_views, one launch:
//   k_ensemble_views   image fp32 [N,3,H,W] -> up to 8 views fp32 [N,3,h_k,w_k], pointers, sizes and flip bits by value in the
//                      kernel's arguments.  blockIdx.y is the view; blockIdx.x walks the view's rows (plane x row) times the
//                      row's groups.  A view of the frame's size is a (mirrored) copy; any other is the bilinear resampling
//                      of the (mirrored) plane in fp64, rounded to fp32 once.
// fosvos_ensemble_merge, one launch:
//   k_ensemble_merge   V logit maps fp32 [N,1,h_k,w_k] -> fp32 [N,1,H,W].  A thread walks the views in order with its four
//                      sums in fp64: a map of the frame's size is a (reversed) 16-byte load, any other four gathers a pixel
//                      through the taps of the (mirrored) column.
//
// The thread map of both.  A segment is one OUTPUT row; a thread takes one group of it: the head [0, k0) up to the row's first
// 16-byte boundary (k0 = 0..3 floats), or four consecutive pixels from there on - every full group is one aligned 16-byte
// store, the head and the tail are scalar stores.  64 consecutive threads store 1 KiB of a row.  The row's taps are taken once
// per thread (once per view in the merge), the column taps once per pixel.  The sources are gathered (a resampled map) or
// loaded as floats4 at the alignment they have (a same-size map).  No LDS, no workspace, no atomics, nothing waits for
// another workgroup.
//
// The taps (util/frame_resample.taps; n_src samples in, n_dst out, either may be the larger): num = (2x+1) n_src - n_dst,
// i0 = num / (2 n_dst), r = the remainder; num < 0: i0 = 0, r = 0; i0 >= n_src - 1: i0 = n_src - 1, r = 0;
// i1 = min(i0 + 1, n_src - 1); w0 = 2 n_dst - r, w1 = r.  With sides of at most 8192 num stays below 2^27.

#include "common.hpp"

// the fp64 expressions are the host's, operation for operation
#pragma clang fp contract(off)

using namespace fosvos;

namespace {
constexpr int kEnsembleThreads = 256;
constexpr int kMaxViews = FOSVOS_ENSEMBLE_MAX_VIEWS;
constexpr int kMaxSide = 8192;

// 16 bytes at the alignment the data has, not the one a float4 would promise
struct __attribute__((packed, aligned(4))) floats4 {
    float v[4];
};

template <typename T>
struct ViewTable {
    T *p[kMaxViews];
    int h[kMaxViews], w[kMaxViews];
    uint32_t flip;  // bit k: view k is mirrored along W
};

struct Tap {
    int i0, i1;
    double w0, w1;
};
__device__ __forceinline__ Tap tap_at(int x, int n_src, int n_dst) {
    const int num = (2 * x + 1) * n_src - n_dst;
    int i0 = 0, r = 0;
    if (num >= 0) {
        i0 = num / (2 * n_dst);
        r = num - i0 * (2 * n_dst);
    }
    if (i0 >= n_src - 1) i0 = n_src - 1, r = 0;
    Tap t;
    t.i0 = i0;
    t.i1 = min(i0 + 1, n_src - 1);
    t.w0 = (double)(2 * n_dst - r);
    t.w1 = (double)r;
    return t;
}
// the resampled value of the output pixel whose column taps are tx (columns c0, c1 of the rows a0, a1), in the host's order
__device__ __forceinline__ double resampled(const float *__restrict__ a0, const float *__restrict__ a1, int c0, int c1,
                                            const Tap &tx, const Tap &ty, double norm) {
    const double top = (double)a0[c0] * tx.w0 + (double)a0[c1] * tx.w1;
    const double bot = (double)a1[c0] * tx.w0 + (double)a1[c1] * tx.w1;
    const double v = top * ty.w0 + bot * ty.w1;
    return v / norm;
}

// the group of thread slot `j` in a row of `w` floats that starts at `row`: pixels [qa, qb)
struct Group {
    int qa, qb;
};
__device__ __forceinline__ Group group_of(int j, int w, const float *row) {
    const int k0 = (int)((16u - ((unsigned)(uintptr_t)row & 15u)) & 15u) >> 2;  // floats up to the 16-byte boundary
    Group g;
    if (j == 0) {
        g.qa = 0;
        g.qb = min(k0, w);
    } else {
        g.qa = min(k0 + 4 * (j - 1), w);
        g.qb = min(g.qa + 4, w);
    }
    return g;
}
__host__ __device__ __forceinline__ int64_t slots_of(int w) { return w / 4 + 2; }

// four floats of a same-size row for the output pixels q .. q + 3: columns q .. q + 3, or mirrored W - 1 - q down
__device__ __forceinline__ void load_same(const float *__restrict__ row, int q, int W, bool flip, float (&v)[4]) {
    const floats4 t = *reinterpret_cast<const floats4 *>(row + (flip ? W - 4 - q : q));
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = t.v[flip ? 3 - i : i];
}
__device__ __forceinline__ void store_group(float *__restrict__ row, const Group &g, const float (&v)[4]) {
    float *at = row + g.qa;
    if (g.qb - g.qa == 4 && ((uintptr_t)at & 15u) == 0) {
        *reinterpret_cast<float4 *>(at) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (g.qa + i < g.qb) at[i] = v[i];
}

__global__ __launch_bounds__(kEnsembleThreads) void k_ensemble_views(const float *__restrict__ image,
                                                                      const ViewTable<float> views, int planes, int H, int W) {
    const int k = blockIdx.y;
    const int hs = views.h[k], ws = views.w[k];
    const bool flip = (views.flip >> k) & 1u;
    const int64_t slots = slots_of(ws);
    const int64_t gid = (int64_t)blockIdx.x * kEnsembleThreads + threadIdx.x;
    if (gid >= (int64_t)planes * hs * slots) return;
    const int64_t seg = gid / slots;
    const int64_t plane = seg / hs;
    const int y = (int)(seg - plane * hs);
    float *__restrict__ row = views.p[k] + seg * ws;
    const Group g = group_of((int)(gid - seg * slots), ws, row);
    if (g.qa >= g.qb) return;
    const float *__restrict__ src = image + plane * H * W;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (hs == H && ws == W) {
        const float *__restrict__ a = src + (int64_t)y * W;
        if (g.qb - g.qa == 4) {
            load_same(a, g.qa, W, flip, v);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (g.qa + i < g.qb) v[i] = a[flip ? W - 1 - (g.qa + i) : g.qa + i];
        }
    } else {
        const Tap ty = tap_at(y, H, hs);
        const float *__restrict__ a0 = src + (int64_t)ty.i0 * W;
        const float *__restrict__ a1 = src + (int64_t)ty.i1 * W;
        const double norm = (double)(4 * hs * ws);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (g.qa + i < g.qb) {
                const Tap tx = tap_at(g.qa + i, W, ws);
                v[i] = (float)resampled(a0, a1, flip ? W - 1 - tx.i0 : tx.i0, flip ? W - 1 - tx.i1 : tx.i1, tx, ty, norm);
            }
        }
    }
    store_group(row, g, v);
}

__global__ __launch_bounds__(kEnsembleThreads) void k_ensemble_merge(const ViewTable<const float> views, int V, int N, int H,
                                                                      int W, float *__restrict__ out) {
    const int64_t slots = slots_of(W);
    const int64_t gid = (int64_t)blockIdx.x * kEnsembleThreads + threadIdx.x;
    if (gid >= (int64_t)N * H * slots) return;
    const int64_t seg = gid / slots;
    const int64_t n = seg / H;
    const int y = (int)(seg - n * H);
    float *__restrict__ row = out + seg * W;
    const Group g = group_of((int)(gid - seg * slots), W, row);
    if (g.qa >= g.qb) return;
    const bool full = g.qb - g.qa == 4;
    const double norm = (double)(4 * H * W);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < V; ++k) {
        const int hk = views.h[k], wk = views.w[k];
        const bool flip = (views.flip >> k) & 1u;
        const float *__restrict__ map = views.p[k] + n * hk * wk;
        double u[4] = {0.0, 0.0, 0.0, 0.0};
        if (hk == H && wk == W) {
            const float *__restrict__ a = map + (int64_t)y * W;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (full) {
                load_same(a, g.qa, W, flip, v);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (g.qa + i < g.qb) v[i] = a[flip ? W - 1 - (g.qa + i) : g.qa + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = (double)v[i];
        } else {
            const Tap ty = tap_at(y, hk, H);
            const float *__restrict__ a0 = map + (int64_t)ty.i0 * wk;
            const float *__restrict__ a1 = map + (int64_t)ty.i1 * wk;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (g.qa + i < g.qb) {
                    const int x = g.qa + i;
                    const Tap tx = tap_at(flip ? W - 1 - x : x, wk, W);  // mirrored back: the output column reads its twin
                    u[i] = resampled(a0, a1, tx.i0, tx.i1, tx, ty, norm);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = k == 0 ? u[i] : acc[i] + u[i];  // acc = u_0: a lone -0.0 stays -0.0
    }
    float v[4];
    const double count = (double)V;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)(acc[i] / count);
    store_group(row, g, v);
}

template <typename T>
int fill_table(const char *who, const fosvos_ensemble_view *views, int V, ViewTable<T> &table) {
    FOSVOS_REQUIRE(views != nullptr, FOSVOS_E_ARG, "%s: null pointer", who);
    FOSVOS_REQUIRE(V >= 1 && V <= kMaxViews, FOSVOS_E_ARG, "%s: V=%d outside [1, %d]", who, V, kMaxViews);
    for (int k = 0; k < V; ++k) {
        FOSVOS_REQUIRE(views[k].data != nullptr, FOSVOS_E_ARG, "%s: null view %d", who, k);
        FOSVOS_REQUIRE(views[k].h >= 1 && views[k].h <= kMaxSide && views[k].w >= 1 && views[k].w <= kMaxSide, FOSVOS_E_SHAPE,
                       "%s: view %d is %d x %d, sides outside 1..%d", who, k, views[k].h, views[k].w, kMaxSide);
        table.p[k] = static_cast<T *>(views[k].data);
        table.h[k] = views[k].h, table.w[k] = views[k].w;
        table.flip |= views[k].flip ? 1u << k : 0u;
    }
    return FOSVOS_OK;
}
int check_frame(const char *who, int N, int H, int W) {
    FOSVOS_REQUIRE(N >= 1 && N <= 65535, FOSVOS_E_SHAPE, "%s: N=%d outside 1..65535", who, N);
    FOSVOS_REQUIRE(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, FOSVOS_E_SHAPE, "%s: the frame is %d x %d, sides outside 1..%d",
                   who, H, W, kMaxSide);
    return FOSVOS_OK;
}
}  // namespace

extern "C" int fosvos_ensemble_views(const float *image, int N, int H, int W, const fosvos_ensemble_view *views, int V,
                                     int device, void *stream) {
    FOSVOS_REQUIRE(image != nullptr, FOSVOS_E_ARG, "ensemble_views: null pointer");
    ViewTable<float> table = {};
    if (int rc = fill_table("ensemble_views", views, V, table)) return rc;
    if (int rc = check_frame("ensemble_views", N, H, W)) return rc;
    int64_t threads = 0;
    for (int k = 0; k < V; ++k) threads = std::max(threads, (int64_t)N * 3 * table.h[k] * slots_of(table.w[k]));
    FOSVOS_REQUIRE(threads <= INT32_MAX, FOSVOS_E_SHAPE, "ensemble_views: %lld groups of four pixels in a view, more than 2^31 - 1",
                   (long long)threads);
    FOSVOS_ENTER(device);
    FOSVOS_PROF("k_ensemble_views", stream, 0.0);
    hipLaunchKernelGGL(k_ensemble_views, dim3((unsigned)cdiv(threads, kEnsembleThreads), (unsigned)V), dim3(kEnsembleThreads), 0,
                       (hipStream_t)stream, image, table, N * 3, H, W);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_ensemble_merge(const fosvos_ensemble_view *views, int V, int N, int H, int W, float *out, int device,
                                     void *stream) {
    FOSVOS_REQUIRE(out != nullptr, FOSVOS_E_ARG, "ensemble_merge: null pointer");
    ViewTable<const float> table = {};
    if (int rc = fill_table("ensemble_merge", views, V, table)) return rc;
    if (int rc = check_frame("ensemble_merge", N, H, W)) return rc;
    const int64_t threads = (int64_t)N * H * slots_of(W);
    FOSVOS_REQUIRE(threads <= INT32_MAX, FOSVOS_E_SHAPE, "ensemble_merge: %lld groups of four pixels, more than 2^31 - 1",
                   (long long)threads);
    FOSVOS_ENTER(device);
    FOSVOS_PROF("k_ensemble_merge", stream, 0.0);
    hipLaunchKernelGGL(k_ensemble_merge, dim3((unsigned)cdiv(threads, kEnsembleThreads)), dim3(kEnsembleThreads), 0,
                       (hipStream_t)stream, table, V, N, H, W, out);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
