// Cleaning a mask by its shape on the device: the 8-connected components of `logits >= 0`, the small ones dropped, the
// largest kept, or only those near a seed (the mask kept in the frame before).  The reference has no such step; the bytes are
// the ones util/mask_components.py states in numpy, and every comparison with it is exact equality.
//
// All of it is integer work combined by min, max, or and add, so no result depends on the order workgroups arrive in.  A
// component's label is the smallest raster index y * W + x of its pixels ("root"); the label word of a pixel always holds the
// index of a pixel of its own component that is not larger than its own, so following labels ("find") walks strictly
// decreasing indices and ends at a word that holds its own index.
//
// Stages, each its own launch, ordered by the stream; no kernel waits for another workgroup:
//   k_cc_seed_pack   seed bytes -> the 64-pixel-a-word bit plane S (as k_jf_pack of eval.hip packs its planes); zeroes the
//                    frame's flag "the seed has a pixel"
//   k_cc_dilate      S -> D, the plane dilated by the disk of `radius`: the union over dy of the row's word spread left and
//                    right by floor(sqrt(r*r - dy*dy)) (the method k_jf_count of eval.hip documents), one thread a word.  A
//                    workgroup that read a set bit of S ORs the frame's flag, so "the seed is empty" never reaches the host
//   k_cc_label_tile  (a) a workgroup labels a tile of 16 rows x 64 columns in LDS.  A wave owns a row of the tile: __ballot
//                    gives the row's 64-bit mask, a pixel starts with the label of the first pixel of its horizontal run, and
//                    only the first pixel of a run (and a pixel whose upper neighbour is clear) unites with the row above -
//                    N, or NW and NE where N is clear - by find + atomicMin on LDS words.  After a barrier every pixel
//                    resolves its tile-local root, the tile counts each local root's pixels (and ORs bit 31 where one lies
//                    inside D) in LDS, and writes label[p] = the raster index of the local root, area[p] = that count at a
//                    local root and 0 elsewhere.  The frame's first tile zeroes its `largest` key.
//   k_cc_seams       (b) one thread per pixel of a tile's first row (below the first tile row) and first column (right of the
//                    first tile column) unites it with its neighbours across the border, the diagonals across tile corners
//                    included.  Global memory, find + atomicMin.
//   k_cc_flatten     (c) every foreground pixel resolves its root and stores it; a tile-local root that is not the
//                    component's root adds its count to area[root] and ORs its bit 31 there: one atomic per tile-local
//                    component, not one per pixel.
//   k_cc_largest     (d) (largest only) the root pixel of an eligible component does atomicMax on the frame's 64-bit key
//                    area << 32 | ~root: the largest area, on equal areas the smaller root
//   k_cc_apply       (e) a wave per 64-pixel word: a foreground pixel whose component is not kept becomes `fill`, every other
//                    value passes as the 32 bits it is; the kept bytes; and, in a chain, __ballot(kept) IS the next frame's
//                    seed word (and that frame's flag is zeroed).
//
// Coherence inside a launch (an XCD's L2 does not see another's plain stores before the launch ends): in k_cc_seams and
// k_cc_flatten a label word may be written by any workgroup, so EVERY access to a label word in these two kernels is an
// agent-scope atomic (relaxed load / store, fetch_min), and so is every access to an area word that another workgroup may
// add to (a component's root word: it is only ever the target of fetch_add / fetch_or there, never read).  Nothing is handed
// from one workgroup to another: a stale-free value is not needed, only SOME value the word held, and every value a label
// word ever holds is an index of the same component no larger than the last.  Everything else is read in a later launch than
// it was written in.
#include "common.hpp"

using namespace fosvos;

namespace {
typedef unsigned long long u64;

constexpr int kCcThreads = 256;
constexpr int kCcTileRows = 16, kCcTileCols = 64, kCcTilePixels = kCcTileRows * kCcTileCols;
constexpr int kCcMaxRadius = 63;
constexpr uint32_t kCcTouched = 0x80000000u, kCcAreaMask = 0x7fffffffu;

inline int cc_words(int W) { return (W + 63) / 64; }

#define CC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int g_load(const int32_t *p) { return __hip_atomic_load(p, CC_RLX_AGENT); }

// the root of pixel x's tree: strictly decreasing indices, so at most x steps
__device__ __forceinline__ int g_find(const int32_t *lab, int x) {
    for (int nx = g_load(lab + x); nx != x; nx = g_load(lab + x)) x = nx;
    return x;
}
// unite the trees of a and b: the larger root is hung under the smaller.  Every turn that does not finish lowers a or b
__device__ __forceinline__ void g_union(int32_t *lab, int a, int b) {
    for (;;) {
        a = g_find(lab, a);
        b = g_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(lab + a, b, CC_RLX_AGENT);
        if (old == a) return;
        a = old;  // somebody hung a elsewhere meanwhile (old < a): unite that tree with b's
    }
}

// the same on the LDS words of a tile (workgroup scope)
__device__ __forceinline__ int l_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int l_find(const int *lab, int x) {
    for (int nx = l_load(lab + x); nx != x; nx = l_load(lab + x)) x = nx;
    return x;
}
__device__ __forceinline__ void l_union(int *lab, int a, int b) {
    for (;;) {
        a = l_find(lab, a);
        b = l_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;
    }
}

// ------------------------------------------------------------------------------------------ records, seed
// grid (ceil(H * Wp / 4), frames): one wave packs one word
__global__ __launch_bounds__(kCcThreads) void k_cc_seed_pack(const uint8_t *__restrict__ seed, int H, int W, int Wp,
                                                             u64 *__restrict__ plane, int32_t *__restrict__ any) {
    const int64_t words = (int64_t)H * Wp;
    const int64_t w = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t y = w / Wp;
    const int x = (int)(w - y * Wp) * 64 + lane;
    const bool in = w < words && x < W;
    const uint8_t s = in ? seed[blockIdx.y * ((int64_t)H * W) + y * W + x] : (uint8_t)0;
    const u64 m = __ballot(s != 0);
    if (lane == 0 && w < words) plane[blockIdx.y * words + w] = m;
    if (blockIdx.x == 0 && threadIdx.x == 0) any[blockIdx.y] = 0;  // k_cc_dilate ORs into it, one launch on
}

// OR of (hi:lo) shifted up by 0..h bits (h <= 63), its high word: `m` spread towards higher columns, fed by `below`
__device__ __forceinline__ u64 cc_spread_up(u64 below, u64 m, int h) {
    u64 lo = below, hi = m;
    for (int cover = 0; cover < h;) {
        const int s = min(cover + 1, h - cover);
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
        cover += s;
    }
    return hi;
}
__device__ __forceinline__ u64 cc_spread_down(u64 m, u64 above, int h) {
    u64 lo = m, hi = above;
    for (int cover = 0; cover < h;) {
        const int s = min(cover + 1, h - cover);
        lo |= (lo >> s) | (hi << (64 - s));
        hi |= hi >> s;
        cover += s;
    }
    return lo;
}

// grid (ceil(H * Wp / 256), frames): one thread dilates one word.  A workgroup that saw a set seed pixel ORs the frame's flag:
// one atomic per 256 words (one per word, from the kernels that write the plane, ran one after the other on that one address
// for 90 us a frame)
__global__ __launch_bounds__(kCcThreads) void k_cc_dilate(const u64 *__restrict__ plane, int H, int W, int Wp, int r,
                                                          u64 *__restrict__ out, int32_t *__restrict__ any) {
    __shared__ int half[2 * kCcMaxRadius + 1];  // the disk's half-width at each dy
    for (int i = threadIdx.x; i <= 2 * r; i += kCcThreads) {
        const int dy = i - r, rem = r * r - dy * dy;
        int h = 0;
        while ((h + 1) * (h + 1) <= rem) ++h;
        half[i] = h;
    }
    __syncthreads();
    const int64_t words = (int64_t)H * Wp;
    const int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    plane += blockIdx.y * words;
    out += blockIdx.y * words;
    const int seen = __syncthreads_or(i < words && plane[i] != 0);
    if (threadIdx.x == 0 && seen) __hip_atomic_fetch_or(any + blockIdx.y, 1, CC_RLX_AGENT);
    if (i >= words) return;
    const int y = (int)(i / Wp), c = (int)(i - (int64_t)y * Wp);
    u64 d = 0;
    for (int dy = max(-r, -y); dy <= min(r, H - 1 - y); ++dy) {
        const u64 *row = plane + (int64_t)(y + dy) * Wp + c;
        const u64 m = row[0], left = c > 0 ? row[-1] : 0, right = c + 1 < Wp ? row[1] : 0;
        const int h = half[dy + r];
        d |= cc_spread_up(left, m, h) | cc_spread_down(m, right, h);
    }
    const int nb = W - 64 * c;  // columns of the image in this word
    out[i] = nb >= 64 ? d : d & ((1ull << nb) - 1);
}

// ------------------------------------------------------------------------------------------ (a) a tile in LDS
// grid (tiles_x * tiles_y, frames).  dil, area, key: null for the bare labelling (fosvos_component_roots)
__global__ __launch_bounds__(kCcThreads) void k_cc_label_tile(const float *__restrict__ logits, const u64 *__restrict__ dil,
                                                              int H, int W, int Wp, int tiles_x,
                                                              int32_t *__restrict__ labels, int32_t *__restrict__ area,
                                                              u64 *__restrict__ key) {
    __shared__ int lab[kCcTilePixels];
    __shared__ unsigned cnt[kCcTilePixels];
    __shared__ u64 rowm[kCcTileRows];
    const int64_t hw = (int64_t)H * W;
    logits += blockIdx.y * hw;
    labels += blockIdx.y * hw;
    if (key != nullptr && blockIdx.x == 0 && threadIdx.x == 0) key[blockIdx.y] = 0;  // read by (d), two launches on
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kCcTileRows, x0 = tx * kCcTileCols;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 + lane;
    constexpr int kRows = kCcTileRows / (kCcThreads / 64);  // rows a wave owns: wv, wv + 4, ...
    bool fg[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int ly = wv + 4 * k, y = y0 + ly, i = ly * 64 + lane;
        const bool in = y < H && x < W;
        const float v = in ? logits[(int64_t)y * W + x] : -1.f;
        fg[k] = v >= 0.f;
        const u64 m = __ballot(fg[k]);
        if (lane == 0) rowm[ly] = m;
        const u64 clear_below = ~m & ((1ull << lane) - 1);  // the run starts behind the nearest clear pixel to the left
        const int start = clear_below ? 64 - __clzll(clear_below) : 0;
        lab[i] = fg[k] ? ly * 64 + start : -1;
        cnt[i] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int ly = wv + 4 * k, i = ly * 64 + lane;
        if (fg[k] && ly > 0) {
            const u64 up = rowm[ly - 1], m = rowm[ly];
            const bool w_set = lane > 0 && ((m >> (lane - 1)) & 1);
            const bool n_set = (up >> lane) & 1;
            const bool nw_set = lane > 0 && ((up >> (lane - 1)) & 1), ne_set = lane < 63 && ((up >> (lane + 1)) & 1);
            // a set W neighbour has united the run with N and NW already (N is its NE, NW its N)
            if (n_set) {
                if (!w_set) l_union(lab, i, i - 64);
            } else {
                if (nw_set && !w_set) l_union(lab, i, i - 65);
                if (ne_set) l_union(lab, i, i - 63);
            }
        }
    }
    __syncthreads();
    int root[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int ly = wv + 4 * k, y = y0 + ly, i = ly * 64 + lane;
        root[k] = fg[k] ? l_find(lab, i) : -1;
        if (area != nullptr) {
            const u64 m = rowm[ly];
            const u64 d = (dil != nullptr && y < H) ? dil[blockIdx.y * ((int64_t)H * Wp) + (int64_t)y * Wp + tx] : 0;
            // a row that is one piece of one local component (the usual case inside a blob) counts with one LDS atomic
            const int first = m ? __ffsll((long long)m) - 1 : 0;
            const int r0 = __shfl(root[k], first, 64);
            const bool one = __ballot(fg[k] && root[k] != r0) == 0;
            if (one) {
                if (m && lane == first) {
                    atomicAdd(&cnt[r0], (unsigned)__popcll(m));
                    if (m & d) atomicOr(&cnt[r0], kCcTouched);
                }
            } else if (fg[k]) {
                atomicAdd(&cnt[root[k]], 1u);
                if ((d >> lane) & 1) atomicOr(&cnt[root[k]], kCcTouched);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRows; ++k) {
        const int ly = wv + 4 * k, y = y0 + ly, i = ly * 64 + lane;
        if (y < H && x < W) {
            const int64_t p = (int64_t)y * W + x;
            labels[p] = fg[k] ? (y0 + (root[k] >> 6)) * W + x0 + (root[k] & 63) : -1;
            if (area != nullptr) area[blockIdx.y * hw + p] = (fg[k] && root[k] == i) ? (int32_t)cnt[i] : 0;
        }
    }
}

// ------------------------------------------------------------------------------------------ (b) seams
// grid (ceil((n_h + n_v) / 256), frames): item t < n_h is pixel (16 (t / W + 1), t % W), the others (t' % H, 64 (t' / H + 1))
__global__ __launch_bounds__(kCcThreads) void k_cc_seams(int32_t *__restrict__ labels, int H, int W, int64_t n_h,
                                                         int64_t n_v) {
    labels += blockIdx.y * ((int64_t)H * W);
    int64_t t = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (t < n_h) {
        const int y = (int)(t / W + 1) * kCcTileRows, x = (int)(t % W);
        const int p = y * W + x;
        if (g_load(labels + p) < 0) return;
        const int q = p - W;
        if (g_load(labels + q) >= 0) {  // N set: NW and NE hang on it (inside its tile, or through the vertical seam)
            g_union(labels, p, q);
        } else {
            if (x > 0 && g_load(labels + q - 1) >= 0) g_union(labels, p, q - 1);
            if (x + 1 < W && g_load(labels + q + 1) >= 0) g_union(labels, p, q + 1);
        }
    } else if ((t -= n_h) < n_v) {
        const int x = (int)(t / H + 1) * kCcTileCols, y = (int)(t % H);
        const int p = y * W + x;
        if (g_load(labels + p) < 0) return;
        const int q = p - 1;
        if (g_load(labels + q) >= 0) {  // W set: NW and SW hang on it (inside its tile, or through the horizontal seam)
            g_union(labels, p, q);
        } else {
            if (y > 0 && g_load(labels + q - W) >= 0) g_union(labels, p, q - W);
            if (y + 1 < H && g_load(labels + q + W) >= 0) g_union(labels, p, q + W);
        }
    }
}

// ------------------------------------------------------------------------------------------ (c) flatten
// grid (ceil(H W / 256), frames)
__global__ __launch_bounds__(kCcThreads) void k_cc_flatten(int32_t *__restrict__ labels, int32_t *__restrict__ area,
                                                           int64_t hw) {
    const int64_t p = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (p >= hw) return;
    labels += blockIdx.y * hw;
    const int l = g_load(labels + p);
    if (l < 0) return;
    const int r = g_find(labels, l);
    if (r != l) __hip_atomic_store(labels + p, r, CC_RLX_AGENT);
    if (area != nullptr && r != (int)p) {
        area += blockIdx.y * hw;
        // p is not its component's root, so nobody adds to area[p] in this launch: a plain read of what (a) wrote
        const uint32_t a = (uint32_t)area[p];
        if (a & kCcAreaMask) __hip_atomic_fetch_add(area + r, (int32_t)(a & kCcAreaMask), CC_RLX_AGENT);
        if (a & kCcTouched) __hip_atomic_fetch_or(area + r, (int32_t)kCcTouched, CC_RLX_AGENT);
    }
}

// ------------------------------------------------------------------------------------------ (d), (e)
__device__ __forceinline__ bool cc_eligible(uint32_t a, int min_area, bool gate) {
    return (int)(a & kCcAreaMask) >= min_area && (!gate || (a & kCcTouched));
}

// grid (ceil(H W / 256), frames).  any: the frames' seed flags, null without a seed
__global__ __launch_bounds__(kCcThreads) void k_cc_largest(const int32_t *__restrict__ labels,
                                                           const int32_t *__restrict__ area, int64_t hw, int min_area,
                                                           const int32_t *__restrict__ any, u64 *__restrict__ key) {
    const int64_t p = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (p >= hw) return;
    if (labels[blockIdx.y * hw + p] != (int)p) return;
    const uint32_t a = (uint32_t)area[blockIdx.y * hw + p];
    const bool gate = any != nullptr && any[blockIdx.y] != 0;
    if (cc_eligible(a, min_area, gate))
        __hip_atomic_fetch_max(key + blockIdx.y, ((u64)(a & kCcAreaMask) << 32) | (uint32_t)~(uint32_t)p, CC_RLX_AGENT);
}

// grid (ceil(H * Wp / 4), frames): one wave per word; `out` may be `logits`.  next_plane / next_any: the seed plane and flag of the frame behind
// this one (a chain, one frame a launch), or null
__global__ __launch_bounds__(kCcThreads) void k_cc_apply(const uint32_t *logits, const int32_t *__restrict__ labels,
                                                         const int32_t *__restrict__ area, int H, int W, int Wp, int min_area,
                                                         int largest, const int32_t *__restrict__ any,
                                                         const u64 *__restrict__ key, uint32_t fill_bits,
                                                         uint32_t *out, uint8_t *__restrict__ kept,
                                                         u64 *__restrict__ next_plane, int32_t *__restrict__ next_any) {
    const int64_t words = (int64_t)H * Wp, frame = blockIdx.y * ((int64_t)H * W);
    const int64_t w = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t y = w / Wp;
    const int x = (int)(w - y * Wp) * 64 + lane;
    const bool in = w < words && x < W;
    const int64_t at = frame + y * W + x;
    const uint32_t bits = in ? logits[at] : 0xbf800000u;
    const bool fg = __uint_as_float(bits) >= 0.f;
    bool keep = false;
    if (fg) {
        const int r = labels[at];
        const uint32_t a = (uint32_t)area[frame + r];
        const bool gate = any != nullptr && any[blockIdx.y] != 0;
        keep = cc_eligible(a, min_area, gate);
        if (largest) {
            const u64 k = key[blockIdx.y];
            keep = keep && k != 0 && (uint32_t)~(uint32_t)k == (uint32_t)r;
        }
    }
    if (in) {
        out[at] = (fg && !keep) ? fill_bits : bits;
        if (kept != nullptr) kept[at] = keep ? 1 : 0;
    }
    const u64 m = __ballot(keep);
    if (next_plane != nullptr) {
        if (lane == 0 && w < words) next_plane[blockIdx.y * words + w] = m;
        if (blockIdx.x == 0 && threadIdx.x == 0) next_any[blockIdx.y] = 0;  // the next frame's k_cc_dilate ORs into it
    }
}

// ------------------------------------------------------------------------------------------ host
struct CcGeometry {
    int Wp, tiles_x, tiles_y;
    int64_t hw, words, n_h, n_v;
};
CcGeometry cc_geometry(int H, int W) {
    CcGeometry g;
    g.Wp = cc_words(W);
    g.tiles_x = (int)cdiv(W, kCcTileCols);
    g.tiles_y = (int)cdiv(H, kCcTileRows);
    g.hw = (int64_t)H * W;
    g.words = (int64_t)H * g.Wp;
    g.n_h = (int64_t)(g.tiles_y - 1) * W;
    g.n_v = (int64_t)(g.tiles_x - 1) * H;
    return g;
}

// the workspace: [key u64 N][S u64 N words][D u64 N words][area i32 N hw][labels i32 N hw][any i32 N]
struct CcWorkspace {
    u64 *key, *seed, *dil;
    int32_t *area, *labels, *any;
};
CcWorkspace cc_carve(void *workspace, int N, const CcGeometry &g) {
    CcWorkspace ws;
    ws.key = reinterpret_cast<u64 *>(workspace);
    ws.seed = ws.key + N;
    ws.dil = ws.seed + (int64_t)N * g.words;
    ws.area = reinterpret_cast<int32_t *>(ws.dil + (int64_t)N * g.words);
    ws.labels = ws.area + (int64_t)N * g.hw;
    ws.any = ws.labels + (int64_t)N * g.hw;
    return ws;
}

int cc_check_shape(const char *who, int N, int H, int W) {
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), FOSVOS_E_SHAPE,
                   "%s: N=%d (<= 65535) H=%d W=%d (H W < 2^31)", who, N, H, W);
    return FOSVOS_OK;
}

// stages (a) to (c) on `nf` frames: labels (and area, dil: null for the bare labelling) point at the first of them
int cc_label(const float *logits, const u64 *dil, int nf, int H, int W, const CcGeometry &g, int32_t *labels, int32_t *area,
             u64 *key, hipStream_t st) {
    FOSVOS_PROF("k_cc_label_tile", st, 0.0);
    hipLaunchKernelGGL(k_cc_label_tile, dim3((unsigned)(g.tiles_x * g.tiles_y), (unsigned)nf), dim3(kCcThreads), 0, st, logits,
                       dil, H, W, g.Wp, g.tiles_x, labels, area, key);
    FOSVOS_LAUNCH_CHECK();
    if (g.n_h + g.n_v > 0) {
        FOSVOS_PROF("k_cc_seams", st, 0.0);
        hipLaunchKernelGGL(k_cc_seams, dim3((unsigned)cdiv(g.n_h + g.n_v, kCcThreads), (unsigned)nf), dim3(kCcThreads), 0, st,
                           labels, H, W, g.n_h, g.n_v);
        FOSVOS_LAUNCH_CHECK();
    }
    FOSVOS_PROF("k_cc_flatten", st, 0.0);
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)cdiv(g.hw, kCcThreads), (unsigned)nf), dim3(kCcThreads), 0, st, labels, area,
                       g.hw);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
}  // namespace

extern "C" size_t fosvos_components_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || N > 65535 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return 0;
    const CcGeometry g = cc_geometry(H, W);
    return (size_t)N * (sizeof(u64) + 2 * (size_t)g.words * sizeof(u64) + 2 * (size_t)g.hw * sizeof(int32_t) + sizeof(int32_t));
}

extern "C" int fosvos_component_roots(const float *logits, int N, int H, int W, int32_t *roots, void *workspace,
                                      size_t workspace_bytes, int device, void *stream) {
    (void)workspace;  // the labels live in `roots` itself: nothing else is needed
    (void)workspace_bytes;
    FOSVOS_REQUIRE(logits && roots, FOSVOS_E_ARG, "component_roots: null pointer");
    if (int rc = cc_check_shape("component_roots", N, H, W)) return rc;
    FOSVOS_ENTER(device);
    return cc_label(logits, nullptr, N, H, W, cc_geometry(H, W), roots, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int fosvos_clean_components(const float *logits, const uint8_t *seed, int N, int H, int W, int radius,
                                       int min_area, int largest, int chain, float fill, float *out_logits, uint8_t *kept,
                                       void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(logits && out_logits && workspace, FOSVOS_E_ARG, "clean_components: null pointer");
    if (int rc = cc_check_shape("clean_components", N, H, W)) return rc;
    FOSVOS_REQUIRE(radius >= 0 && radius <= kCcMaxRadius, FOSVOS_E_ARG, "clean_components: radius %d outside [0, %d]", radius,
                   kCcMaxRadius);
    FOSVOS_REQUIRE(min_area >= 0, FOSVOS_E_ARG, "clean_components: min_area %d < 0", min_area);
    uint32_t fill_bits;
    memcpy(&fill_bits, &fill, sizeof(fill_bits));
    // finite (exponent not all ones) and negative; -0.0 is not < 0
    FOSVOS_REQUIRE((fill_bits & 0x7f800000u) != 0x7f800000u && fill < 0.f, FOSVOS_E_ARG,
                   "clean_components: fill must be finite and negative, got %g", (double)fill);
    FOSVOS_REQUIRE(((uintptr_t)workspace & 7) == 0, FOSVOS_E_ARG, "clean_components: the workspace must be 8-byte aligned");
    const size_t need = fosvos_components_workspace_bytes(N, H, W);
    FOSVOS_REQUIRE(workspace_bytes >= need, FOSVOS_E_WORKSPACE, "clean_components: workspace %zu B < %zu B", workspace_bytes,
                   need);
    FOSVOS_ENTER(device);
    const CcGeometry g = cc_geometry(H, W);
    const CcWorkspace ws = cc_carve(workspace, N, g);
    hipStream_t st = (hipStream_t)stream;
    largest = largest != 0;
    // a chain runs its frames one after the other (frame n's seed plane is written by frame n - 1's apply); without one
    // all N frames go through every stage together
    const int nf = chain ? 1 : N, seed_frames = seed == nullptr ? 0 : nf;
    if (seed_frames) {
        FOSVOS_PROF("k_cc_seed_pack", st, 0.0);
        hipLaunchKernelGGL(k_cc_seed_pack, dim3((unsigned)cdiv(g.words, kCcThreads / 64), (unsigned)seed_frames),
                           dim3(kCcThreads), 0, st, seed, H, W, g.Wp, ws.seed, ws.any);
        FOSVOS_LAUNCH_CHECK();
    }
    for (int n0 = 0; n0 < N; n0 += nf) {
        const bool seeded = seed != nullptr || n0 > 0;
        const int64_t px = (int64_t)n0 * g.hw, wd = (int64_t)n0 * g.words;
        if (seeded) {
            FOSVOS_PROF("k_cc_dilate", st, 0.0);
            hipLaunchKernelGGL(k_cc_dilate, dim3((unsigned)cdiv(g.words, kCcThreads), (unsigned)nf), dim3(kCcThreads), 0, st,
                               ws.seed + wd, H, W, g.Wp, radius, ws.dil + wd, ws.any + n0);
            FOSVOS_LAUNCH_CHECK();
        }
        if (int rc = cc_label(logits + px, seeded ? ws.dil + wd : nullptr, nf, H, W, g, ws.labels + px, ws.area + px,
                              largest ? ws.key + n0 : nullptr, st))
            return rc;
        const int32_t *any = seeded ? ws.any + n0 : nullptr;
        if (largest) {
            FOSVOS_PROF("k_cc_largest", st, 0.0);
            hipLaunchKernelGGL(k_cc_largest, dim3((unsigned)cdiv(g.hw, kCcThreads), (unsigned)nf), dim3(kCcThreads), 0, st,
                               ws.labels + px, ws.area + px, g.hw, min_area, any, ws.key + n0);
            FOSVOS_LAUNCH_CHECK();
        }
        const bool next = chain && n0 + 1 < N;
        FOSVOS_PROF("k_cc_apply", st, 0.0);
        hipLaunchKernelGGL(k_cc_apply, dim3((unsigned)cdiv(g.words, kCcThreads / 64), (unsigned)nf), dim3(kCcThreads), 0, st,
                           reinterpret_cast<const uint32_t *>(logits + px), ws.labels + px, ws.area + px, H, W, g.Wp,
                           min_area, largest, any, ws.key + n0, fill_bits, reinterpret_cast<uint32_t *>(out_logits + px),
                           kept ? kept + px : nullptr, next ? ws.seed + wd + g.words : nullptr,
                           next ? ws.any + n0 + 1 : nullptr);
        FOSVOS_LAUNCH_CHECK();
    }
    return FOSVOS_OK;
}
