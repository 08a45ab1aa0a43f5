// Class-balanced BCE-with-logits: loss + gradient, fused (reference: src/layers/osvos_layers.py:17-44).
//
// One loss kernel serves every entry point: k_loss<M> walks M logit maps that share one label batch (M = 1: the plain and the
// per-frame loss; M = 5: the offline objective's four side maps and the fused one).  Three launches:
//   k_count    per-block positive counts            -> ws.count[block] of the frame's first record
//   k_loss<M>  every block re-sums the counts in index order (so all agree bit-for-bit) - or takes them from ext_counts -,
//              then writes each map's grad and per-block fp64 partial sums of its positive / negative losses
//   k_finish   one wave per record sums the partials in index order and writes the fp32 loss
// All sums are fixed-order: results are bitwise reproducible run to run, and a map's result does not depend on M - the
// multi-map loss equals the per-map loss bit for bit because it IS the same code.
//
// HBM-bound.  Algorithmic bytes per pixel: pass 1 reads the label (4 B); pass 2 reads the label once (4 B) and per map reads
// the logit and writes the gradient (8 B) = 16 B/pixel for one map.  M maps of one label cost 4 + (4 + M x 8) B/pixel where
// M one-map losses cost M x 16, in one set of launches instead of M.
//
// The void form (V = true; fosvos_cbce_loss_frames_void, one map): a byte per pixel says "ignored".  k_count<true> counts
// the positives among the valid pixels and the valid pixels, k_loss<1, true> balances the classes over the valid pixels only,
// replaces a void pixel's logit by 0 before any arithmetic (so a NaN there reaches neither a sum nor a gradient) and writes
// +0.0 as its gradient, k_finish<true> divides by the valid count.  V is a template parameter: the plain instantiations
// carry none of this (their two extra kernel arguments are never read), and with an all-zero void map every operation and
// its order are the plain form's, so the results agree bit for bit.  One more byte a pixel in each of the two passes.
#include "common.hpp"

using namespace fosvos;

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kPerThread = 4;

struct Ws {
    unsigned long long count[kMaxBlocks];
    double pos[kMaxBlocks];
    double neg[kMaxBlocks];
};

__device__ __forceinline__ void load4(const float *__restrict__ p, int64_t i, int64_t n, float (&v)[4], float fill) {
    if (i + 3 < n) {
        const float4 t = *reinterpret_cast<const float4 *>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (i + j < n) ? p[i + j] : fill;
    }
}

// the void bytes of four pixels as "valid" flags (outside the frame: not valid)
__device__ __forceinline__ void load4_valid(const uint8_t *__restrict__ p, int64_t i, int64_t n, bool (&ok)[4]) {
    if (i + 3 < n) {
        const uint32_t t = *reinterpret_cast<const uint32_t *>(p + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = ((t >> (8 * j)) & 0xffu) == 0;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = (i + j < n) && p[i + j] == 0;
    }
}

// one pixel: its loss term and its gradient
__device__ __forceinline__ float px_loss_grad(float xx, bool y, float w_pos, float w_neg, float &g) {
    const float e = expf(-fabsf(xx));          // in (0,1]
    const float l = fmaxf(xx, 0.f) - (y ? xx : 0.f) + log1pf(e);
    const float inv = 1.f / (1.f + e);
    const float sig = xx >= 0.f ? inv : e * inv;
    g = y ? w_pos * (sig - 1.f) : w_neg * sig;
    return l;
}

// blockIdx.y = frame: every frame of a batch is its own loss (own class counts, own workspace record, own output)
// (ws_stride: records per frame = the number of maps of k_loss; a frame keeps its counts in its first record)
// V: void_px [frames][n] bytes, non-zero = ignored; count[] then holds the valid positives, valid[frame][block] the valid pixels
template <bool V>
__global__ __launch_bounds__(kBlock) void k_count(const float *__restrict__ label, int64_t n, Ws *ws, int ws_stride,
                                                   const uint8_t *__restrict__ void_px, unsigned long long *valid) {
    label += (int64_t)blockIdx.y * n;
    ws += (int64_t)blockIdx.y * ws_stride;
    unsigned cnt = 0, cnt_valid = 0;
    if constexpr (V) void_px += (int64_t)blockIdx.y * n;
    const int64_t stride = (int64_t)gridDim.x * kBlock * kPerThread;
    for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread; i < n; i += stride) {
        float y[4];
        load4(label, i, n, y, 0.f);
        if constexpr (V) {
            bool ok[4];
            load4_valid(void_px, i, n, ok);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cnt += (ok[j] && y[j] >= 0.5f) ? 1u : 0u;
                cnt_valid += ok[j] ? 1u : 0u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += (y[j] >= 0.5f) ? 1u : 0u;
        }
    }
    __shared__ unsigned s[kBlock / 64];
    unsigned w = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) ws->count[blockIdx.x] = (unsigned long long)s[0] + s[1] + s[2] + s[3];
    if constexpr (V) {
        __shared__ unsigned sv[kBlock / 64];
        unsigned v = cnt_valid;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0)
            valid[(int64_t)blockIdx.y * kMaxBlocks + blockIdx.x] = (unsigned long long)sv[0] + sv[1] + sv[2] + sv[3];
    }
}

// The logit maps of one launch: separate tensors, so the table travels by value in the kernel arguments (arrays of M: the
// one-map instance carries two pointers and a float).
template <int M>
struct Maps {
    const float *x[M];
    float *grad[M];  // an entry may be null
    float scale[M];  // the factor on map m's gradient
};

// M maps with one label: record blockIdx.y * M + m takes map m's partials, the counts are in the frame's first record
// (k_count with ws_stride = M).  M is a template parameter so that the table is indexed by constants.
// ext_counts (data-parallel batches): {positives, pixels} of the WHOLE batch, counted over all ranks, instead of the workspace's
// V (one map, no ext_counts): the classes are balanced over the valid pixels, see the head of the file
template <int M, bool V>
__global__ __launch_bounds__(kBlock) void k_loss(Maps<M> maps, const float *__restrict__ label, int64_t n, int size_average,
                                                  Ws *ws, int n_count_blocks, const double *__restrict__ ext_counts,
                                                  const uint8_t *__restrict__ void_px,
                                                  const unsigned long long *__restrict__ valid) {
    const int64_t frame_off = (int64_t)blockIdx.y * n;
    label += frame_off;
    ws += (int64_t)blockIdx.y * M;
    __shared__ double s_pos[M][kBlock / 64], s_neg[M][kBlock / 64];
    __shared__ unsigned long long s_np;
    __shared__ unsigned long long s_nv;
    if constexpr (V) {
        void_px += frame_off;
        valid += (int64_t)blockIdx.y * kMaxBlocks;
        __shared__ unsigned long long s_v[kBlock / 64];
        unsigned long long c = 0;
        for (int b = threadIdx.x; b < n_count_blocks; b += kBlock) c += valid[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) s_nv = s_v[0] + s_v[1] + s_v[2] + s_v[3];
    }
    if (!ext_counts) {   // integer sum of the per-block counts: order-independent, so every block agrees exactly
        __shared__ unsigned long long s_c[kBlock / 64];
        unsigned long long c = 0;
        for (int b = threadIdx.x; b < n_count_blocks; b += kBlock) c += ws->count[b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) s_np = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        __syncthreads();
    }
    const double n_tot = V ? (double)s_nv : ext_counts ? ext_counts[1] : (double)n;
    const double n_pos = ext_counts ? ext_counts[0] : (double)s_np;
    const double n_neg = n_tot - n_pos;
    float w_pos[M], w_neg[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        double gscale = (double)maps.scale[m];
        if (size_average) gscale /= n_tot;
        w_pos[m] = (float)(n_neg / n_tot * gscale);  // weight of a positive pixel
        w_neg[m] = (float)(n_pos / n_tot * gscale);
        if constexpr (V) {
            if (!(n_tot > 0.0)) w_pos[m] = w_neg[m] = 0.f;  // every pixel is void: nothing is written but +0.0
        }
    }

    double pos[M], neg[M];
#pragma unroll
    for (int m = 0; m < M; ++m) pos[m] = neg[m] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kBlock * kPerThread;
    for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPerThread; i < n; i += stride) {
        float yv[4], xv[M][4];
        load4(label, i, n, yv, 0.f);
#pragma unroll
        for (int m = 0; m < M; ++m) load4(maps.x[m] + frame_off, i, n, xv[m], 0.f);  // all loads in flight before any store
        bool y[4], ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = yv[j] >= 0.5f;
        if constexpr (V) load4_valid(void_px, i, n, ok);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (V) {
                    // a void pixel's logit is replaced before anything is computed from it
                    const float l = px_loss_grad(ok[j] ? xv[m][j] : 0.f, y[j], w_pos[m], w_neg[m], g[j]);
                    if (ok[j]) {  // (ok implies i + j < n)
                        if (y[j]) pos[m] += (double)l; else neg[m] += (double)l;
                    } else {
                        g[j] = 0.f;
                    }
                } else {
                    const float l = px_loss_grad(xv[m][j], y[j], w_pos[m], w_neg[m], g[j]);
                    if (i + j < n) {
                        if (y[j]) pos[m] += (double)l; else neg[m] += (double)l;
                    }
                }
            }
            if (maps.grad[m]) {
                float *grad = maps.grad[m] + frame_off;
                if (i + 3 < n) {
                    *reinterpret_cast<float4 *>(grad + i) = make_float4(g[0], g[1], g[2], g[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (i + j < n) grad[i + j] = g[j];
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const double p = wave_sum(pos[m]), q = wave_sum(neg[m]);
        if ((threadIdx.x & 63) == 0) {
            s_pos[m][threadIdx.x >> 6] = p;
            s_neg[m][threadIdx.x >> 6] = q;
        }
    }
    __syncthreads();
    if (threadIdx.x < M) {
        const int m = threadIdx.x;
        ws[m].pos[blockIdx.x] = (s_pos[m][0] + s_pos[m][1]) + (s_pos[m][2] + s_pos[m][3]);
        ws[m].neg[blockIdx.x] = (s_neg[m][0] + s_neg[m][1]) + (s_neg[m][2] + s_neg[m][3]);
    }
}

// blockIdx.x = record (frame x map); the class counts are in the first record of the frame
template <bool V>
__global__ __launch_bounds__(64) void k_finish(int64_t n, int size_average, const Ws *ws, int n_blocks,
                                                float *__restrict__ loss_out, const double *__restrict__ ext_counts, int maps,
                                                const unsigned long long *__restrict__ valid) {
    const Ws *ws_count = ws + (blockIdx.x / maps) * maps;
    unsigned long long nv = 0;
    if constexpr (V) {  // (one map a frame: blockIdx.x = frame)
        for (int b = threadIdx.x; b < n_blocks; b += 64) nv += valid[(int64_t)blockIdx.x * kMaxBlocks + b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
    }
    ws += blockIdx.x;
    loss_out += blockIdx.x;
    // lane t sums entries t, t+64, ... then a fixed butterfly: the order never changes run to run
    unsigned long long np = 0;
    double pos = 0.0, neg = 0.0;
    for (int b0 = threadIdx.x; b0 < n_blocks; b0 += 64 * 8) {  // 8 entries in flight (same order of additions)
        unsigned long long c[8];
        double p[8], q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int b = min(b0 + 64 * j, n_blocks - 1);
            c[j] = ext_counts ? 0ull : ws_count->count[b];
            p[j] = ws->pos[b];
            q[j] = ws->neg[b];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (b0 + 64 * j < n_blocks) {
                np += c[j];
                pos += p[j];
                neg += q[j];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o, 64);
    pos = wave_sum(pos);
    neg = wave_sum(neg);
    if (threadIdx.x != 0) return;
    const double n_tot = V ? (double)nv : ext_counts ? ext_counts[1] : (double)n;
    const double n_pos = ext_counts ? ext_counts[0] : (double)np, n_neg = n_tot - n_pos;
    double loss = n_neg / n_tot * pos + n_pos / n_tot * neg;
    if (size_average) loss /= n_tot;
    if constexpr (V) {
        if (!(n_tot > 0.0)) loss = 0.0;
    }
    *loss_out = (float)loss;
}
}  // namespace


extern "C" size_t fosvos_cbce_workspace_bytes(int64_t) { return sizeof(Ws); }

extern "C" size_t fosvos_cbce_multi_workspace_bytes(int64_t, int n_frames, int n_maps) {
    return n_frames > 0 && n_maps > 0 ? (size_t)n_frames * n_maps * sizeof(Ws) : 0;
}

namespace {
typedef Maps<FOSVOS_CBCE_MAX_MAPS> MapTable;  // what an entry point fills; the launch takes its first M entries

template <int M>
void launch_loss(const MapTable &table, const float *label, int64_t numel, int n_frames, int size_average, Ws *ws, int blocks,
                 const double *ext_counts, hipStream_t s) {
    Maps<M> maps;
    for (int m = 0; m < M; ++m) {
        maps.x[m] = table.x[m];
        maps.grad[m] = table.grad[m];
        maps.scale[m] = table.scale[m];
    }
    hipLaunchKernelGGL((k_loss<M, false>), dim3(blocks, n_frames), dim3(kBlock), 0, s, maps, label, numel, size_average, ws,
                       blocks, ext_counts, (const uint8_t *)nullptr, (const unsigned long long *)nullptr);
}

// Every loss entry point: the argument checks (all of them in front of the first launch), then the launches `parts` names
// (FOSVOS_CBCE_COUNT | _LOSS | _FINISH).  who: the entry point, for the messages; loss_label: what the launch profiler calls
// the loss launch; ext_counts: the batch's class counts (null: k_count takes the frames' own).  void_px: null, or the void
// bytes of the one-map void form, whose workspace holds the frames' valid counts behind the records.
int cbce_run(const char *who, const char *loss_label, const MapTable &maps, int n_maps, const float *label, int64_t numel,
             int n_frames, int size_average, const double *ext_counts, float *loss_out, void *workspace,
             size_t workspace_bytes, int parts, int device, void *stream, const uint8_t *void_px = nullptr) {
    FOSVOS_REQUIRE(parts > 0 && parts <= 7, FOSVOS_E_ARG, "%s: parts=%d", who, parts);
    FOSVOS_REQUIRE(n_maps >= 1 && n_maps <= FOSVOS_CBCE_MAX_MAPS, FOSVOS_E_ARG, "%s: n_maps=%d (1..%d)", who, n_maps,
                   FOSVOS_CBCE_MAX_MAPS);
    FOSVOS_REQUIRE(workspace && (label || !(parts & (FOSVOS_CBCE_COUNT | FOSVOS_CBCE_LOSS))) &&
                       (loss_out || !(parts & FOSVOS_CBCE_FINISH)),
                   FOSVOS_E_ARG, "%s: null pointer", who);
    FOSVOS_REQUIRE(numel > 0, FOSVOS_E_SHAPE, "%s: numel=%lld", who, (long long)numel);
    FOSVOS_REQUIRE(n_frames >= 1 && n_frames <= 65535, FOSVOS_E_SHAPE, "%s: n_frames=%d", who, n_frames);
    FOSVOS_REQUIRE(n_frames == 1 || numel % 4 == 0, FOSVOS_E_SHAPE,
                   "%s: %lld elements per frame - frames after the first would start off a 16-byte boundary", who,
                   (long long)numel);
    FOSVOS_REQUIRE(!void_px || (n_maps == 1 && !ext_counts && (uintptr_t)void_px % 4 == 0), FOSVOS_E_ARG,
                   "%s: the void form takes one map, its own counts and void bytes on a 4-byte boundary", who);
    const size_t need = (size_t)n_frames * n_maps * sizeof(Ws) +
                        (void_px ? (size_t)n_frames * kMaxBlocks * sizeof(unsigned long long) : 0);
    FOSVOS_REQUIRE(workspace_bytes >= need, FOSVOS_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    FOSVOS_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)label % 16 == 0, FOSVOS_E_ARG,
                   "%s: label must be 16-byte aligned, the workspace 8-byte", who);
    for (int m = 0; m < n_maps; ++m) {
        FOSVOS_REQUIRE(maps.x[m] || !(parts & FOSVOS_CBCE_LOSS), FOSVOS_E_ARG, "%s: logits[%d] is null", who, m);
        FOSVOS_REQUIRE((uintptr_t)maps.x[m] % 16 == 0 && (uintptr_t)maps.grad[m] % 16 == 0, FOSVOS_E_ARG,
                       "%s: map %d: pointers must be 16-byte aligned", who, m);
    }
    FOSVOS_ENTER(device);
    int blocks = (int)cdiv(numel, (int64_t)kBlock * kPerThread);
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    Ws *ws = reinterpret_cast<Ws *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (void_px) {
        unsigned long long *valid = reinterpret_cast<unsigned long long *>(ws + n_frames);
        FOSVOS_PROF("k_count_void", s, 0.0);
        hipLaunchKernelGGL(k_count<true>, dim3(blocks, n_frames), dim3(kBlock), 0, s, label, numel, ws, 1, void_px, valid);
        FOSVOS_LAUNCH_CHECK();
        Maps<1> one;
        one.x[0] = maps.x[0];
        one.grad[0] = maps.grad[0];
        one.scale[0] = maps.scale[0];
        FOSVOS_PROF(loss_label, s, 0.0);
        hipLaunchKernelGGL((k_loss<1, true>), dim3(blocks, n_frames), dim3(kBlock), 0, s, one, label, numel, size_average, ws,
                           blocks, (const double *)nullptr, void_px, (const unsigned long long *)valid);
        FOSVOS_LAUNCH_CHECK();
        FOSVOS_PROF("k_finish_void", s, 0.0);
        hipLaunchKernelGGL(k_finish<true>, dim3(n_frames), dim3(64), 0, s, numel, size_average, ws, blocks, loss_out,
                           (const double *)nullptr, 1, (const unsigned long long *)valid);
        FOSVOS_LAUNCH_CHECK();
        return FOSVOS_OK;
    }
    if (!ext_counts && (parts & FOSVOS_CBCE_COUNT)) {
        FOSVOS_PROF("k_count", s, 0.0);
        hipLaunchKernelGGL(k_count<false>, dim3(blocks, n_frames), dim3(kBlock), 0, s, label, numel, ws, n_maps,
                           (const uint8_t *)nullptr, (unsigned long long *)nullptr);
        FOSVOS_LAUNCH_CHECK();
    }
    if (parts & FOSVOS_CBCE_LOSS) {
        static constexpr decltype(&launch_loss<1>) launch[FOSVOS_CBCE_MAX_MAPS] = {
            launch_loss<1>, launch_loss<2>, launch_loss<3>, launch_loss<4>,
            launch_loss<5>, launch_loss<6>, launch_loss<7>, launch_loss<8>};
        FOSVOS_PROF(loss_label, s, 0.0);
        launch[n_maps - 1](maps, label, numel, n_frames, size_average, ws, blocks, ext_counts, s);
        FOSVOS_LAUNCH_CHECK();
    }
    if (parts & FOSVOS_CBCE_FINISH) {
        FOSVOS_PROF("k_finish", s, 0.0);
        hipLaunchKernelGGL(k_finish<false>, dim3(n_frames * n_maps), dim3(64), 0, s, numel, size_average, ws, blocks, loss_out,
                           ext_counts, n_maps, (const unsigned long long *)nullptr);
        FOSVOS_LAUNCH_CHECK();
    }
    return FOSVOS_OK;
}

// the one-map entry points: one tensor of logits, one of gradients
int cbce_run1(const char *who, const float *logits, const float *label, int64_t numel, int n_frames, int size_average,
              float grad_scale, const double *ext_counts, float *loss_out, float *grad, void *workspace,
              size_t workspace_bytes, int parts, int device, void *stream) {
    MapTable maps = {};
    maps.x[0] = logits;
    maps.grad[0] = grad;
    maps.scale[0] = grad_scale;
    return cbce_run(who, "k_loss", maps, 1, label, numel, n_frames, size_average, ext_counts, loss_out, workspace,
                    workspace_bytes, parts, device, stream);
}
constexpr int kAllParts = FOSVOS_CBCE_COUNT | FOSVOS_CBCE_LOSS | FOSVOS_CBCE_FINISH;
}  // namespace

extern "C" int fosvos_cbce_loss(const float *logits, const float *label, int64_t numel, int size_average,
                                float grad_scale, float *loss_out, float *grad, void *workspace,
                                size_t workspace_bytes, int device, void *stream) {
    return cbce_run1("cbce_loss", logits, label, numel, 1, size_average, grad_scale, nullptr, loss_out, grad, workspace,
                     workspace_bytes, kAllParts, device, stream);
}

extern "C" int fosvos_cbce_loss_frames(const float *logits, const float *label, int64_t frame_numel, int n_frames,
                                       int size_average, float grad_scale, float *loss_out, float *grad, void *workspace,
                                       size_t workspace_bytes, int device, void *stream) {
    return cbce_run1("cbce_loss_frames", logits, label, frame_numel, n_frames, size_average, grad_scale, nullptr, loss_out,
                     grad, workspace, workspace_bytes, kAllParts, device, stream);
}

extern "C" size_t fosvos_cbce_void_workspace_bytes(int64_t, int n_frames) {
    return n_frames > 0 ? (size_t)n_frames * (sizeof(Ws) + kMaxBlocks * sizeof(unsigned long long)) : 0;
}

extern "C" int fosvos_cbce_loss_frames_void(const float *logits, const float *label, const uint8_t *void_px,
                                            int64_t frame_numel, int n_frames, int size_average, float grad_scale,
                                            float *loss_out, float *grad, void *workspace, size_t workspace_bytes, int device,
                                            void *stream) {
    FOSVOS_REQUIRE(void_px, FOSVOS_E_ARG, "cbce_loss_frames_void: null void map");
    MapTable maps = {};
    maps.x[0] = logits;
    maps.grad[0] = grad;
    maps.scale[0] = grad_scale;
    return cbce_run("cbce_loss_frames_void", "k_loss_void", maps, 1, label, frame_numel, n_frames, size_average, nullptr,
                    loss_out, workspace, workspace_bytes, kAllParts, device, stream, void_px);
}

extern "C" int fosvos_cbce_loss_frames_parts(const float *logits, const float *label, int64_t frame_numel, int n_frames,
                                             int size_average, float grad_scale, float *loss_out, float *grad,
                                             void *workspace, size_t workspace_bytes, int parts, int device, void *stream) {
    return cbce_run1("cbce_loss_frames_parts", logits, label, frame_numel, n_frames, size_average, grad_scale, nullptr,
                     loss_out, grad, workspace, workspace_bytes, parts, device, stream);
}

extern "C" int fosvos_cbce_loss_batch_counts(const float *logits, const float *label, int64_t numel, int size_average,
                                             float grad_scale, const double *batch_counts, float *loss_out,
                                             float *grad, void *workspace, size_t workspace_bytes, int device,
                                             void *stream) {
    FOSVOS_REQUIRE(batch_counts, FOSVOS_E_ARG, "cbce_loss_batch_counts: null batch_counts");
    return cbce_run1("cbce_loss_batch_counts", logits, label, numel, 1, size_average, grad_scale, batch_counts, loss_out,
                     grad, workspace, workspace_bytes, kAllParts, device, stream);
}

extern "C" int fosvos_cbce_loss_frames_multi(const float *const *logits, const float *label, int64_t frame_numel,
                                             int n_frames, int n_maps, int size_average, const float *map_scale,
                                             float *loss_out, float *const *grad, void *workspace, size_t workspace_bytes,
                                             int parts, int device, void *stream) {
    // the only stage that reads the maps is the loss launch: the tables of another stage's call may be absent
    FOSVOS_REQUIRE((logits && map_scale) || !(parts & FOSVOS_CBCE_LOSS), FOSVOS_E_ARG,
                   "cbce_loss_frames_multi: null pointer");
    MapTable maps = {};
    if (parts & FOSVOS_CBCE_LOSS) {
        for (int m = 0; m < n_maps && m < FOSVOS_CBCE_MAX_MAPS; ++m) {
            maps.x[m] = logits[m];
            maps.grad[m] = grad ? grad[m] : nullptr;
            maps.scale[m] = map_scale[m];
        }
    }
    return cbce_run("cbce_loss_frames_multi", "k_loss_multi", maps, n_maps, label, frame_numel, n_frames, size_average,
                    nullptr, loss_out, workspace, workspace_bytes, parts, device, stream);
}
