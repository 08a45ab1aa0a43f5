// Pseudo-labels for online adaptation on the device: "far from a mask" at large radii, and the labelling of a frame's logits
// against the mask kept in the frame before.  The reference has no such step; the bytes are the ones util/online_adapt.py
// states in numpy (far_from, adapt_labels), and every comparison with it is exact equality.
//
// far_from(mask, d): 1 where every set pixel q is further than d, (py - qy)^2 + (px - qx)^2 > d^2, all in int32.  The
// Euclidean gate separates into two passes:
//   k_gate_cols      one thread a column: g[y][x] = the vertical distance from (y, x) to the nearest set pixel of column x,
//                    saturated at d + 1 (uint16: d <= 4095) - one walk down, one walk up.  A workgroup that saw a set pixel
//                    ORs the frame's flag "the mask has a set pixel" (an agent-scope atomic: another workgroup may write it).
//   k_gate_rows<L>   one workgroup a row: the row of g staged in LDS, then pixel x is NEAR iff some x' with |x - x'| <= d has
//                    (x - x')^2 + g[x']^2 <= d^2 - a window loop that stops at the first hit.  A saturated g can never hit:
//                    (d + 1)^2 > d^2.  L = false writes far = !near as bytes; L = true is the labelling fused behind it:
//                    far (only when the frame's flag is set: an empty core names no negatives) -> negative, else
//                    logit >= pos_logit -> positive, else void, with the three class counts reduced in the workgroup and
//                    added to counts[frame] by one atomic per workgroup and class.
// Nothing waits for another workgroup; the flag and the counts are zeroed by a memset in front of the launches and read (the
// flag) only in a later launch than the one that ORs it.
//
// fosvos_adapt_labels: core = erosion of last_mask by the disk of `erode` = far_from(last_mask, erode, set = clear pixels)
// (two launches, skipped when erode == 0), then the gate of the core at neg_distance with the fused row pass (two launches).
#include "common.hpp"

using namespace fosvos;

namespace {
constexpr int kGateThreads = 256;
constexpr int kGateColThreads = 64;  // the column pass: a wave a workgroup, so that the few waves spread over the CUs
constexpr int kGateBatch = 16;  // rows of a column whose loads the column pass issues together
constexpr int kGateMaxDistance = 4095, kGateMaxSide = 8192, kGateMaxFrames = 65535;

#define GATE_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// grid (ceil(W / 64), frames).  set(q) = (mask[q] != 0) != invert
__global__ __launch_bounds__(kGateColThreads) void k_gate_cols(const uint8_t *__restrict__ mask, int H, int W, int cap, int invert,
                                                             uint16_t *__restrict__ g, int32_t *__restrict__ any) {
    const int x = blockIdx.x * kGateColThreads + threadIdx.x;
    const int64_t frame = (int64_t)blockIdx.y * H * W;
    bool seen = false;
    if (x < W) {
        const uint8_t *m = mask + frame + x;
        uint16_t *gc = g + frame + x;
        // kGateBatch rows a turn: their loads are in flight together (one load a turn left the walk waiting out the memory
        // latency 2 H times: 280 us for a 480 x 854 frame)
        int run = cap;
        for (int y0 = 0; y0 < H; y0 += kGateBatch) {
            uint8_t v[kGateBatch];
#pragma unroll
            for (int j = 0; j < kGateBatch; ++j) v[j] = y0 + j < H ? m[(int64_t)(y0 + j) * W] : (uint8_t)0;
#pragma unroll
            for (int j = 0; j < kGateBatch; ++j) {
                if (y0 + j < H) {
                    const bool set = (v[j] != 0) != (invert != 0);
                    run = set ? 0 : min(run + 1, cap);
                    seen |= set;
                    gc[(int64_t)(y0 + j) * W] = (uint16_t)run;
                }
            }
        }
        run = cap;
        for (int y0 = (H - 1) / kGateBatch * kGateBatch; y0 >= 0; y0 -= kGateBatch) {
            uint16_t down[kGateBatch];  // 0 iff the pixel is set (cap >= 1)
#pragma unroll
            for (int j = 0; j < kGateBatch; ++j) down[j] = y0 + j < H ? gc[(int64_t)(y0 + j) * W] : (uint16_t)0;
#pragma unroll
            for (int j = kGateBatch - 1; j >= 0; --j) {
                if (y0 + j < H) {
                    run = down[j] == 0 ? 0 : min(run + 1, cap);
                    if (run < (int)down[j]) gc[(int64_t)(y0 + j) * W] = (uint16_t)run;
                }
            }
        }
    }
    const int block_seen = __syncthreads_or(seen);
    if (threadIdx.x == 0 && block_seen) __hip_atomic_fetch_or(any + blockIdx.y, 1, GATE_RLX_AGENT);
}

// grid (H, frames).  LABEL = false: out[y][x] = far.  LABEL = true: label / void_px / counts as the head of the file says
template <bool LABEL>
__global__ __launch_bounds__(kGateThreads) void k_gate_rows(const uint16_t *__restrict__ g, int H, int W, int d,
                                                             uint8_t *__restrict__ out, const int32_t *__restrict__ any,
                                                             const float *__restrict__ logits, float pos_logit,
                                                             float *__restrict__ label, uint8_t *__restrict__ void_px,
                                                             int32_t *__restrict__ counts) {
    __shared__ uint16_t row[kGateMaxSide];
    const int64_t at = ((int64_t)blockIdx.y * H + blockIdx.x) * W;
    for (int x = threadIdx.x; x < W; x += kGateThreads) row[x] = g[at + x];
    __syncthreads();
    const int d2 = d * d;
    bool gate_on = true;
    if constexpr (LABEL) gate_on = any[blockIdx.y] != 0;  // written one launch ago
    int n_pos = 0, n_neg = 0, n_void = 0;
    for (int x = threadIdx.x; x < W; x += kGateThreads) {
        bool near = false;
        const int lo = max(0, x - d), hi = min(W - 1, x + d);
        for (int xp = lo; xp <= hi; ++xp) {
            const int dx = x - xp, gy = row[xp];
            if (dx * dx + gy * gy <= d2) {
                near = true;
                break;
            }
        }
        if constexpr (LABEL) {
            const bool far = gate_on && !near;
            const bool pos = !far && logits[at + x] >= pos_logit;  // a NaN is never positive
            label[at + x] = pos ? 1.f : 0.f;
            void_px[at + x] = (far || pos) ? 0 : 1;
            n_neg += far ? 1 : 0;
            n_pos += pos ? 1 : 0;
            n_void += (far || pos) ? 0 : 1;
        } else {
            out[at + x] = near ? 0 : 1;
        }
    }
    if constexpr (LABEL) {
        __shared__ int s_cnt[3][kGateThreads / 64];
        int c[3] = {n_pos, n_neg, n_void};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
            if ((threadIdx.x & 63) == 0) s_cnt[k][threadIdx.x >> 6] = c[k];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const int k = threadIdx.x;
            const int total = s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
            if (total) __hip_atomic_fetch_add(counts + (int64_t)blockIdx.y * 3 + k, total, GATE_RLX_AGENT);
        }
    }
}

// the workspace: [any i32 N, rounded up to 16 B][g u16 N H W, rounded up to 16 B]([core u8 N H W] for the labelling)
inline size_t gate_any_bytes(int N) { return ((size_t)N * sizeof(int32_t) + 15) / 16 * 16; }
inline size_t gate_g_bytes(int N, int H, int W) { return ((size_t)N * H * W * sizeof(uint16_t) + 15) / 16 * 16; }
inline bool gate_shape_ok(int N, int H, int W) {
    return N >= 1 && N <= kGateMaxFrames && H >= 1 && H <= kGateMaxSide && W >= 1 && W <= kGateMaxSide;
}

int gate_check(const char *who, int N, int H, int W, int distance, const char *what) {
    FOSVOS_REQUIRE(gate_shape_ok(N, H, W), FOSVOS_E_SHAPE, "%s: N=%d (1..%d) H=%d W=%d (1..%d)", who, N, kGateMaxFrames, H, W,
                   kGateMaxSide);
    FOSVOS_REQUIRE(distance >= 0 && distance <= kGateMaxDistance, FOSVOS_E_ARG, "%s: %s %d outside [0, %d]", who, what,
                   distance, kGateMaxDistance);
    return FOSVOS_OK;
}

void launch_cols(const uint8_t *mask, int N, int H, int W, int d, int invert, uint16_t *g, int32_t *any, hipStream_t st) {
    hipLaunchKernelGGL(k_gate_cols, dim3((unsigned)cdiv(W, kGateColThreads), (unsigned)N), dim3(kGateColThreads), 0, st, mask, H, W,
                       d + 1, invert, g, any);
}
}  // namespace

extern "C" size_t fosvos_distance_gate_workspace_bytes(int N, int H, int W) {
    return gate_shape_ok(N, H, W) ? gate_any_bytes(N) + gate_g_bytes(N, H, W) : 0;
}

extern "C" size_t fosvos_adapt_labels_workspace_bytes(int N, int H, int W) {
    return gate_shape_ok(N, H, W) ? gate_any_bytes(N) + gate_g_bytes(N, H, W) + (size_t)N * H * W : 0;
}

extern "C" int fosvos_distance_gate(const uint8_t *mask, int N, int H, int W, int distance, int invert, uint8_t *out,
                                    void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(mask && out && workspace, FOSVOS_E_ARG, "distance_gate: null pointer");
    if (int rc = gate_check("distance_gate", N, H, W, distance, "distance")) return rc;
    FOSVOS_REQUIRE(((uintptr_t)workspace & 15) == 0, FOSVOS_E_ARG, "distance_gate: the workspace must be 16-byte aligned");
    const size_t need = fosvos_distance_gate_workspace_bytes(N, H, W);
    FOSVOS_REQUIRE(workspace_bytes >= need, FOSVOS_E_WORKSPACE, "distance_gate: workspace %zu B < %zu B", workspace_bytes, need);
    FOSVOS_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    int32_t *any = reinterpret_cast<int32_t *>(workspace);
    uint16_t *g = reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(workspace) + gate_any_bytes(N));
    FOSVOS_HIP_CHECK(hipMemsetAsync(any, 0, (size_t)N * sizeof(int32_t), st));
    FOSVOS_PROF("k_gate_cols", st, 0.0);
    launch_cols(mask, N, H, W, distance, invert != 0, g, any, st);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_gate_rows", st, 0.0);
    hipLaunchKernelGGL(k_gate_rows<false>, dim3((unsigned)H, (unsigned)N), dim3(kGateThreads), 0, st, (const uint16_t *)g, H, W,
                       distance, out, (const int32_t *)nullptr, (const float *)nullptr, 0.f, (float *)nullptr,
                       (uint8_t *)nullptr, (int32_t *)nullptr);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

extern "C" int fosvos_adapt_labels(const float *logits, const uint8_t *last_mask, int N, int H, int W, float pos_logit,
                                   int neg_distance, int erode, float *label, uint8_t *void_px, int32_t *counts,
                                   void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(logits && last_mask && label && void_px && counts && workspace, FOSVOS_E_ARG, "adapt_labels: null pointer");
    if (int rc = gate_check("adapt_labels", N, H, W, neg_distance, "neg_distance")) return rc;
    FOSVOS_REQUIRE(erode >= 0 && erode <= kGateMaxDistance, FOSVOS_E_ARG, "adapt_labels: erode %d outside [0, %d]", erode,
                   kGateMaxDistance);
    FOSVOS_REQUIRE(pos_logit == pos_logit, FOSVOS_E_ARG, "adapt_labels: pos_logit is NaN");
    FOSVOS_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)label & 3) == 0 &&
                       ((uintptr_t)logits & 3) == 0,
                   FOSVOS_E_ARG, "adapt_labels: the workspace must be 16-byte aligned, counts / label / logits 4-byte");
    const size_t need = fosvos_adapt_labels_workspace_bytes(N, H, W);
    FOSVOS_REQUIRE(workspace_bytes >= need, FOSVOS_E_WORKSPACE, "adapt_labels: workspace %zu B < %zu B", workspace_bytes, need);
    FOSVOS_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    int32_t *any = reinterpret_cast<int32_t *>(workspace);
    uint16_t *g = reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(workspace) + gate_any_bytes(N));
    uint8_t *core = reinterpret_cast<uint8_t *>(g) + gate_g_bytes(N, H, W);
    FOSVOS_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(int32_t), st));
    const uint8_t *gated = last_mask;
    if (erode > 0) {
        FOSVOS_HIP_CHECK(hipMemsetAsync(any, 0, (size_t)N * sizeof(int32_t), st));
        FOSVOS_PROF("k_gate_cols", st, 0.0);
        launch_cols(last_mask, N, H, W, erode, 1, g, any, st);
        FOSVOS_LAUNCH_CHECK();
        FOSVOS_PROF("k_gate_rows", st, 0.0);
        hipLaunchKernelGGL(k_gate_rows<false>, dim3((unsigned)H, (unsigned)N), dim3(kGateThreads), 0, st, (const uint16_t *)g, H,
                           W, erode, core, (const int32_t *)nullptr, (const float *)nullptr, 0.f, (float *)nullptr,
                           (uint8_t *)nullptr, (int32_t *)nullptr);
        FOSVOS_LAUNCH_CHECK();
        gated = core;
    }
    FOSVOS_HIP_CHECK(hipMemsetAsync(any, 0, (size_t)N * sizeof(int32_t), st));
    FOSVOS_PROF("k_gate_cols", st, 0.0);
    launch_cols(gated, N, H, W, neg_distance, 0, g, any, st);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_gate_rows_label", st, 0.0);
    hipLaunchKernelGGL(k_gate_rows<true>, dim3((unsigned)H, (unsigned)N), dim3(kGateThreads), 0, st, (const uint16_t *)g, H, W,
                       neg_distance, (uint8_t *)nullptr, (const int32_t *)any, logits, pos_logit, label, void_px, counts);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
