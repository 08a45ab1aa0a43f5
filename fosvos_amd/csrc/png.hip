// PNG files of the probability bytes, encoded on the device (fosvos_png_encode): uint8 [N,H,W] -> N standalone 8-bit
// greyscale PNG byte streams.  The layout is the one util/png_layout.py states in numpy (the tests compare byte for byte):
//
//   signature | IHDR | IDAT(segment 0) | IDAT(segment 1) | ... | IDAT(final: 03 00 + Adler-32) | IEND
//
// The filtered stream (H rows of filter byte 0 + W pixels) is cut into segments of kSeg = 4096 consecutive bytes.  A segment
// is one fixed-Huffman deflate block (BFINAL = 0) followed by an empty stored block, which pads it to a byte boundary - or,
// where that would be longer, one stored block - in an IDAT chunk of its own, so neither bits nor CRCs cross segments.
// Inside a segment a maximal run of L equal bytes is a literal, then distance-1 matches of 258 while 258 bytes are left,
// then one match of the rest (>= 3) or the rest (1, 2) as literals.
//
// Two launches, one workgroup of 256 threads per segment, 16 consecutive bytes per thread:
//   k_png_measure  token bit count of the segment -> its chunk length (fixed or stored form), and its Adler-32 sums
//                  a = sum(byte), b = sum((n - i) * byte_i), each < 2^32 for n <= 4096 and reduced mod 65521 once
//   k_png_emit     the workgroup finds its place in the file (sum of the chunk lengths in front of it), builds the whole
//                  chunk in LDS - header, bits OR-ed into 32-bit words at their prefix-summed bit offsets, CRC-32 from
//                  per-thread slices combined with x^(8 n) mod P - and copies it out with dword stores (bytes at the two
//                  ragged ends: chunks start at any byte).  One more workgroup per frame writes signature + IHDR,
//                  the Adler-32 combined over all segments, the final IDAT, IEND and the file length.
// Run boundaries across the 256 threads come from a max-scan (start of the run entering a thread's bytes) and a reverse
// min-scan (end of the run leaving them).  LDS: 4 KB segment + 4.1 KB chunk + 1 KB CRC table + scan scratch.
#include "common.hpp"

using namespace fosvos;

namespace {
constexpr int kSeg = 4096, kPngThreads = 256, kPer = kSeg / kPngThreads;  // 16 bytes a thread: one ds_read_b128
constexpr int kChunkWords = (3 + 12 + 2 + 5 + kSeg + 3) / 4 + 1;
constexpr uint32_t kCrcPoly = 0xedb88320u, kAdlerMod = 65521u, kStoredFlag = 0x80000000u;
constexpr int kWsWords = 4;  // per segment: chunk data length | stored flag, adler a, adler b, unused
static_assert(kPer == 16, "a thread reads its bytes as one uint4");

inline int64_t png_stream_bytes(int H, int W) { return (int64_t)H * ((int64_t)W + 1); }
inline int64_t png_segments(int H, int W) { return cdiv(png_stream_bytes(H, W), kSeg); }
inline int64_t png_file_bound(int H, int W) { return 8 + 25 + 2 + png_stream_bytes(H, W) + 17 * png_segments(H, W) + 18 + 12; }

// ---------------------------------------------------------------------------------------- GF(2) arithmetic of CRC-32
// a * b mod P in the reflected representation (x^0 = bit 31)
__device__ __forceinline__ uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 2
    for (int i = 31; i >= 0; --i) {
        p ^= ((a >> i) & 1u) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}
// x^(8 n) mod P; x8[k] = x^(8 * 2^k)
__device__ __forceinline__ uint32_t gf_pow8(uint32_t n, const uint32_t *x8) {
    uint32_t p = 0x80000000u;
    for (int k = 0; n; n >>= 1, ++k)
        if (n & 1u) p = gf_mul(x8[k], p);
    return p;
}
__device__ __forceinline__ uint32_t crc_step(uint32_t c, uint32_t byte, const uint32_t *tab) {
    return tab[(c ^ byte) & 255u] ^ (c >> 8);
}

struct PngShared {
    __attribute__((aligned(16))) uint8_t seg[kSeg];
    __attribute__((aligned(16))) uint32_t chunk[kChunkWords];
    uint32_t crc_tab[256];
    uint32_t x8[16];
    int scan[kPngThreads];
    uint32_t wave[kPngThreads / 64];
    uint8_t small[72];
};

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return wave[0] + wave[1] + wave[2] + wave[3];
}
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t *wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return wave[0] ^ wave[1] ^ wave[2] ^ wave[3];
}
// inclusive scans over the 256 threads (max of ints; sum of uints)
__device__ __forceinline__ int block_scan_max(int v, uint32_t *wave) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v = max(v, u);
    }
    __syncthreads();
    if (lane == 63) wave[wv] = (uint32_t)v;
    __syncthreads();
    for (int i = 0; i < wv; ++i) v = max(v, (int)wave[i]);
    return v;
}
__device__ __forceinline__ uint32_t block_scan_sum(uint32_t v, uint32_t *wave) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();
    if (lane == 63) wave[wv] = v;
    __syncthreads();
    for (int i = 0; i < wv; ++i) v += wave[i];
    return v;
}

// The n bytes of segment `seg` of the filtered stream of one frame -> sh.seg (coalesced byte loads; bytes past n are 0).
__device__ __forceinline__ void load_segment(const uint8_t *__restrict__ img, int W, uint32_t seg, int n, PngShared &sh) {
    // (H * (W + 1) <= 2^30: stream positions, rows and columns fit 32 bits)
    const uint32_t wp = (uint32_t)W + 1u;
    const uint32_t g0 = (uint32_t)seg * kSeg + threadIdx.x;
    uint32_t row = g0 / wp, col = g0 - row * wp;
#pragma unroll 2
    for (int j = 0; j < kPer; ++j) {
        const int i = j * kPngThreads + threadIdx.x;
        uint8_t v = 0;
        if (i < n && col > 0) v = img[(int64_t)row * W + col - 1];
        sh.seg[i] = v;
        col += kPngThreads;
        if (col >= wp) {
            const uint32_t q = col / wp;
            row += q;
            col -= q * wp;
        }
    }
    __syncthreads();
}

// The tokens of this thread's 16 bytes: code[j] / nb[j] = the bits position 16 tid + j adds to the fixed-Huffman block (LSB
// first; 0 bits where a match that started earlier covers the byte).  Returns the thread's bit total.
__device__ __forceinline__ uint32_t thread_tokens(PngShared &sh, int n, uint32_t (&code)[kPer], uint32_t (&nb)[kPer],
                                                  uint32_t (&bytes)[kPer]) {
    const int tid = threadIdx.x, p0 = tid * kPer;
    const uint4 v = *reinterpret_cast<const uint4 *>(sh.seg + p0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t prev = p0 > 0 ? sh.seg[p0 - 1] : 0u;
    uint32_t starts = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        bytes[j] = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        if (p0 + j < n && (p0 + j == 0 || bytes[j] != prev)) starts |= 1u << j;
        prev = bytes[j];
    }
    // the run entering this thread's bytes started at the last start of an earlier thread; the run leaving them ends at
    // the first start of a later thread (or n)
    const int last_start = starts ? p0 + 31 - __clz((int)starts) : -1;
    const int first_start = starts ? p0 + __ffs((int)starts) - 1 : -1;
    const int incl = block_scan_max(last_start, sh.wave);
    sh.scan[tid] = incl;
    __syncthreads();
    int cur_s = tid > 0 ? sh.scan[tid - 1] : 0;
    __syncthreads();
    // reverse min-scan of first_start as a max-scan of its negation over the mirrored thread order
    sh.scan[tid] = first_start < 0 ? -n : -first_start;
    __syncthreads();
    const int mirrored = block_scan_max(sh.scan[kPngThreads - 1 - tid], sh.wave);
    __syncthreads();
    sh.scan[kPngThreads - 1 - tid] = -mirrored;
    __syncthreads();
    const int e_out = tid + 1 < kPngThreads ? sh.scan[tid + 1] : n;
    __syncthreads();

    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = p0 + j;
        // (selects, not branches: sixteen unrolled copies of nested branches cost an exec-mask register pair each)
        const bool in = i < n;
        cur_s = (starts & (1u << j)) ? i : cur_s;
        const uint32_t later = j + 1 < kPer ? starts >> (j + 1) : 0u;
        const int e = later ? i + __ffs((int)later) : e_out;
        const int k = i - cur_s, rem = e - cur_s - 1;
        const int jj = max(k - 1, 0), blk = jj / 258, off = jj - blk * 258, q = rem / 258, r = rem - q * 258;
        const bool in_rem = k > 0 && rem >= 3, full = in_rem && blk < q, tail = in_rem && blk >= q && r >= 3;
        const bool literal = in && !(full || tail);
        const int len = (in && (full || tail) && off == 0) ? (full ? 258 : r) : 0;  // > 0: a match of this length starts here
        const uint32_t b = bytes[j];
        const uint32_t lit_c = b < 144u ? 0x30u + b : 0x190u + b - 144u, lit_bits = b < 144u ? 8u : 9u;
        const uint32_t lm = len >= 3 ? (uint32_t)len - 3u : 0u;
        const uint32_t eb = (lm < 8u || len == 258) ? 0u : 29u - (uint32_t)__clz((int)lm);  // floor(log2(lm)) - 2
        const uint32_t sym = len == 258 ? 285u : (lm < 8u ? 257u + lm : 261u + 4u * eb + ((lm >> eb) & 3u));
        const uint32_t extra = lm & ((1u << eb) - 1u);
        const uint32_t sym_c = sym < 280u ? sym - 256u : 0xC0u + sym - 280u, sym_bits = sym < 280u ? 7u : 8u;
        const uint32_t m_code = (__brev(sym_c) >> (32u - sym_bits)) | (extra << sym_bits);
        code[j] = literal ? __brev(lit_c) >> (32u - lit_bits) : (len ? m_code : 0u);
        nb[j] = literal ? lit_bits : (len ? sym_bits + eb + 5u : 0u);  // (+ the distance code of 1: five zero bits)
        total += nb[j];
    }
    return total;
}

// grid (segments, N)
__global__ __launch_bounds__(kPngThreads) void k_png_measure(const uint8_t *__restrict__ img, int H, int W,
                                                            uint32_t *__restrict__ ws) {
    __shared__ PngShared sh;
    const uint32_t n_total = (uint32_t)H * ((uint32_t)W + 1u), seg = blockIdx.x;
    const int n = (int)min((uint32_t)kSeg, n_total - seg * kSeg);
    img += (int64_t)blockIdx.y * H * W;
    load_segment(img, W, seg, n, sh);
    uint32_t code[kPer], nb[kPer], bytes[kPer];
    const uint32_t bits = block_sum(thread_tokens(sh, n, code, nb, bytes), sh.wave);
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = threadIdx.x * kPer + j;
        if (i < n) {
            a += bytes[j];
            b += (uint32_t)(n - i) * bytes[j];
        }
    }
    a = block_sum(a, sh.wave);
    b = block_sum(b, sh.wave);
    if (threadIdx.x == 0) {
        const uint32_t fixed_len = (3u + bits + 7u + 3u + 7u) / 8u + 4u, stored_len = 5u + (uint32_t)n;
        const bool stored = fixed_len > stored_len;
        uint32_t *rec = ws + ((size_t)blockIdx.y * gridDim.x + seg) * kWsWords;
        rec[0] = ((stored ? stored_len : fixed_len) + (seg == 0 ? 2u : 0u)) | (stored ? kStoredFlag : 0u);
        rec[1] = a % kAdlerMod;
        rec[2] = b % kAdlerMod;
        rec[3] = 0;
    }
}

__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// The parts of a file that belong to no segment, by one workgroup per frame (block n_seg of k_png_emit's grid): signature and
// IHDR; behind the last segment's chunk the final IDAT with the Adler-32 combined over all segments, IEND; the length.
__device__ __forceinline__ void png_frame_ends(PngShared &sh, int H, int W, const uint32_t *__restrict__ ws, uint32_t n_seg,
                                               uint8_t *__restrict__ out, int32_t *__restrict__ length) {
    const int tid = threadIdx.x;
    const uint32_t n_total = (uint32_t)H * ((uint32_t)W + 1u);
    // A = 1 + sum a_s;  B = n_total + sum (b_s + a_s * bytes behind segment s)      (mod 65521)
    uint32_t sa = 0, sb = 0, bytes = 0;
    for (uint32_t s = tid; s < n_seg; s += kPngThreads) {
        const uint32_t a = ws[(size_t)s * kWsWords + 1], b = ws[(size_t)s * kWsWords + 2];
        const uint32_t behind = n_total - min(n_total, (s + 1u) * kSeg);
        bytes += 12u + (ws[(size_t)s * kWsWords] & ~kStoredFlag);
        sa = (sa + a) % kAdlerMod;
        sb = (sb + b + (a * (behind % kAdlerMod)) % kAdlerMod) % kAdlerMod;  // (65520^2 < 2^32)
    }
    sa = block_sum(sa, sh.wave);  // 256 terms below 65521 each
    sb = block_sum(sb, sh.wave);
    const uint32_t end = 33u + block_sum(bytes, sh.wave);  // where the last segment's chunk ends
    if (tid == 0) {
        uint8_t *h = sh.small;
        const uint32_t sig0 = 0x474e5089u, sig1 = 0x0a1a0a0du;  // 89 'P' 'N' 'G' \r \n 1a \n
        for (int i = 0; i < 4; ++i) h[i] = (uint8_t)(sig0 >> (8 * i)), h[4 + i] = (uint8_t)(sig1 >> (8 * i));
        put_be32(h + 8, 13u);
        h[12] = 'I', h[13] = 'H', h[14] = 'D', h[15] = 'R';
        put_be32(h + 16, (uint32_t)W);
        put_be32(h + 20, (uint32_t)H);
        h[24] = 8, h[25] = 0, h[26] = 0, h[27] = 0, h[28] = 0;
        uint32_t c = 0xffffffffu;
        for (int i = 12; i < 29; ++i) c = crc_step(c, h[i], sh.crc_tab);
        put_be32(h + 29, c ^ 0xffffffffu);

        const uint32_t A = (1u + sa) % kAdlerMod, B = (sb + n_total % kAdlerMod) % kAdlerMod;
        uint8_t *t = sh.small + 36;
        put_be32(t, 6u);
        t[4] = 'I', t[5] = 'D', t[6] = 'A', t[7] = 'T';
        t[8] = 0x03, t[9] = 0x00;  // the final, empty fixed-Huffman block
        put_be32(t + 10, (B << 16) | A);
        c = 0xffffffffu;
        for (int i = 4; i < 14; ++i) c = crc_step(c, t[i], sh.crc_tab);
        put_be32(t + 14, c ^ 0xffffffffu);
        put_be32(t + 18, 0u);
        t[22] = 'I', t[23] = 'E', t[24] = 'N', t[25] = 'D';
        put_be32(t + 26, 0xae426082u);
        *length = (int32_t)(end + 30u);
    }
    __syncthreads();
    if (tid < 33) out[tid] = sh.small[tid];
    if (tid >= 64 && tid < 94) out[end + tid - 64] = sh.small[36 + tid - 64];
}

// grid (segments + 1, N)
__global__ __launch_bounds__(kPngThreads) void k_png_emit(const uint8_t *__restrict__ img, int H, int W,
                                                         const uint32_t *__restrict__ ws, uint8_t *__restrict__ out,
                                                         int64_t capacity, int32_t *__restrict__ lengths) {
    __shared__ PngShared sh;
    const int tid = threadIdx.x;
    const uint32_t n_total = (uint32_t)H * ((uint32_t)W + 1u);  // <= 2^30
    const uint32_t seg = blockIdx.x, n_seg = gridDim.x - 1;
    const int n = (int)min((uint32_t)kSeg, n_total - seg * kSeg);
    img += (int64_t)blockIdx.y * H * W;
    ws += (int64_t)blockIdx.y * n_seg * kWsWords;
    out += (int64_t)blockIdx.y * capacity;

    // CRC-32 byte table and the powers x^(8 * 2^k)
    {
        uint32_t c = (uint32_t)tid;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
        sh.crc_tab[tid] = c;
        if (tid < 16) {
            uint32_t p = 0x00800000u;  // x^8
            for (int k = 0; k < tid; ++k) p = gf_mul(p, p);
            sh.x8[tid] = p;
        }
    }
    if (seg == n_seg) {
        __syncthreads();
        png_frame_ends(sh, H, W, ws, n_seg, out, lengths + blockIdx.y);
        return;
    }
    // where this chunk starts: signature + IHDR, then the chunks of the segments in front
    uint32_t before = 0;
    for (uint32_t s = tid; s < seg; s += kPngThreads) before += 12u + (ws[(size_t)s * kWsWords] & ~kStoredFlag);
    const uint32_t offset = 33u + block_sum(before, sh.wave);
    const uint32_t rec0 = ws[(size_t)seg * kWsWords];
    const bool stored = (rec0 & kStoredFlag) != 0;
    const uint32_t dlen = rec0 & ~kStoredFlag, zhdr = seg == 0 ? 2u : 0u;
    uint8_t *dst = out + offset;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);  // the chunk sits at byte `mis` of sh.chunk: dwords line up
    const uint32_t total = 12u + dlen, n_words = (mis + total + 3u) / 4u;
    for (uint32_t i = tid; i < n_words; i += kPngThreads) sh.chunk[i] = 0;

    load_segment(img, W, seg, n, sh);  // (ends in a barrier: tables and zeroes are visible)
    uint32_t code[kPer], nb[kPer], bytes[kPer];
    const uint32_t my_bits = thread_tokens(sh, n, code, nb, bytes);
    const uint32_t bit_end = block_scan_sum(my_bits, sh.wave);

    uint8_t *cb = reinterpret_cast<uint8_t *>(sh.chunk) + mis;  // the chunk's bytes
    uint8_t *data = cb + 8 + zhdr;                              // the segment's deflate bytes
    if (tid == 0) {
        put_be32(cb, dlen);
        cb[4] = 'I', cb[5] = 'D', cb[6] = 'A', cb[7] = 'T';
        if (zhdr) cb[8] = 0x78, cb[9] = 0x01;
        if (stored) {
            data[0] = 0;
            data[1] = (uint8_t)n, data[2] = (uint8_t)(n >> 8);
            data[3] = (uint8_t)~n, data[4] = (uint8_t)(~n >> 8);
        } else {
            cb[8 + dlen - 2] = 0xff, cb[8 + dlen - 1] = 0xff;  // 00 00 FF FF of the empty stored block
        }
    }
    if (stored) {
#pragma unroll
        for (int j = 0; j < kPer; ++j)
            if (tid * kPer + j < n) data[5 + tid * kPer + j] = (uint8_t)bytes[j];
    }
    __syncthreads();
    if (!stored) {
        // the thread's bits, OR-ed into the words they fall in (its first and last word are shared with its neighbours)
        uint32_t pos = 8u * (mis + 8u + zhdr) + 3u + (bit_end - my_bits);
        if (tid == 0) atomicOr(&sh.chunk[(8u * (mis + 8u + zhdr)) >> 5], 2u << ((8u * (mis + 8u + zhdr)) & 31u));  // BFINAL 0, BTYPE 01
        uint32_t word = pos >> 5, fill = pos & 31u;
        unsigned long long acc = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            acc |= (unsigned long long)code[j] << fill;
            fill += nb[j];
            if (fill >= 32u) {
                atomicOr(&sh.chunk[word++], (uint32_t)acc);
                acc >>= 32;
                fill -= 32u;
            }
        }
        if (fill && acc) atomicOr(&sh.chunk[word], (uint32_t)acc);
    }
    __syncthreads();

    // CRC-32 of 'IDAT' + data: raw CRCs of 256 slices, each moved to its place by x^(8 * bytes behind it)
    {
        const uint32_t L = 4u + dlen, m = (L + kPngThreads - 1) / kPngThreads;
        const uint32_t lo = min(L, (uint32_t)tid * m), hi = min(L, lo + m);
        uint32_t raw = 0;
        for (uint32_t i = lo; i < hi; ++i) raw = crc_step(raw, cb[4 + i], sh.crc_tab);
        uint32_t part = hi > lo ? gf_mul(gf_pow8(L - hi, sh.x8), raw) : 0u;
        if (tid == 0) part ^= gf_mul(gf_pow8(L, sh.x8), 0xffffffffu);  // the initial value, carried through L bytes
        const uint32_t crc = block_xor(part, sh.wave) ^ 0xffffffffu;
        if (tid == 0) put_be32(cb + 8 + dlen, crc);
        __syncthreads();
    }

    // out: bytes at the ragged ends, dwords between (never a byte outside [dst, dst + total): neighbours write there)
    {
        uint32_t *dst_w = reinterpret_cast<uint32_t *>(dst - mis);
        const uint8_t *cbytes = reinterpret_cast<const uint8_t *>(sh.chunk);
        const uint32_t end = mis + total;
        const uint32_t first_full = mis ? 1u : 0u, last_full = end / 4u;  // words [first_full, last_full) are whole
        for (uint32_t i = first_full + tid; i < last_full; i += kPngThreads) dst_w[i] = sh.chunk[i];
        if (tid < 4u && mis && tid >= mis && tid < end) dst[tid - mis] = cbytes[tid];
        if (tid < (end & 3u) && last_full >= first_full) {
            const uint32_t i = last_full * 4u + tid;
            if (i >= mis) dst[i - mis] = cbytes[i];
        }
    }

}
}  // namespace

extern "C" size_t fosvos_png_capacity_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)png_file_bound(H, W);
}

extern "C" size_t fosvos_png_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * (size_t)png_segments(H, W) * kWsWords * sizeof(uint32_t);
}

extern "C" int fosvos_png_encode(const uint8_t *bytes, int N, int H, int W, uint8_t *out, size_t capacity, int32_t *lengths,
                                 void *workspace, size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && png_stream_bytes(H, W) <= ((int64_t)1 << 30), FOSVOS_E_SHAPE,
                   "png_encode: N=%d (<= 65535) H=%d W=%d (H * (W + 1) <= 2^30)", N, H, W);
    FOSVOS_REQUIRE(bytes && out && lengths && workspace, FOSVOS_E_ARG, "png_encode: null pointer");
    FOSVOS_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)lengths & 3) == 0, FOSVOS_E_ARG,
                   "png_encode: the workspace and the lengths must be 4-byte aligned");
    const size_t need_cap = fosvos_png_capacity_bytes(N, H, W), need_ws = fosvos_png_workspace_bytes(N, H, W);
    FOSVOS_REQUIRE(capacity >= need_cap, FOSVOS_E_WORKSPACE, "png_encode: capacity %zu B a frame < %zu B", capacity, need_cap);
    FOSVOS_REQUIRE(workspace_bytes >= need_ws, FOSVOS_E_WORKSPACE, "png_encode: workspace %zu B < %zu B", workspace_bytes,
                   need_ws);
    FOSVOS_ENTER(device);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)png_segments(H, W), (unsigned)N);
    uint32_t *ws = reinterpret_cast<uint32_t *>(workspace);
    FOSVOS_PROF("k_png_measure", stream, 0.0);
    hipLaunchKernelGGL(k_png_measure, grid, dim3(kPngThreads), 0, st, bytes, H, W, ws);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF("k_png_emit", stream, 0.0);
    hipLaunchKernelGGL(k_png_emit, dim3(grid.x + 1, grid.y), dim3(kPngThreads), 0, st, bytes, H, W, ws, out, (int64_t)capacity,
                       lengths);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
