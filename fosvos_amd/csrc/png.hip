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
//
// huffman = 1 runs the <true> instantiations of the same two kernels, which add a third form of a
// segment: a dynamic-Huffman block (BTYPE = 10) with a literal/length code fitted to the segment's tokens (png_layout.py
// states it: two-queue Huffman construction over the symbols sorted by (count, symbol), counts halved while the tree is
// deeper than 15, canonical codes, HDIST = 0, a fixed code-length code, zero runs as symbols 17 / 18).
//   measure  histogram of the token symbols (LDS atomics), rank sort by (count << 9 | symbol), the merge by one lane, depths
//            by a walk to the root per leaf; the fitted block's bit count; the shortest of {fitted, fixed, stored} wins
//            (fixed or stored on a tie) and, where it is the fitted one, the 286 lengths go to the workspace
//   emit     canonical codes from the lengths (a ballot per code length gives a symbol's rank among its equals), the
//            header, the code-length sequence (zero runs from a 320-bit mask of the non-zero lengths), the tokens
//            recoded, the end-of-block code; chunk length, CRC and copy-out as for the other forms
//
// fosvos_png_encode_indexed: the same two kernels write the label maps of a multi-object pass as palette files.  k_png_emit takes
// the form of the file's head as a parameter (PngHead): IHDR colour type 3 instead of 0 and, between IHDR and the first IDAT,
// one PLTE chunk of 256 entries whose CRC-32 the frame's last workgroup computes like a segment's; every chunk behind it
// starts 780 bytes later.  fosvos_png_encode passes {0, 33, no palette}: its files are what they were.
#include "common.hpp"

using namespace fosvos;

namespace {
constexpr int kSeg = 4096, kPngThreads = 256, kPer = kSeg / kPngThreads;  // 16 bytes a thread: one ds_read_b128
constexpr int kChunkWords = (3 + 12 + 2 + 5 + kSeg + 3) / 4 + 1;
constexpr uint32_t kCrcPoly = 0xedb88320u, kAdlerMod = 65521u, kStoredFlag = 0x80000000u;
constexpr int kWsWords = 4;  // per segment: chunk data length | stored flag, adler a, adler b, form (fitted mode)
// the fitted form: 286 literal/length symbols (padded to 288: whole dwords), code lengths <= 15 bits; behind the N * S
// records of a fitted-mode workspace come N * S times kLenWords words of code lengths, one byte a symbol
constexpr int kLitLen = 286, kLitPad = 288, kLenWords = kLitPad / 4, kEob = 256, kMaxBits = 15, kZeroRun = 138;
constexpr uint32_t kNoToken = kLitPad - 1;
constexpr uint32_t kFormFixed = 0, kFormStored = 1, kFormFitted = 2;
// code-length code: bits of symbol 0..18 (png_layout.CL_LENGTHS), written in the order of RFC 1951 3.2.7 with HCLEN = 19
constexpr int kClBits[19] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 4, 4};
constexpr int kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr unsigned long long cl_header_bits() {
    unsigned long long v = 0;
    for (int i = 0; i < 19; ++i) v |= (unsigned long long)kClBits[kClOrder[i]] << (3 * i);
    return v;
}
constexpr unsigned long long kClHeader = cl_header_bits();  // the 57 bits behind HLIT, HDIST, HCLEN
constexpr uint32_t kFitHeaderBits = 3 + 5 + 5 + 4 + 57;
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

// The form of a file's head: the IHDR colour type, the bytes in front of the first IDAT chunk (signature 8 + IHDR 25, and for
// an indexed file the PLTE chunk of 12 + 768) and the 256 RGB entries of that chunk (null: no PLTE).
struct PngHead {
    uint32_t color_type, first_idat;
    const uint8_t *palette;
};
constexpr uint32_t kHeadBytes = 33u, kPlteData = 768u, kPlteChunk = 12u + kPlteData;

struct PngShared {
    __attribute__((aligned(16))) uint8_t seg[kSeg];
    __attribute__((aligned(16))) uint32_t chunk[kChunkWords];
    uint32_t crc_tab[256];
    uint32_t x8[16];
    int scan[kPngThreads];
    uint32_t wave[kPngThreads / 64];
    uint8_t small[72];
};

// what the fitted form needs beside PngShared
struct PngFit {
    uint32_t hist[kLitPad];                                // symbol counts
    __attribute__((aligned(16))) uint32_t key[kLitPad];    // count << 9 | symbol; ~0 for an unused symbol
    uint32_t lw[kLitPad], iw[kLitPad];                     // weights: leaves in sorted order, merged nodes in the order made
    uint16_t lpar[kLitPad], ipar[kLitPad], order[kLitPad]; // parents (merged-node numbers); sorted place -> symbol
    uint32_t tab[kLitPad];                                 // emit: code, bit-reversed | length << 16
    __attribute__((aligned(16))) uint8_t len[kLitPad];     // code lengths
    unsigned long long nz[5];                              // bit p: position p of the code-length sequence is not 0
    uint32_t cnt[5][16];                                   // symbols of each length in each 64-symbol chunk
    uint32_t next[16];                                     // first code of each length
    uint32_t deepest;
};

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
// kFitted: tok[j] = the token's literal/length symbol | number of extra bits << 9 | extra bits << 12 | 1 << 17 for a match;
// kNoToken (a padding symbol whose count and code length stay 0) where no token starts.
template <bool kFitted>
__device__ __forceinline__ uint32_t thread_tokens(PngShared &sh, int n, uint32_t (&code)[kPer], uint32_t (&nb)[kPer],
                                                  uint32_t (&bytes)[kPer], uint32_t (&tok)[kPer]) {
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
        if constexpr (kFitted) {
            tok[j] = literal ? b : (len ? sym | (eb << 9) | (extra << 12) | (1u << 17) : kNoToken);
            // (taken here, in a VGPR: left to sink to its use behind the barriers, it keeps sixteen pairs of lane masks alive)
            asm volatile("" : "+v"(tok[j]));
        }
        total += nb[j];
    }
    return total;
}

// ------------------------------------------------------------------------------------------------- the fitted form
// OR up to 32 bits into the chunk at bit `pos`
__device__ __forceinline__ void or_bits(uint32_t *words, uint32_t pos, uint32_t v) {
    const unsigned long long acc = (unsigned long long)v << (pos & 31u);
    if ((uint32_t)acc) atomicOr(&words[pos >> 5], (uint32_t)acc);
    if ((uint32_t)(acc >> 32)) atomicOr(&words[(pos >> 5) + 1], (uint32_t)(acc >> 32));
}

// f.hist (counts of the used symbols, at least two) -> f.len, by all 256 threads.  Ends in a barrier.
__device__ __forceinline__ void fitted_lengths(PngFit &f) {
    const int tid = threadIdx.x;
    for (;;) {
        for (int s = tid; s < kLitPad; s += kPngThreads) {
            const uint32_t c = s < kLitLen ? f.hist[s] : 0u;
            f.key[s] = c ? (c << 9 | (uint32_t)s) : 0xffffffffu;
            f.len[s] = 0;
        }
        if (tid == 0) f.deepest = 0;
        __syncthreads();
        // rank sort: a symbol's place is the number of smaller keys (keys of used symbols are distinct)
        const uint32_t my0 = f.key[tid], my1 = tid + kPngThreads < kLitPad ? f.key[tid + kPngThreads] : 0xffffffffu;
        uint32_t r0 = 0, r1 = 0, m = 0;
        for (int i = 0; i < kLitPad / 4; ++i) {
            const uint4 k = reinterpret_cast<const uint4 *>(f.key)[i];
            r0 += (k.x < my0) + (k.y < my0) + (k.z < my0) + (k.w < my0);
            r1 += (k.x < my1) + (k.y < my1) + (k.z < my1) + (k.w < my1);
            m += (k.x != 0xffffffffu) + (k.y != 0xffffffffu) + (k.z != 0xffffffffu) + (k.w != 0xffffffffu);
        }
        if (my0 != 0xffffffffu) f.lw[r0] = my0 >> 9, f.order[r0] = (uint16_t)tid;
        if (my1 != 0xffffffffu) f.lw[r1] = my1 >> 9, f.order[r1] = (uint16_t)(tid + kPngThreads);
        __syncthreads();
        // the merge, a serial chain of m - 1 steps: one lane.  Heads of the two queues in registers; ~0 = queue empty.
        if (tid == 0) {
            uint32_t li = 0, ii = 0, wl = f.lw[0], wi = 0xffffffffu;
            for (uint32_t k = 0; k + 1 < m; ++k) {
                uint32_t w = 0;
                for (int pick = 0; pick < 2; ++pick) {
                    if (wl <= wi) {  // (a tie goes to the leaf)
                        w += wl;
                        f.lpar[li++] = (uint16_t)k;
                        wl = li < m ? f.lw[li] : 0xffffffffu;
                    } else {
                        w += wi;
                        f.ipar[ii++] = (uint16_t)k;
                        wi = ii < k ? f.iw[ii] : 0xffffffffu;
                    }
                }
                f.iw[k] = w;
                if (ii == k) wi = w;  // the new node is the head of a queue that was empty
            }
        }
        __syncthreads();
        // a leaf's depth: steps to the root (node m - 2)
        for (uint32_t i = tid; i < m; i += kPngThreads) {
            uint32_t d = 1, p = f.lpar[i];
            while (p != m - 2u) p = f.ipar[p], ++d;
            f.len[f.order[i]] = (uint8_t)d;
            atomicMax(&f.deepest, d);
        }
        __syncthreads();
        if (f.deepest <= (uint32_t)kMaxBits) return;
        __syncthreads();  // (everyone has read `deepest`)
        for (int s = tid; s < kLitLen; s += kPngThreads) f.hist[s] = (f.hist[s] + 1u) >> 1;
        __syncthreads();
    }
}

// The code-length sequence of f.len: positions 0 .. n_lit - 1 are the literal/length lengths up to the last used symbol,
// position n_lit the one distance length (1).  This thread's positions are tid and 256 + tid: hc / hn = their bits (LSB
// first; 0 bits inside a zero run that an earlier position encodes), hoff = the bit offsets in the block.  Returns the
// bits of header + sequence.  Zero runs: 18 while >= 11 zeros are left, 17 for 3..10, else plain zeros.
__device__ __forceinline__ uint32_t fitted_header(PngFit &f, uint32_t *wave, uint32_t (&hc)[2], uint32_t (&hn)[2],
                                                  uint32_t (&hoff)[2], uint32_t &n_lit) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t l[2] = {f.len[tid], tid < kLitLen - kPngThreads ? (uint32_t)f.len[kPngThreads + tid] : 0u};
    const unsigned long long b0 = __ballot(l[0] != 0u), b1 = __ballot(l[1] != 0u);
    if (lane == 0) {
        f.nz[wv] = b0;
        // (the end of block, symbol 256, is always used: b1 != 0)  bit n_lit - 256: the distance length
        if (wv == 0) f.nz[4] = b1 | (2ull << (63 - __clzll((long long)b1)));
    }
    __syncthreads();
    n_lit = (uint32_t)(kPngThreads + 63 - __clzll((long long)f.nz[4]));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t p = (uint32_t)(h * kPngThreads + tid);
        const uint32_t len = p == n_lit ? 1u : l[h];
        uint32_t sym = len, xv = 0, xb = 0;
        bool emits = p <= n_lit;
        {
            // the zero run around p: behind the last non-zero position below p, up to the first one above (bit n_lit is
            // set: there is one).  Selects over the five mask words, no loops of data-dependent length.
            const int pw = (int)(p >> 6);
            const unsigned long long lo = (1ull << (p & 63u)) - 1ull, hi = ~((2ull << (p & 63u)) - 1ull);
            int start = 0, end = 0;
#pragma unroll 1
            for (int w = 0; w < 5; ++w) {
                const unsigned long long c = f.nz[w] & (w < pw ? ~0ull : (w == pw ? lo : 0ull));
                start = c ? w * 64 + 64 - __clzll((long long)c) : start;
            }
#pragma unroll 1
            for (int w = 4; w >= 0; --w) {
                const unsigned long long c = f.nz[w] & (w > pw ? ~0ull : (w == pw ? hi : 0ull));
                end = c ? w * 64 + __ffsll((long long)c) - 1 : end;
            }
            const int k = (int)p - start, blk = k / kZeroRun, off = k - blk * kZeroRun, rem = end - start - blk * kZeroRun;
            const bool zero = emits && len == 0u, r18 = zero && rem >= 11, r17 = zero && !r18 && rem >= 3;
            emits = emits && (!(r18 || r17) || off == 0);
            sym = r18 ? 18u : (r17 ? 17u : sym);
            xv = r18 ? (uint32_t)min(rem, kZeroRun) - 11u : (r17 ? (uint32_t)rem - 3u : 0u);
            xb = r18 ? 7u : (r17 ? 3u : 0u);
        }
        // the canonical codes of kClBits: 4 bits 0..12 for symbols 0..10, 17, 18; 5 bits 26..31 for 11..16
        const bool five = sym >= 11u && sym <= 16u;
        const uint32_t c = five ? 15u + sym : (sym >= 17u ? sym - 6u : sym), bits = five ? 5u : 4u;
        hc[h] = emits ? (__brev(c) >> (32u - bits)) | (xv << bits) : 0u;
        hn[h] = emits ? bits + xb : 0u;
    }
    const uint32_t s0 = block_scan_sum<true>(hn[0], wave);
    const uint32_t t0 = wave[0] + wave[1] + wave[2] + wave[3];
    const uint32_t s1 = block_scan_sum<true>(hn[1], wave);
    const uint32_t t1 = wave[0] + wave[1] + wave[2] + wave[3];
    hoff[0] = kFitHeaderBits + s0 - hn[0];
    hoff[1] = kFitHeaderBits + t0 + s1 - hn[1];
    __syncthreads();  // (`wave` is free again)
    return kFitHeaderBits + t0 + t1;
}

// f.len -> f.tab: canonical codes (RFC 1951 3.2.2), bit-reversed for LSB-first output.  A symbol's code is the first code
// of its length + the number of smaller symbols of that length: a ballot per length, counts per 64-symbol chunk.
__device__ __forceinline__ void fitted_codes(PngFit &f) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t l0 = f.len[tid], l1 = tid < kLitLen - kPngThreads ? (uint32_t)f.len[kPngThreads + tid] : 0u;
    unsigned long long mine0 = 0, mine1 = 0;
#pragma unroll 1
    for (uint32_t b = 1; b <= (uint32_t)kMaxBits; ++b) {
        const unsigned long long m0 = __ballot(l0 == b), m1 = __ballot(l1 == b);
        mine0 = l0 == b ? m0 : mine0;
        mine1 = l1 == b ? m1 : mine1;
        if (lane == 0) {
            f.cnt[wv][b] = (uint32_t)__popcll(m0);
            if (wv == 0) f.cnt[4][b] = (uint32_t)__popcll(m1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t code = 0, before = 0;
        for (int b = 1; b <= kMaxBits; ++b) {
            code = (code + before) << 1;
            f.next[b] = code;
            before = f.cnt[0][b] + f.cnt[1][b] + f.cnt[2][b] + f.cnt[3][b] + f.cnt[4][b];
        }
    }
    __syncthreads();
    const unsigned long long lower = (1ull << lane) - 1ull;
    uint32_t t = 0;
    if (l0) {
        uint32_t r = (uint32_t)__popcll(mine0 & lower);
        for (int c = 0; c < wv; ++c) r += f.cnt[c][l0];
        t = (__brev(f.next[l0] + r) >> (32u - l0)) | (l0 << 16);
    }
    f.tab[tid] = t;
    if (tid < kLitPad - kPngThreads) {  // (wave 0)
        t = 0;
        if (l1) {
            const uint32_t r = (uint32_t)__popcll(mine1 & lower) + f.cnt[0][l1] + f.cnt[1][l1] + f.cnt[2][l1] + f.cnt[3][l1];
            t = (__brev(f.next[l1] + r) >> (32u - l1)) | (l1 << 16);
        }
        f.tab[kPngThreads + tid] = t;
    }
    __syncthreads();
}

// grid (segments, N)
template <bool kFitted>
__global__ __launch_bounds__(kPngThreads) void k_png_measure(const uint8_t *__restrict__ img, int H, int W,
                                                            uint32_t *__restrict__ ws) {
    __shared__ PngShared sh;
    const uint32_t n_total = (uint32_t)H * ((uint32_t)W + 1u), seg = blockIdx.x;
    const int n = (int)min((uint32_t)kSeg, n_total - seg * kSeg);
    img += (int64_t)blockIdx.y * H * W;
    load_segment(img, W, seg, n, sh);
    uint32_t code[kPer], nb[kPer], bytes[kPer], tok[kPer];
    const uint32_t bits = block_sum(thread_tokens<kFitted>(sh, n, code, nb, bytes, tok), sh.wave);
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
    const uint32_t fixed_len = (3u + bits + 7u + 3u + 7u) / 8u + 4u, stored_len = 5u + (uint32_t)n;
    const bool stored = fixed_len > stored_len;
    uint32_t len = stored ? stored_len : fixed_len, form = stored ? kFormStored : kFormFixed;
    if constexpr (kFitted) {
        __shared__ PngFit fit;
        for (int s = threadIdx.x; s < kLitPad; s += kPngThreads) fit.hist[s] = s == kEob ? 1u : 0u;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPer; ++j)
            if (tok[j] != kNoToken) atomicAdd(&fit.hist[tok[j] & 511u], 1u);
        __syncthreads();
        fitted_lengths(fit);
        uint32_t tb = 0;  // a token: its code, its extra bits, and for a match the distance code of 1 bit
#pragma unroll
        for (int j = 0; j < kPer; ++j) tb += fit.len[tok[j] & 511u] + ((tok[j] >> 9) & 7u) + (tok[j] >> 17);
        tb = block_sum(tb, sh.wave);
        uint32_t hc[2], hn[2], hoff[2], n_lit;
        const uint32_t head = fitted_header(fit, sh.wave, hc, hn, hoff, n_lit);
        const uint32_t fitted_len = (head + tb + fit.len[kEob] + 3u + 7u) / 8u + 4u;
        if (fitted_len < len) {  // (a tie stays with the fixed / stored choice)
            len = fitted_len, form = kFormFitted;
            uint32_t *lens = ws + (size_t)gridDim.y * gridDim.x * kWsWords + ((size_t)blockIdx.y * gridDim.x + seg) * kLenWords;
            if (threadIdx.x < kLenWords) lens[threadIdx.x] = reinterpret_cast<const uint32_t *>(fit.len)[threadIdx.x];
        }
    }
    if (threadIdx.x == 0) {
        uint32_t *rec = ws + ((size_t)blockIdx.y * gridDim.x + seg) * kWsWords;
        rec[0] = (len + (seg == 0 ? 2u : 0u)) | (stored && form != kFormFitted ? kStoredFlag : 0u);
        rec[1] = a % kAdlerMod;
        rec[2] = b % kAdlerMod;
        rec[3] = kFitted ? form : 0u;
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
__device__ __forceinline__ void png_frame_ends(PngShared &sh, int H, int W, const PngHead head,
                                               const uint32_t *__restrict__ ws, uint32_t n_seg, uint8_t *__restrict__ out,
                                               int32_t *__restrict__ length) {
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
    const uint32_t end = head.first_idat + block_sum(bytes, sh.wave);  // where the last segment's chunk ends
    if (head.palette) {
        // PLTE behind IHDR: length, tag, the 768 palette bytes, and the CRC-32 of tag + bytes from per-thread slices of 4
        // bytes, each moved to its place by x^(8 * bytes behind it), as for the segments' chunks
        const uint32_t L = 4u + kPlteData, lo = min(L, (uint32_t)tid * 4u), hi = min(L, lo + 4u);
        uint32_t raw = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            const uint32_t byte = i < 4u ? (0x45544c50u >> (8u * i)) & 255u : head.palette[i - 4u];  // 'P' 'L' 'T' 'E'
            raw = crc_step(raw, byte, sh.crc_tab);
        }
        uint32_t part = hi > lo ? gf_mul(gf_pow8(L - hi, sh.x8), raw) : 0u;
        if (tid == 0) part ^= gf_mul(gf_pow8(L, sh.x8), 0xffffffffu);
        const uint32_t crc = block_xor(part, sh.wave) ^ 0xffffffffu;
        uint8_t *plte = out + kHeadBytes;
        if (tid == 0) {
            put_be32(plte, kPlteData);
            plte[4] = 'P', plte[5] = 'L', plte[6] = 'T', plte[7] = 'E';
            put_be32(plte + 8 + kPlteData, crc);
        }
        for (uint32_t i = tid; i < kPlteData; i += kPngThreads) plte[8 + i] = head.palette[i];
    }
    if (tid == 0) {
        uint8_t *h = sh.small;
        const uint32_t sig0 = 0x474e5089u, sig1 = 0x0a1a0a0du;  // 89 'P' 'N' 'G' \r \n 1a \n
        for (int i = 0; i < 4; ++i) h[i] = (uint8_t)(sig0 >> (8 * i)), h[4 + i] = (uint8_t)(sig1 >> (8 * i));
        put_be32(h + 8, 13u);
        h[12] = 'I', h[13] = 'H', h[14] = 'D', h[15] = 'R';
        put_be32(h + 16, (uint32_t)W);
        put_be32(h + 20, (uint32_t)H);
        h[24] = 8, h[25] = (uint8_t)head.color_type, h[26] = 0, h[27] = 0, h[28] = 0;
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
template <bool kFitted>
__global__ __launch_bounds__(kPngThreads) void k_png_emit(const uint8_t *__restrict__ img, int H, int W, const PngHead head,
                                                         const uint32_t *__restrict__ ws, uint8_t *__restrict__ out,
                                                         int64_t capacity, int32_t *__restrict__ lengths) {
    __shared__ PngShared sh;
    const int tid = threadIdx.x;
    const uint32_t n_total = (uint32_t)H * ((uint32_t)W + 1u);  // <= 2^30
    const uint32_t seg = blockIdx.x, n_seg = gridDim.x - 1;
    const int n = (int)min((uint32_t)kSeg, n_total - seg * kSeg);
    img += (int64_t)blockIdx.y * H * W;
    const uint32_t *lens = ws + (size_t)gridDim.y * n_seg * kWsWords + ((size_t)blockIdx.y * n_seg + seg) * kLenWords;
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
        png_frame_ends(sh, H, W, head, ws, n_seg, out, lengths + blockIdx.y);
        return;
    }
    // where this chunk starts: the file's head, then the chunks of the segments in front
    uint32_t before = 0;
    for (uint32_t s = tid; s < seg; s += kPngThreads) before += 12u + (ws[(size_t)s * kWsWords] & ~kStoredFlag);
    const uint32_t offset = head.first_idat + block_sum(before, sh.wave);
    const uint32_t rec0 = ws[(size_t)seg * kWsWords];
    const bool stored = (rec0 & kStoredFlag) != 0;
    const uint32_t dlen = rec0 & ~kStoredFlag, zhdr = seg == 0 ? 2u : 0u;
    const bool fitted = kFitted && ws[(size_t)seg * kWsWords + 3] == kFormFitted;
    uint8_t *dst = out + offset;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 3u);  // the chunk sits at byte `mis` of sh.chunk: dwords line up
    const uint32_t total = 12u + dlen, n_words = (mis + total + 3u) / 4u;
    for (uint32_t i = tid; i < n_words; i += kPngThreads) sh.chunk[i] = 0;

    load_segment(img, W, seg, n, sh);  // (ends in a barrier: tables and zeroes are visible)
    uint32_t code[kPer], nb[kPer], bytes[kPer], tok[kPer];
    uint32_t my_bits = thread_tokens<kFitted>(sh, n, code, nb, bytes, tok);
    uint32_t hc[2], hn[2], hoff[2], n_lit;     // (fitted form) this thread's part of the code-length sequence
    uint32_t first_bit = 3u, eob = 0;  // where the tokens start in the block: behind its header; the end-of-block code
    if constexpr (kFitted) {
        __shared__ PngFit fit;
        if (fitted) {  // (uniform over the workgroup)
            if (tid < kLenWords) reinterpret_cast<uint32_t *>(fit.len)[tid] = lens[tid];
            __syncthreads();
            fitted_codes(fit);
            first_bit = fitted_header(fit, sh.wave, hc, hn, hoff, n_lit);
            my_bits = 0;
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const uint32_t t = fit.tab[tok[j] & 511u], l = t >> 16;  // (no token: an entry of 0 bits)
                code[j] = (t & 0xffffu) | (((tok[j] >> 12) & 31u) << l);
                nb[j] = l + ((tok[j] >> 9) & 7u) + (tok[j] >> 17);  // (+ a match's distance code: one 0 bit)
                my_bits += nb[j];
            }
            eob = fit.tab[kEob];
        }
    }
    const uint32_t bit_end = block_scan_sum<kFitted>(my_bits, sh.wave);

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
        uint32_t pos = 8u * (mis + 8u + zhdr) + first_bit + (bit_end - my_bits);
        if (!fitted && tid == 0) atomicOr(&sh.chunk[(8u * (mis + 8u + zhdr)) >> 5], 2u << ((8u * (mis + 8u + zhdr)) & 31u));  // BFINAL 0, BTYPE 01
        if constexpr (kFitted) {
            if (fitted) {
                const uint32_t base = 8u * (mis + 8u + zhdr);
                if (tid == 0) {  // BFINAL 0, BTYPE 10; HLIT, HDIST 0, HCLEN 19 - 4; the code-length code
                    or_bits(sh.chunk, base, 4u | ((n_lit - 257u) << 3) | (15u << 13));
                    or_bits(sh.chunk, base + 17u, (uint32_t)kClHeader);
                    or_bits(sh.chunk, base + 49u, (uint32_t)(kClHeader >> 32));
                }
                if (hn[0]) or_bits(sh.chunk, base + hoff[0], hc[0]);
                if (hn[1]) or_bits(sh.chunk, base + hoff[1], hc[1]);
                if (tid == kPngThreads - 1) or_bits(sh.chunk, pos + my_bits, eob & 0xffffu);  // (the fixed one: 7 zeros)
            }
        }
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

template <bool kFitted>
int png_launch(const uint8_t *bytes, int N, int H, int W, const PngHead head, uint8_t *out, size_t capacity, int32_t *lengths,
               uint32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)png_segments(H, W), (unsigned)N);
    FOSVOS_PROF(kFitted ? "k_png_measure_fitted" : "k_png_measure", stream, 0.0);
    hipLaunchKernelGGL(k_png_measure<kFitted>, grid, dim3(kPngThreads), 0, st, bytes, H, W, ws);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF(kFitted ? "k_png_emit_fitted" : "k_png_emit", stream, 0.0);
    hipLaunchKernelGGL(k_png_emit<kFitted>, dim3(grid.x + 1, grid.y), dim3(kPngThreads), 0, st, bytes, H, W, head, ws,
                       out, (int64_t)capacity, lengths);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}
}  // namespace

extern "C" size_t fosvos_png_capacity_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)png_file_bound(H, W);
}

extern "C" size_t fosvos_png_workspace_bytes(int N, int H, int W, int huffman) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * (size_t)png_segments(H, W) * (kWsWords + (huffman ? kLenWords : 0)) * sizeof(uint32_t);
}

// both file encoders: the greyscale one (no palette) and the indexed one
static int png_encode_any(const char *who, const uint8_t *bytes, int N, int H, int W, int huffman, const uint8_t *palette,
                          uint8_t *out, size_t capacity, int32_t *lengths, void *workspace, size_t workspace_bytes, int device,
                          void *stream) {
    FOSVOS_REQUIRE(huffman == 0 || huffman == 1, FOSVOS_E_ARG, "%s: huffman=%d (0 fixed, 1 fitted)", who, huffman);
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && png_stream_bytes(H, W) <= ((int64_t)1 << 30), FOSVOS_E_SHAPE,
                   "%s: N=%d (<= 65535) H=%d W=%d (H * (W + 1) <= 2^30)", who, N, H, W);
    FOSVOS_REQUIRE(bytes && out && lengths && workspace, FOSVOS_E_ARG, "%s: null pointer", who);
    FOSVOS_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)lengths & 3) == 0, FOSVOS_E_ARG,
                   "%s: the workspace and the lengths must be 4-byte aligned", who);
    const size_t need_cap = fosvos_png_capacity_bytes(N, H, W) + (palette ? kPlteChunk : 0u);
    const size_t need_ws = fosvos_png_workspace_bytes(N, H, W, huffman);
    FOSVOS_REQUIRE(capacity >= need_cap, FOSVOS_E_WORKSPACE, "%s: capacity %zu B a frame < %zu B", who, capacity, need_cap);
    FOSVOS_REQUIRE(workspace_bytes >= need_ws, FOSVOS_E_WORKSPACE, "%s: workspace %zu B < %zu B", who, workspace_bytes, need_ws);
    FOSVOS_ENTER(device);
    uint32_t *ws = reinterpret_cast<uint32_t *>(workspace);
    const PngHead head = {palette ? 3u : 0u, kHeadBytes + (palette ? kPlteChunk : 0u), palette};
    // (<false> named first: the fixed kernels stay in front of the fitted ones in the code object)
    return huffman == 0 ? png_launch<false>(bytes, N, H, W, head, out, capacity, lengths, ws, stream)
                        : png_launch<true>(bytes, N, H, W, head, out, capacity, lengths, ws, stream);
}

extern "C" int fosvos_png_encode(const uint8_t *bytes, int N, int H, int W, int huffman, uint8_t *out, size_t capacity,
                                 int32_t *lengths, void *workspace, size_t workspace_bytes, int device, void *stream) {
    return png_encode_any("png_encode", bytes, N, H, W, huffman, nullptr, out, capacity, lengths, workspace, workspace_bytes,
                          device, stream);
}

extern "C" size_t fosvos_png_indexed_capacity_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)png_file_bound(H, W) + kPlteChunk;
}

extern "C" int fosvos_png_encode_indexed(const uint8_t *labels, const uint8_t *palette, int N, int H, int W, int huffman,
                                         uint8_t *out, size_t capacity, int32_t *lengths, void *workspace,
                                         size_t workspace_bytes, int device, void *stream) {
    FOSVOS_REQUIRE(palette != nullptr, FOSVOS_E_ARG, "png_encode_indexed: null palette");
    return png_encode_any("png_encode_indexed", labels, N, H, W, huffman, palette, out, capacity, lengths, workspace,
                          workspace_bytes, device, stream);
}
