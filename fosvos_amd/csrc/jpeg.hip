// JPEG files of the streamed output frames, encoded on the device (fosvos_jpeg_encode): uint8 [N,H,W,3] BGR or [N,H,W] grey ->
// N standalone baseline JFIF files.  The layout is the one util/jpeg_layout.py states in integers (the tests compare byte
// for byte):
//
//   SOI | APP0 | DQT (x2 colour) | SOF0 | DHT x2 (x4 colour) | DRI | SOS | interval 0 | RST0 | interval 1 | ... | EOI
//
// 4:4:4, an MCU is one 8x8 block per component; a restart interval is kRi = 32 MCUs in raster order and needs nothing from
// any other, so one workgroup of 256 threads encodes one interval, whole, in LDS:
//   1  thread (MCU m = tid & 31, row r = tid >> 5) loads the 8 pixels of its row (8-byte loads where the row segment is
//      aligned and inside the frame, bytes with the edge replicated otherwise), converts them (16-bit fixed point), shifts
//      by -128 and runs the DCT row pass in registers -> stage (int16)
//   2  thread (MCU m, column u = tid >> 5) runs the column pass per component, quantises (round half away from zero, AC
//      clamped to +-1023) and stores the coefficient at its zigzag place (int16), OR-ing the block's 64-bit non-zero mask
//   3  a thread owns kPer consecutive zigzag places of one block.  With the mask a non-zero coefficient stands alone: its
//      zero run is the distance to the next lower set bit, it carries the ZRLs in front of it, and the highest one (or the
//      DC where no AC is set) carries the EOB - at most 3 * 11 + 16 + 10 + 4 = 63 bits.  Bit counts are prefix-summed over
//      the workgroup, then the same codes are OR-ed MSB first into big-endian words of LDS; the 1-padding to the byte.
//   4  per word the 0xFF bytes are counted and prefix-summed: the stuffed length (k_jpeg<.., false>, "measure", which ends
//      here and writes it to the workspace) or the place of every byte in the file (k_jpeg<.., true>, "emit": the
//      workgroup starts behind the header and the measured intervals in front of it, 2 marker bytes each, and writes its
//      bytes, the 00 behind every FF and its RST marker with byte stores).
// One more workgroup per frame of the emit launch writes the header, EOI and the file length.  The DCT is the
// Loeffler-Ligtenberg-Moschytz factorisation with 13-bit constants (jpeg_layout.fdct_1d).  Integers only.
//
// 4:2:0 (sampling 420, colour only; k_jpeg<3, .., true>): an MCU is 16x16 pixels and six blocks, Y(0,0)
// Y(0,1) Y(1,0) Y(1,1) Cb Cr, an interval is kRi420 = 16 MCUs - again 96 blocks, so phases 3 and 4 are the ones above with
// another block -> (MCU, table) map - and phases 1 and 2 become (jpeg_blocks_420):
//   1  thread (MCU m = tid & 15, row r = tid >> 4 of 16) loads the 16 pixels of its row (13 aligned words funnel-shifted to
//      the row's byte offset where the segment is inside the frame, bytes with the edge replicated otherwise), converts
//      them at full resolution and runs the row pass of its two luma blocks.  It sums its 8 horizontal chroma pairs; rows
//      r and r ^ 1 are lanes tid and tid ^ 16 of one wave, so one __shfl_xor per pair completes the 2x2 sums in registers:
//      the even row takes Cb, the odd row Cr, each adds the alternating bias, shifts and runs that block's row pass.
//   2  thread (MCU m, column u = (tid >> 4) & 7, half = tid >> 7) runs the column pass of three blocks - Y(half,0)
//      Y(half,1) and Cb or Cr.  A chroma row below the picture's last one reads that one's row-pass result (the layout
//      replicates the halved plane).  A dummy luma block (beyond ceil(W/8) x ceil(H/8) blocks) is skipped here: its mask
//      stays "DC only", and one thread per MCU then copies the DC of the block in front of it, in coding order.
// LDS holds block (slot s of 6, MCU m) at index s * 16 + m, so that the 16 MCUs of a wave's lanes stay an odd word stride apart.
#include "common.hpp"

using namespace fosvos;

namespace {
constexpr int kRi = 32, kJpegThreads = 256, kStride = 66;  // halfwords per block in LDS: 33 words, odd
constexpr int kRi420 = 16;                                 // MCUs of an interval with 4:2:0: 16 x 6 blocks
constexpr int kAcMax = 1023, kBlockBytes = 208;           // 64 coefficients of at most 26 bits
constexpr int kHeaderMax = 640;
// SOI .. SOS (jpeg_layout.header_bytes)
constexpr __host__ __device__ int jpeg_header_bytes(int C) {
    const int tables = C == 3 ? 2 : 1;
    return 2 + 18 + 69 * tables + 10 + 3 * C + 216 * tables + 6 + 8 + 2 * C;
}
static_assert(jpeg_header_bytes(1) <= kHeaderMax && jpeg_header_bytes(3) <= kHeaderMax, "the header is built in LDS");

struct JpegQ {
    uint8_t q[2][64];  // natural order
};

// Annex K.1 / K.2, natural order
constexpr uint8_t kQBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
     103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct ZigTables {
    uint8_t nat[64];  // zigzag place -> natural index
    uint8_t inv[64];  // natural index -> zigzag place
};
constexpr ZigTables make_zigzag() {
    ZigTables t{};
    int z = 0;
    for (int s = 0; s < 15; ++s)
        for (int i = 0; i <= s; ++i) {
            const int a = (s & 1) ? i : s - i, b = s - a;  // even diagonals run upwards
            if (a < 8 && b < 8) {
                t.nat[z] = (uint8_t)(a * 8 + b);
                t.inv[a * 8 + b] = (uint8_t)z;
                ++z;
            }
        }
    return t;
}
constexpr ZigTables kZigHost = make_zigzag();
static_assert(kZigHost.nat[2] == 8 && kZigHost.nat[3] == 16 && kZigHost.nat[9] == 24 && kZigHost.nat[62] == 62 && kZigHost.inv[63] == 63,
              "the zigzag order of Figure A.6");
__device__ const ZigTables kZig = make_zigzag();

// Annex K.3: code counts per length and the symbols in code order; DC0, AC0, DC1, AC1
struct HuffSpec {
    uint8_t counts[16];
    uint8_t n;
    uint8_t syms[162];
};
constexpr HuffSpec kDc0 = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDc1 = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAc0 = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAc1 = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
__device__ const HuffSpec kSpecs[4] = {kDc0, kAc0, kDc1, kAc1};

// symbol -> code | bits << 16, the canonical assignment of Annex C
struct HuffEnc {
    uint32_t e[256];
};
constexpr HuffEnc make_enc(const HuffSpec &s) {
    HuffEnc t{};
    uint32_t code = 0;
    int k = 0;
    for (int bits = 1; bits <= 16; ++bits) {
        for (int i = 0; i < s.counts[bits - 1]; ++i) t.e[s.syms[k++]] = code++ | ((uint32_t)bits << 16);
        code <<= 1;
    }
    return t;
}
__device__ const HuffEnc kEnc[4] = {make_enc(kDc0), make_enc(kAc0), make_enc(kDc1), make_enc(kAc1)};

inline int64_t jpeg_mcus(int H, int W, bool s420) { return s420 ? cdiv(H, 16) * cdiv(W, 16) : cdiv(H, 8) * cdiv(W, 8); }
inline int64_t jpeg_intervals(int H, int W, bool s420) { return cdiv(jpeg_mcus(H, W, s420), s420 ? kRi420 : kRi); }
// jpeg_layout.capacity: 26 bits a coefficient, doubled by the stuffing, two marker bytes an interval; 4:2:0: six blocks
// for every MCU of the padded grid
inline int64_t jpeg_file_bound(int H, int W, int C, bool s420) {
    return jpeg_header_bytes(C) + 2 * (int64_t)kBlockBytes * jpeg_mcus(H, W, s420) * (s420 ? 6 : C) + 2 * jpeg_intervals(H, W, s420);
}

template <int C>
struct JpegShared {
    static constexpr int kBlocks = kRi * C;
    static constexpr int kBitWords = kBlocks * kBlockBytes / 4 + 2;  // (a code spans up to three words)
    union {
        int16_t stage[kBlocks * kStride];  // phase 1 -> 2: row pass results, [block][row][u]
        uint32_t bits[kBitWords];          // phase 3 -> 4: the interval's bits, big-endian words
        uint8_t header[kHeaderMax];        // the workgroup of the frame's ends
    };
    int16_t coef[kBlocks * kStride];  // [block = component * 32 + MCU][zigzag place]
    uint32_t nz[kBlocks][2];          // bit z: the coefficient at zigzag place z is not 0
    uint32_t enc_ac[2][256];
    uint32_t enc_dc[2][12];
    uint32_t wave[kJpegThreads / 64];
};

// One pass of the DCT over d[0..7], in place (jpeg_layout.fdct_1d)
template <bool kFirst>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
    constexpr int kConstBits = 13, kPass1Bits = 2, n = kFirst ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
    constexpr int r = 1 << (n - 1);
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if constexpr (kFirst) {
        d[0] = (t10 + t11) * (1 << kPass1Bits);
        d[4] = (t10 - t11) * (1 << kPass1Bits);
    } else {
        d[0] = (t10 + t11 + (1 << (kPass1Bits - 1))) >> kPass1Bits;
        d[4] = (t10 - t11 + (1 << (kPass1Bits - 1))) >> kPass1Bits;
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = (z1 + t13 * 6270 + r) >> n;
    d[6] = (z1 - t12 * 15137 + r) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z5 - z3 * 16069, z4 = z5 - z4 * 3196;
    d[7] = (t4 + z1 + z3 + r) >> n;
    d[5] = (t5 + z2 + z4 + r) >> n;
    d[3] = (t6 + z2 + z3 + r) >> n;
    d[1] = (t7 + z1 + z4 + r) >> n;
}

// Component c (Y, Cb, Cr) of a BGR pixel, 0..255: libjpeg's 16-bit fixed-point rows (jpeg_layout._planes)
__device__ __forceinline__ int jpeg_ycc(int c, int b, int g, int r) {
    const int v = c == 0   ? 19595 * r + 38470 * g + 7471 * b + 32768
                  : c == 1 ? -11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767
                           : 32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767;
    return v >> 16;
}

// Phase 2 for column u of staged block b: column pass, quantisation with table `table` (round half away from zero, AC
// clamped), the coefficients to their zigzag places, the block's non-zero mask.  `rows`: the real rows of the staged block;
// a row beyond them reads row rows - 1.
template <int C>
__device__ __forceinline__ void quantise_column(JpegShared<C> &sh, const JpegQ &qt, int b, int u, int table, int rows) {
    int d[8];
#pragma unroll
    for (int yy = 0; yy < 8; ++yy) d[yy] = sh.stage[b * kStride + min(yy, rows - 1) * 8 + u];
    fdct_1d<false>(d);
    uint32_t nz0 = 0, nz1 = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int nat = v * 8 + u;
        const uint32_t q8 = (uint32_t)qt.q[table][nat] << 3;
        const uint32_t a = (uint32_t)(d[v] < 0 ? -d[v] : d[v]);
        int mag = (int)((a + (q8 >> 1)) / q8);
        if (nat != 0) mag = min(mag, kAcMax);
        const int z = kZig.inv[nat];
        sh.coef[b * kStride + z] = (int16_t)(d[v] < 0 ? -mag : mag);
        if (mag) (z < 32 ? nz0 : nz1) |= 1u << (z & 31);
    }
    if (nz0) atomicOr(&sh.nz[b][0], nz0);
    if (nz1) atomicOr(&sh.nz[b][1], nz1);
}

// The bits the coefficient at zigzag place k of a block adds to the scan (see phase 3 above): code, right-aligned, and
// its length.  nzb: the block's mask with bit 0 (the DC) set; v: the coefficient, or the DC difference for k = 0.
__device__ __forceinline__ void coef_code(int k, unsigned long long nzb, int v, const uint32_t *enc_dc, const uint32_t *enc_ac,
                                          unsigned long long &code, uint32_t &len) {
    const int a = v < 0 ? -v : v;
    const uint32_t s = 32u - (uint32_t)__clz(a);  // size category (0 for 0)
    const uint32_t value = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
    code = 0, len = 0;
    uint32_t e;
    if (k == 0) {
        e = enc_dc[s];
    } else {
        const int prev = 63 - __clzll((long long)(nzb & ((1ull << k) - 1ull)));  // (bit 0 is set)
        const uint32_t run = (uint32_t)(k - prev - 1);
        const uint32_t zrl = enc_ac[0xF0];
        for (uint32_t i = 0; i < (run >> 4); ++i) code = (code << (zrl >> 16)) | (zrl & 0xffffu), len += zrl >> 16;
        e = enc_ac[((run & 15u) << 4) | s];
    }
    code = (((code << (e >> 16)) | (e & 0xffffu)) << s) | value;
    len += (e >> 16) + s;
    const int top = 63 - __clzll((long long)nzb);
    if (k == top && top < 63) {
        const uint32_t eob = enc_ac[0x00];
        code = (code << (eob >> 16)) | (eob & 0xffffu), len += eob >> 16;
    }
}

// OR `len` (1..63) bits into the big-endian words at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t *words, uint32_t pos, unsigned long long code, uint32_t len) {
    const unsigned long long v = code << (64u - len);
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v, o = pos & 31u, w = pos >> 5;
    const uint32_t w0 = hi >> o, w1 = o ? (hi << (32u - o)) | (lo >> o) : lo, w2 = o ? lo << (32u - o) : 0u;
    if (w0) atomicOr(&words[w], w0);
    if (w1) atomicOr(&words[w + 1], w1);
    if (w2) atomicOr(&words[w + 2], w2);
}

__device__ __forceinline__ void put_be16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 8), p[1] = (uint8_t)v; }

// SOI .. SOS into h; returns the length (jpeg_layout.header)
template <int C, bool k420>
__device__ int build_header(uint8_t *h, int H, int W, const JpegQ &qt) {
    constexpr int kTables = C == 3 ? 2 : 1;
    int n = 0;
    h[n++] = 0xFF, h[n++] = 0xD8;
    const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 18; ++i) h[n++] = app0[i];
    for (int t = 0; t < kTables; ++t) {
        h[n++] = 0xFF, h[n++] = 0xDB, h[n++] = 0, h[n++] = 67, h[n++] = (uint8_t)t;
        for (int z = 0; z < 64; ++z) h[n++] = qt.q[t][kZig.nat[z]];
    }
    h[n++] = 0xFF, h[n++] = 0xC0, h[n++] = 0, h[n++] = (uint8_t)(8 + 3 * C), h[n++] = 8;
    put_be16(h + n, (uint32_t)H), put_be16(h + n + 2, (uint32_t)W), n += 4;
    h[n++] = (uint8_t)C;
    for (int c = 0; c < C; ++c) h[n++] = (uint8_t)(c + 1), h[n++] = (k420 && c == 0) ? 0x22 : 0x11, h[n++] = c ? 1 : 0;
    for (int t = 0; t < 2 * kTables; ++t) {
        const HuffSpec &s = kSpecs[t];
        h[n++] = 0xFF, h[n++] = 0xC4;
        put_be16(h + n, 2u + 1u + 16u + s.n), n += 2;
        h[n++] = (uint8_t)(((t & 1) << 4) | (t >> 1));
        for (int i = 0; i < 16; ++i) h[n++] = s.counts[i];
        for (int i = 0; i < s.n; ++i) h[n++] = s.syms[i];
    }
    h[n++] = 0xFF, h[n++] = 0xDD, h[n++] = 0, h[n++] = 4, h[n++] = 0, h[n++] = k420 ? kRi420 : kRi;
    h[n++] = 0xFF, h[n++] = 0xDA, h[n++] = 0, h[n++] = (uint8_t)(6 + 2 * C), h[n++] = (uint8_t)C;
    for (int c = 0; c < C; ++c) h[n++] = (uint8_t)(c + 1), h[n++] = c ? 0x11 : 0x00;
    h[n++] = 0, h[n++] = 63, h[n++] = 0;
    return n;
}

// A luma block beyond the frame's block grid (jpeg_layout.dummy_blocks)
__device__ __forceinline__ bool jpeg420_dummy(int slot, uint32_t mx, uint32_t my, uint32_t blocks_w, uint32_t blocks_h) {
    return slot < 4 && (2u * mx + (uint32_t)(slot & 1) >= blocks_w || 2u * my + (uint32_t)(slot >> 1) >= blocks_h);
}

// Phases 1 and 2 of the 4:2:0 form (see the top of the file); block (slot, MCU m) is at index slot * kRi420 + m.
__device__ __forceinline__ void jpeg_blocks_420(JpegShared<3> &sh, const uint8_t *__restrict__ frames, int H, int W,
                                                const JpegQ &qt, uint32_t first, int n_m, uint32_t mcus_w) {
    const int tid = threadIdx.x, m = tid & 15, hi = tid >> 4;
    const uint32_t blocks_w = ((uint32_t)W + 7u) / 8u, blocks_h = ((uint32_t)H + 7u) / 8u;
    // (a thread beyond the interval's last MCU works on that one and stores nothing: the shuffles below stay whole-wave)
    const uint32_t g = first + (uint32_t)min(m, n_m - 1), my = g / mcus_w, mx = g - my * mcus_w;
    const bool live = m < n_m;

    // ---- 1: 16 pixels of row hi -> Y Cb Cr -> row pass of two luma blocks and one chroma block
    {
        const int r = hi, y = min((int)(my * 16u) + r, H - 1), x0 = (int)(mx * 16u);
        const uint8_t *line = frames + (int64_t)y * W * 3;
        uint8_t px[48];
        if (x0 + 16 <= W) {
            const uint8_t *p = line + x0 * 3;
            const uint32_t shift = (uint32_t)((uintptr_t)p & 3u);
            const uint32_t *a = reinterpret_cast<const uint32_t *>(p - shift);  // (an aligned word that holds a byte of the row)
            uint32_t v[13];
#pragma unroll
            for (int i = 0; i < 12; ++i) v[i] = a[i];
            v[12] = shift ? a[12] : 0u;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const uint32_t word = __builtin_amdgcn_alignbyte(v[i + 1], v[i], shift);
#pragma unroll
                for (int j = 0; j < 4; ++j) px[4 * i + j] = (uint8_t)(word >> (8 * j));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint8_t *q = line + min(x0 + i, W - 1) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) px[i * 3 + c] = q[c];
            }
        }
        int cb[16], cr[16];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = half * 8 + i, b = px[3 * k], gg = px[3 * k + 1], rr = px[3 * k + 2];
                d[i] = jpeg_ycc(0, b, gg, rr) - 128;
                cb[k] = jpeg_ycc(1, b, gg, rr), cr[k] = jpeg_ycc(2, b, gg, rr);  // (the 2x2 sums come before the shift)
            }
            fdct_1d<true>(d);
            if (live) {
                int16_t *row = sh.stage + (((r >> 3) * 2 + half) * kRi420 + m) * kStride + (r & 7) * 8;
#pragma unroll
                for (int u = 0; u < 8; ++u) row[u] = (int16_t)d[u];
            }
        }
        // the 2x2 sums: rows r and r ^ 1 are lanes tid and tid ^ 16; the even row finishes Cb, the odd row Cr
        const bool odd = r & 1;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pair_cb = cb[2 * i] + cb[2 * i + 1], pair_cr = cr[2 * i] + cr[2 * i + 1];
            const int other = __shfl_xor(odd ? pair_cb : pair_cr, 16, 64);
            d[i] = (((odd ? pair_cr : pair_cb) + other + 1 + (i & 1)) >> 2) - 128;
        }
        fdct_1d<true>(d);
        if (live) {
            int16_t *row = sh.stage + ((4 + (r & 1)) * kRi420 + m) * kStride + (r >> 1) * 8;
#pragma unroll
            for (int u = 0; u < 8; ++u) row[u] = (int16_t)d[u];
        }
    }
    __syncthreads();

    // ---- 2: column pass, quantisation, zigzag
    if (live) {
        const int u = hi & 7, half = hi >> 3;
        const int chroma_rows = min(8, (H + 1) / 2 - (int)(my * 8u));  // rows of this MCU's chroma blocks inside the halved plane
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int slot = k < 2 ? half * 2 + k : 4 + half;
            if (jpeg420_dummy(slot, mx, my, blocks_w, blocks_h)) continue;
            quantise_column(sh, qt, slot * kRi420 + m, u, k < 2 ? 0 : 1, k < 2 ? 8 : chroma_rows);
        }
    }
    __syncthreads();
    // dummy blocks: the DC of the block in front, in coding order (a copy may be copied on); their masks stay 0
    if (tid < n_m) {
        const uint32_t gm = first + (uint32_t)tid, ry = gm / mcus_w, rx = gm - ry * mcus_w;
        for (int slot = 1; slot < 4; ++slot)
            if (jpeg420_dummy(slot, rx, ry, blocks_w, blocks_h))
                sh.coef[(slot * kRi420 + tid) * kStride] = sh.coef[((slot - 1) * kRi420 + tid) * kStride];
    }
}

// grid (intervals, N) for the measure form, (intervals + 1, N) for the emit form
template <int C, bool kEmit, bool k420 = false>
__global__ __launch_bounds__(kJpegThreads) void k_jpeg(const uint8_t *__restrict__ frames, int H, int W, JpegQ qt,
                                                       uint32_t *__restrict__ ws, uint8_t *__restrict__ out, int64_t capacity,
                                                       int32_t *__restrict__ lengths) {
    using Shared = JpegShared<C>;
    constexpr int kBlocks = Shared::kBlocks;
    constexpr int kPer = C == 3 ? 32 : 8, kParts = 64 / kPer;  // zigzag places a thread owns in phase 3
    static_assert(kBlocks * kParts <= kJpegThreads, "a thread per part of a block");
    static_assert(!k420 || (C == 3 && kRi420 * 6 == kBlocks), "4:2:0 is a colour form with the block count of 4:4:4");
    constexpr int kMcus = k420 ? kRi420 : kRi, kSide = k420 ? 16 : 8, kPerMcu = k420 ? 6 : C;  // of an interval, an MCU, an MCU
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    const uint32_t n_int = kEmit ? gridDim.x - 1 : gridDim.x, interval = blockIdx.x;
    const uint32_t mcus_w = ((uint32_t)W + kSide - 1u) / kSide, mcus = mcus_w * (((uint32_t)H + kSide - 1u) / kSide);  // (H, W <= 65535: < 2^26)
    ws += (size_t)blockIdx.y * n_int;
    constexpr uint32_t kHeaderBytes = jpeg_header_bytes(C);

    if constexpr (kEmit) {
        out += (int64_t)blockIdx.y * capacity;
        if (interval == n_int) {  // the frame's ends: header, EOI, length
            uint32_t before = 0;
            for (uint32_t s = tid; s < n_int; s += kJpegThreads) before += ws[s] + 2u;
            const uint32_t total = kHeaderBytes + block_sum(before, sh.wave);
            if (tid == 0) build_header<C, k420>(sh.header, H, W, qt);
            __syncthreads();
            for (uint32_t i = tid; i < kHeaderBytes; i += kJpegThreads) out[i] = sh.header[i];
            if (tid == 0) {
                out[total - 2] = 0xFF, out[total - 1] = 0xD9;
                lengths[blockIdx.y] = (int32_t)total;
            }
            return;
        }
    }
    frames += (int64_t)blockIdx.y * H * W * C;
    const uint32_t first = interval * kMcus;
    const int n_m = (int)min((uint32_t)kMcus, mcus - first);  // MCUs of this interval

    // tables into LDS, masks to zero
    sh.enc_ac[0][tid] = kEnc[1].e[tid];
    sh.enc_ac[1][tid] = kEnc[3].e[tid];
    if (tid < 12) sh.enc_dc[0][tid] = kEnc[0].e[tid], sh.enc_dc[1][tid] = kEnc[2].e[tid];
    for (int i = tid; i < kBlocks * 2; i += kJpegThreads) (&sh.nz[0][0])[i] = 0;

    if constexpr (k420) {
        jpeg_blocks_420(sh, frames, H, W, qt, first, n_m, mcus_w);
    } else {
        // ---- 1: pixels -> samples -> row pass
        const int m = tid & 31, lane_hi = tid >> 5;
        if (m < n_m) {
            const uint32_t g = first + (uint32_t)m, my = g / mcus_w, mx = g - my * mcus_w;
            const int y = min((int)(my * 8u) + lane_hi, H - 1), x0 = (int)(mx * 8u);
            const uint8_t *p = frames + ((int64_t)y * W + x0) * C;
            uint8_t px[8 * C];
            const bool inside = x0 + 8 <= W;
            if (inside && ((uintptr_t)p & 7u) == 0) {
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) px[8 * i + j] = (uint8_t)(v.x >> (8 * j)), px[8 * i + 4 + j] = (uint8_t)(v.y >> (8 * j));
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const uint8_t *q = frames + ((int64_t)y * W + min(x0 + i, W - 1)) * C;
#pragma unroll
                    for (int c = 0; c < C; ++c) px[i * C + c] = q[c];
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                int d[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if constexpr (C == 3) {
                        d[i] = jpeg_ycc(c, px[3 * i], px[3 * i + 1], px[3 * i + 2]) - 128;
                    } else {
                        d[i] = (int)px[i] - 128;
                    }
                }
                fdct_1d<true>(d);
                int16_t *row = sh.stage + (c * kRi + m) * kStride + lane_hi * 8;
#pragma unroll
                for (int u = 0; u < 8; ++u) row[u] = (int16_t)d[u];
            }
        }
        __syncthreads();

        // ---- 2: column pass, quantisation, zigzag
        if (m < n_m) {
#pragma unroll
            for (int c = 0; c < C; ++c) quantise_column(sh, qt, c * kRi + m, lane_hi, c ? 1 : 0, 8);
        }
    }
    __syncthreads();  // (stage is dead: the same bytes are `bits` from here on)

    // ---- 3: codes.  Sequence block sb = MCU * kPerMcu + its place in the MCU; this thread: places [part * kPer, part * kPer + kPer)
    const int sb = tid / kParts, part = tid % kParts, sm = sb / kPerMcu, sc = sb - sm * kPerMcu;
    const bool active = sb < n_m * kPerMcu;
    const int blk = sc * kMcus + sm;
    const int table = k420 ? (sc >= 4 ? 1 : 0) : (sc ? 1 : 0);
    unsigned long long nzb = 1ull, mine = 0;
    int dc_diff = 0;
    const uint32_t *enc_dc = sh.enc_dc[table], *enc_ac = sh.enc_ac[table];
    const int16_t *cf = sh.coef + blk * kStride;
    if (active) {
        nzb |= (unsigned long long)sh.nz[blk][0] | ((unsigned long long)sh.nz[blk][1] << 32);
        const unsigned long long range = (kPer == 64 ? ~0ull : ((1ull << kPer) - 1ull)) << (part * kPer);
        mine = nzb & range;
        if constexpr (k420) {  // luma runs through the four blocks of an MCU and on to the next MCU's first
            const int prev = (sc >= 1 && sc <= 3) ? blk - kRi420 : sc == 0 ? 3 * kRi420 + sm - 1 : blk - 1;
            if (part == 0) dc_diff = cf[0] - ((sm > 0 || (sc >= 1 && sc <= 3)) ? sh.coef[prev * kStride] : 0);
        } else {
            if (part == 0) dc_diff = cf[0] - (sm > 0 ? sh.coef[(blk - 1) * kStride] : 0);
        }
    }
    uint32_t my_bits = 0;
    for (unsigned long long rest = mine; rest; rest &= rest - 1ull) {
        const int k = __ffsll((long long)rest) - 1;
        unsigned long long code;
        uint32_t len;
        coef_code(k, nzb, k == 0 ? dc_diff : (int)cf[k], enc_dc, enc_ac, code, len);
        my_bits += len;
    }
    const uint32_t bit_end = block_scan_sum(my_bits, sh.wave);
    const uint32_t total_bits = sh.wave[0] + sh.wave[1] + sh.wave[2] + sh.wave[3];
    const uint32_t n_bytes = (total_bits + 7u) / 8u, n_words = (n_bytes + 3u) / 4u;
    for (uint32_t i = tid; i < n_words + 2u; i += kJpegThreads) sh.bits[i] = 0;
    __syncthreads();
    {
        uint32_t pos = bit_end - my_bits;
        for (unsigned long long rest = mine; rest; rest &= rest - 1ull) {
            const int k = __ffsll((long long)rest) - 1;
            unsigned long long code;
            uint32_t len;
            coef_code(k, nzb, k == 0 ? dc_diff : (int)cf[k], enc_dc, enc_ac, code, len);
            put_bits(sh.bits, pos, code, len);
            pos += len;
        }
        const uint32_t pad = (0u - total_bits) & 7u;
        if (tid == 0 && pad) put_bits(sh.bits, total_bits, (1ull << pad) - 1ull, pad);
    }
    __syncthreads();

    // ---- 4: stuffing.  Word i holds bytes 4 i .. 4 i + 3 of the interval, the first in its top bits.
    uint8_t *dst = nullptr;
    if constexpr (kEmit) {
        uint32_t before = 0;
        for (uint32_t s = tid; s < interval; s += kJpegThreads) before += ws[s] + 2u;
        dst = out + kHeaderBytes + block_sum(before, sh.wave);
    }
    uint32_t stuffed = 0;  // 0xFF bytes in front of the words of this round
    for (uint32_t base = 0; base < n_words; base += kJpegThreads) {
        const uint32_t i = base + tid;
        const uint32_t word = i < n_words ? sh.bits[i] : 0u;
        const uint32_t valid = i < n_words ? min(4u, n_bytes - 4u * i) : 0u;
        uint32_t ff = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) ff += (j < valid && ((word >> (24u - 8u * j)) & 255u) == 255u) ? 1u : 0u;
        if constexpr (kEmit) {
            const uint32_t incl = block_scan_sum(ff, sh.wave);
            uint8_t *p = dst + 4u * i + stuffed + (incl - ff);
            for (uint32_t j = 0; j < valid; ++j) {
                const uint8_t byte = (uint8_t)(word >> (24u - 8u * j));
                *p++ = byte;
                if (byte == 255u) *p++ = 0;
            }
            stuffed += sh.wave[0] + sh.wave[1] + sh.wave[2] + sh.wave[3];
        } else {
            stuffed += ff;
        }
    }
    if constexpr (kEmit) {
        if (tid == 0 && interval + 1 < n_int) {
            uint8_t *p = dst + n_bytes + stuffed;
            p[0] = 0xFF, p[1] = (uint8_t)(0xD0u + (interval & 7u));
        }
    } else {
        const uint32_t all = block_sum(stuffed, sh.wave);
        if (tid == 0) ws[interval] = n_bytes + all;
    }
}

template <int C, bool k420>
int jpeg_launch(const uint8_t *frames, int N, int H, int W, const JpegQ &qt, uint8_t *out, size_t out_stride, int32_t *lengths,
                uint32_t *ws, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)jpeg_intervals(H, W, k420), (unsigned)N);
    FOSVOS_PROF(k420 ? "k_jpeg_measure_420" : C == 3 ? "k_jpeg_measure" : "k_jpeg_measure_grey", stream, 0.0);
    hipLaunchKernelGGL((k_jpeg<C, false, k420>), grid, dim3(kJpegThreads), 0, st, frames, H, W, qt, ws, (uint8_t *)nullptr,
                       (int64_t)0, (int32_t *)nullptr);
    FOSVOS_LAUNCH_CHECK();
    FOSVOS_PROF(k420 ? "k_jpeg_emit_420" : C == 3 ? "k_jpeg_emit" : "k_jpeg_emit_grey", stream, 0.0);
    hipLaunchKernelGGL((k_jpeg<C, true, k420>), dim3(grid.x + 1, grid.y), dim3(kJpegThreads), 0, st, frames, H, W, qt, ws, out,
                       (int64_t)out_stride, lengths);
    FOSVOS_LAUNCH_CHECK();
    return FOSVOS_OK;
}

// what the two size queries take (anything else: 0 bytes)
bool jpeg_query_ok(int N, int H, int W, int components, int sampling) {
    return N > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535 && (components == 1 || components == 3) &&
           (sampling == 444 || sampling == 420);
}
}  // namespace

extern "C" size_t fosvos_jpeg_capacity_bytes(int N, int H, int W, int components, int sampling) {
    if (!jpeg_query_ok(N, H, W, components, sampling)) return 0;
    return (size_t)jpeg_file_bound(H, W, components, sampling == 420 && components == 3);
}

extern "C" size_t fosvos_jpeg_workspace_bytes(int N, int H, int W, int components, int sampling) {
    if (!jpeg_query_ok(N, H, W, components, sampling)) return 0;
    return (size_t)N * (size_t)jpeg_intervals(H, W, sampling == 420 && components == 3) * sizeof(uint32_t);
}

extern "C" int fosvos_jpeg_encode(const uint8_t *frames, int N, int H, int W, int components, int sampling, int quality,
                                  uint8_t *out, size_t out_stride, int32_t *lengths, void *workspace, size_t workspace_bytes,
                                  int device, void *stream) {
    FOSVOS_REQUIRE(sampling == 444 || sampling == 420, FOSVOS_E_ARG, "jpeg_encode: sampling=%d (444 or 420)", sampling);
    FOSVOS_REQUIRE(components == 1 || components == 3, FOSVOS_E_SHAPE, "jpeg_encode: components=%d (1 grey, 3 BGR)", components);
    FOSVOS_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 65535 && W <= 65535, FOSVOS_E_SHAPE,
                   "jpeg_encode: N=%d H=%d W=%d (each 1..65535)", N, H, W);
    FOSVOS_REQUIRE(quality >= 1 && quality <= 100, FOSVOS_E_ARG, "jpeg_encode: quality=%d (1..100)", quality);
    FOSVOS_REQUIRE(frames && out && lengths && workspace, FOSVOS_E_ARG, "jpeg_encode: null pointer");
    FOSVOS_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)lengths & 3) == 0, FOSVOS_E_ARG,
                   "jpeg_encode: the workspace and the lengths must be 4-byte aligned");
    const bool s420 = sampling == 420 && components == 3;
    const size_t need_cap = (size_t)jpeg_file_bound(H, W, components, s420);
    const size_t need_ws = (size_t)N * (size_t)jpeg_intervals(H, W, s420) * sizeof(uint32_t);
    FOSVOS_REQUIRE(need_cap <= (size_t)INT32_MAX, FOSVOS_E_SHAPE, "jpeg_encode: H=%d W=%d: the size bound %zu B exceeds 2^31 - 1", H,
                   W, need_cap);
    FOSVOS_REQUIRE(out_stride >= need_cap, FOSVOS_E_WORKSPACE, "jpeg_encode: out_stride %zu B a frame < %zu B", out_stride, need_cap);
    FOSVOS_REQUIRE(workspace_bytes >= need_ws, FOSVOS_E_WORKSPACE, "jpeg_encode: workspace %zu B < %zu B", workspace_bytes, need_ws);
    // the tables of the call's quality: the IJG rule over Annex K (jpeg_layout.quant_tables)
    JpegQ qt;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (kQBase[t][i] * scale + 50) / 100;
            qt.q[t][i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    FOSVOS_ENTER(device);
    uint32_t *ws = reinterpret_cast<uint32_t *>(workspace);
    if (s420) return jpeg_launch<3, true>(frames, N, H, W, qt, out, out_stride, lengths, ws, stream);
    return components == 3 ? jpeg_launch<3, false>(frames, N, H, W, qt, out, out_stride, lengths, ws, stream)
                           : jpeg_launch<1, false>(frames, N, H, W, qt, out, out_stride, lengths, ws, stream);
}
