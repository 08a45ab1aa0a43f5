// The entropy decoder of fosvos_jpeg_decode (jpeg_decode.hip) as one host/device function: baseline Huffman decode of one
// restart interval ("segment") into coefficient blocks, as util/jpeg_read.py states it.  The kernel runs it with one wave per
// segment on wave-uniform state; tests/host/jpeg_entropy_main.cpp runs the same text on the CPU under the sanitizers
// (FOSVOS_HD defined away), which is why nothing here knows about lanes: where the bytes come from (Src) and where a
// block's coefficients go (Sink) are the caller's.
//
// Safety, for any bytes and any tables:
//   * the byte stream is read through Src::get(i) alone, which returns 0 for i >= its length;
//   * a symbol that consumed a bit beyond the last byte ends the segment with status 1;
//   * every coefficient position is checked before it is used (status 3), every table index is masked into the table;
//   * every iteration of every loop consumes at least one bit or ends the segment, and the MCU loop is bounded by the count
//     the caller clamped to the file's grid.
#pragma once
#include <stdint.h>

#ifndef FOSVOS_HD
#define FOSVOS_HD __host__ __device__
#endif
// The decoder's state is the same in every lane of the wave; telling the compiler so keeps it in scalar registers.
#if defined(__HIP_DEVICE_COMPILE__)
#define FOSVOS_WAVE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define FOSVOS_WAVE_UNIFORM(x) ((uint32_t)(x))
#endif

namespace fosvos_jpegd {

constexpr int kOk = 0, kBytes = 1, kCode = 2, kIndex = 3, kRange = 5;
constexpr int kLutBits = 9;
constexpr int kSlots = 8;       // Huffman tables of a file: slot = class * 4 + id
constexpr int kDhtBytes = 272;  // 16 counts + up to 256 symbols, as they stand in the file (zero-filled behind)

// zigzag position -> natural index (a sink's business: the kernel's lanes each know their own position instead)
FOSVOS_HD inline int zigzag_natural(int k) {
    constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// What travels per file beside its bytes (host-built, 8-byte multiple)
struct FileTables {
    uint8_t quant[3][64];             // per component, natural order
    uint8_t dc_slot[3], ac_slot[3];   // per component: the slot of its DC / AC table
    uint8_t pad[2];
    int32_t seg_first, seg_count;     // the file's rows of the segment table
    uint8_t dht[kSlots][kDhtBytes];
};
static_assert(sizeof(FileTables) == 192 + 8 + 8 + kSlots * kDhtBytes, "FileTables is packed by the host");

// One table ready for decoding: a first-level lookup of kLutBits bits (length << 8 | symbol, 0: longer code or none) and
// the canonical walk (first code, symbol offset, count per length) for what it leaves.
struct Huff {
    uint16_t lut[1 << kLutBits];
    uint32_t first[17];
    uint16_t off[17];
    uint8_t count[17];
    uint8_t sym[256];
};

// length << 8 | symbol of the code the 16-bit prefix starts with, among the lengths lo..hi; 0: none
FOSVOS_HD inline uint32_t huff_walk(const Huff &h, uint32_t peek16, int lo, int hi) {
    for (int l = lo; l <= hi; ++l) {
        const uint32_t idx = (peek16 >> (16 - l)) - h.first[l];  // wraps to a large number below the first code
        if (idx < h.count[l]) return (uint32_t)l << 8 | h.sym[(h.off[l] + idx) & 255];
    }
    return 0;
}

// Step 1 (one thread): the walk's tables from the 16 counts.  Step 2 (thread `lane` of `lanes`): symbols and lookup.
FOSVOS_HD inline void huff_codes(const uint8_t *dht, Huff &h) {
    uint32_t code = 0, off = 0;
    h.first[0] = 0, h.off[0] = 0, h.count[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        h.first[l] = code;
        h.off[l] = (uint16_t)off;
        h.count[l] = dht[l - 1];
        code = (code + dht[l - 1]) << 1;
        off += dht[l - 1];
    }
}
FOSVOS_HD inline void huff_fill(const uint8_t *dht, Huff &h, int lane, int lanes) {
    for (int i = lane; i < 256; i += lanes) h.sym[i] = dht[16 + i];
}
FOSVOS_HD inline void huff_lut(Huff &h, int lane, int lanes) {  // after huff_fill is visible
    for (int i = lane; i < (1 << kLutBits); i += lanes) h.lut[i] = (uint16_t)huff_walk(h, (uint32_t)i << (16 - kLutBits), 1, kLutBits);
}

// Block grids of a file: component by component, each in raster order of its padded grid
struct Geometry {
    int comps, s420;
    int mh, mw;              // MCU grid
    int first[3], cols[3];   // per component: first block, block columns
    int blocks;              // of a file
    int mcu_blocks;          // 1, 3 or 6
};
FOSVOS_HD inline Geometry geometry(int H, int W, int comps, int s420) {
    Geometry g;
    g.comps = comps, g.s420 = (s420 && comps == 3) ? 1 : 0;
    const int side = g.s420 ? 16 : 8;
    g.mh = (H + side - 1) / side, g.mw = (W + side - 1) / side;
    int first = 0;
    for (int c = 0; c < 3; ++c) {
        const int f = (g.s420 && c == 0) ? 2 : 1;
        g.first[c] = first, g.cols[c] = f * g.mw;
        if (c < comps) first += f * g.mh * f * g.mw;
    }
    g.blocks = first;
    g.mcu_blocks = g.s420 ? 6 : comps;
    return g;
}
// block j of MCU (my, mx): its component and its index in the file's blocks
FOSVOS_HD inline int mcu_block(const Geometry &g, int my, int mx, int j, int &comp) {
    if (g.s420) {
        if (j < 4) {
            comp = 0;
            return (2 * my + (j >> 1)) * g.cols[0] + 2 * mx + (j & 1);
        }
        comp = j - 3;
        return g.first[comp] + my * g.cols[comp] + mx;
    }
    comp = j;
    return g.first[j] + my * g.cols[j] + mx;
}

// The bit reader: MSB first, stuffing removed in the refill (a byte behind 0xFF is skipped: inside a segment it is 0x00)
template <class Src>
struct Bits {
    Src &src;
    uint32_t len, pos;
    uint64_t acc;
    int nb;        // valid bits in acc
    int phantom;   // how many of them lie beyond the last byte
    FOSVOS_HD Bits(Src &s, uint32_t n) : src(s), len(n), pos(0), acc(0), nb(0), phantom(0) {}
    FOSVOS_HD void refill() {  // to at least 32 bits
        while (nb < 32) {
            uint32_t c = 0;
            if (pos < len) {
                c = src.get(pos++);
                if (c == 0xFF) ++pos;
            } else {
                phantom += 8;
            }
            acc = acc << 8 | c;
            nb += 8;
        }
    }
    FOSVOS_HD uint32_t peek16() const { return (uint32_t)(acc >> (nb - 16)) & 0xFFFFu; }
    FOSVOS_HD uint32_t take(int n) {  // n <= 16 <= nb
        nb -= n;
        return (uint32_t)(acc >> nb) & ((1u << n) - 1u);
    }
    FOSVOS_HD bool overrun() const { return nb < phantom; }
};

// One segment: n_mcu MCUs from first_mcu on (both already clamped into the grid).  Sink: put(zigzag position, value) into the
// current block (all zero after store / zero / at the start), store(block index) writes it out and clears it,
// zero(block index) drops it and writes a zero block.  Returns the status; the block an error falls in and all later ones of the segment are zero.
template <class Src, class Sink>
FOSVOS_HD inline int decode_segment(Src &src, uint32_t len, const Huff *huff, const uint8_t *dc_slot, const uint8_t *ac_slot,
                                    const Geometry &g, int first_mcu, int n_mcu, Sink &sink) {
    Bits<Src> bits(src, len);
    uint32_t pred0 = 0, pred1 = 0, pred2 = 0;
    int my = first_mcu / g.mw, mx = first_mcu - my * g.mw;
    int status = kOk, m = 0, j = 0;
    for (; m < n_mcu && status == kOk; ++m) {
        for (j = 0; j < g.mcu_blocks && status == kOk; ++j) {
            int comp;
            const int index = mcu_block(g, my, mx, j, comp);
            const Huff *h = &huff[dc_slot[comp] & (kSlots - 1)];
            int k = 0;
            while (k < 64) {
                bits.refill();
                const uint32_t peek = bits.peek16();
                uint32_t e = h->lut[peek >> (16 - kLutBits)];
                if (e == 0) e = huff_walk(*h, peek, kLutBits + 1, 16);
                e = FOSVOS_WAVE_UNIFORM(e);
                if (e == 0) {
                    status = kCode;
                    break;
                }
                bits.take((int)(e >> 8));
                const int rs = (int)(e & 255);
                const int s = rs & 15;  // a DC symbol is its size (the host admits none above 15)
                int32_t v = 0;
                if (s) {
                    v = (int32_t)bits.take(s);
                    if (v < (1 << (s - 1))) v -= (1 << s) - 1;
                }
                if (bits.overrun()) {
                    status = kBytes;
                    break;
                }
                if (k == 0) {
                    uint32_t &pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
                    pred += (uint32_t)v;
                    v = (int32_t)pred;
                    h = &huff[ac_slot[comp] & (kSlots - 1)];
                } else if (s == 0) {
                    if (rs != 0xF0) break;  // end of block
                    k += 16;
                    if (k > 63) {
                        status = kIndex;
                        break;
                    }
                    continue;
                } else {
                    k += rs >> 4;
                    if (k > 63) {
                        status = kIndex;
                        break;
                    }
                }
                sink.put(k, (int16_t)(uint16_t)(uint32_t)v);
                ++k;
            }
            if (status == kOk) sink.store(index);
            else sink.zero(index);
        }
        if (status == kOk && ++mx == g.mw) mx = 0, ++my;
    }
    // what the error left: the rest of its MCU, then the MCUs behind it (m and j stand behind the failing block)
    if (status != kOk) {
        int comp;
        for (; j < g.mcu_blocks; ++j) sink.zero(mcu_block(g, my, mx, j, comp));
        if (++mx == g.mw) mx = 0, ++my;
        for (; m < n_mcu; ++m) {
            for (j = 0; j < g.mcu_blocks; ++j) sink.zero(mcu_block(g, my, mx, j, comp));
            if (++mx == g.mw) mx = 0, ++my;
        }
    }
    return status;
}

}  // namespace fosvos_jpegd
