// The entropy decoder of the device JPEG decoder (fosvos_amd/csrc/jpeg_entropy.h) on the CPU, for the sanitizers:
// tests/test_jpeg_entropy_host_cpu.py builds this file with -fsanitize=address,undefined and runs it over good and damaged
// files.  The host form of the kernel's wave: Src is the segment's bytes behind a bounds check, Sink loops over the 64
// "lanes" of a block.
//
//   jpeg_entropy_main IN OUT [IN OUT ...]
//   IN : int32 H, W, components, s420, n_bytes, n_segments; 2384 bytes of tables; n_bytes of the file; int32 [n_segments][4]
//        rows (byte offset, byte length, first MCU, MCU count)
//   OUT: int32 status; int16 [blocks][64]
#define FOSVOS_HD
#include "../../fosvos_amd/csrc/jpeg_entropy.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace fosvos_jpegd;

struct HostBytes {
    const uint8_t *p;
    uint32_t len;
    uint32_t get(uint32_t i) { return i < len ? p[i] : 0; }
};

struct HostBlock {
    int16_t *coef;
    int16_t lanes[64];
    void put(int zigzag, int16_t v) { lanes[zigzag_natural(zigzag)] = v; }
    void store(int index) {
        for (int lane = 0; lane < 64; ++lane) coef[(size_t)index * 64 + lane] = lanes[lane], lanes[lane] = 0;
    }
    void zero(int index) {
        memset(lanes, 0, sizeof(lanes));
        store(index);
    }
};

static int run(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    int32_t head[6];
    if (fread(head, 4, 6, f) != 6) return 2;
    const int H = head[0], W = head[1], comps = head[2], s420 = head[3], n_bytes = head[4], n_segs = head[5];
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (comps != 1 && comps != 3) || n_bytes < 0 || n_segs < 0) return 2;
    std::vector<uint8_t> tables(sizeof(FileTables)), bytes((size_t)n_bytes);
    std::vector<int32_t> segs((size_t)n_segs * 4);
    if (fread(tables.data(), 1, tables.size(), f) != tables.size()) return 2;
    if (n_bytes && fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 2;
    if (n_segs && fread(segs.data(), 4, segs.size(), f) != segs.size()) return 2;
    fclose(f);
    FileTables ft;
    memcpy(&ft, tables.data(), sizeof(ft));
    const Geometry g = geometry(H, W, comps, s420);
    std::vector<Huff> huff(kSlots);
    for (int s = 0; s < kSlots; ++s) {
        huff_codes(ft.dht[s], huff[s]);
        huff_fill(ft.dht[s], huff[s], 0, 1);
        huff_lut(huff[s], 0, 1);
    }
    std::vector<int16_t> coef((size_t)g.blocks * 64, 0);
    int32_t status = 0;
    for (int s = 0; s < n_segs; ++s) {
        const int64_t off = segs[4 * s], len = segs[4 * s + 1], first = segs[4 * s + 2], count = segs[4 * s + 3];
        int st = kBytes;
        if (off >= 0 && len >= 0 && off + len <= n_bytes && first >= 0 && count >= 0 && first + count <= (int64_t)g.mh * g.mw) {
            HostBytes src{bytes.data() + off, (uint32_t)len};
            HostBlock sink;
            sink.coef = coef.data();
            memset(sink.lanes, 0, sizeof(sink.lanes));
            st = decode_segment(src, (uint32_t)len, huff.data(), ft.dc_slot, ft.ac_slot, g, (int)first, (int)count, sink);
        }
        if (st != 0 && (status == 0 || st < status)) status = st;
    }
    f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(&status, 4, 1, f);
    fwrite(coef.data(), 2, coef.size(), f);
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3 || (argc & 1) == 0) {
        fprintf(stderr, "usage: %s IN OUT [IN OUT ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 1 < argc; i += 2) {
        const int rc = run(argv[i], argv[i + 1]);
        if (rc) {
            fprintf(stderr, "%s: cannot read or write (%d)\n", argv[i], rc);
            return rc;
        }
    }
    return 0;
}
