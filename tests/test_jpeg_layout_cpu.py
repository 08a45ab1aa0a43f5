"""The JPEG layout of the device encoder as util/jpeg_layout.py states it, with PIL as the independent decoder and PIL's own
encoder (libjpeg-turbo) as the yardstick of fidelity and size.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_cases as C  # noqa: E402
from util import jpeg_layout as J  # noqa: E402


def dht_segments(data):
    return [payload for marker, payload in J.segments(data) if marker == 0xC4]


# ------------------------------------------------------------------------------------------ 1: decoding and headers
@pytest.mark.parametrize("grey", [False, True], ids=["bgr", "grey"])
@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d" % s)
def test_files_decode_and_carry_pils_tables(size, grey):
    from PIL import Image
    import io
    h, w = size
    img = C.picture(h, w, grey)
    for q in C.QUALITIES:
        data = J.encode(img, q)
        mode, got = C.decode(data)
        assert mode == ("L" if grey else "RGB") and got.shape == img.shape
        theirs = C.pil_encode(img, q, J.RI)
        assert Image.open(io.BytesIO(data)).quantization == Image.open(io.BytesIO(theirs)).quantization
        assert dht_segments(data) == dht_segments(theirs) and len(dht_segments(data)) == (2 if grey else 4)
        assert [m for m, _ in J.segments(data)] == [m for m, _ in J.segments(theirs)]
        assert len(J.header(h, w, 1 if grey else 3, q)) == J.header_bytes(1 if grey else 3)
        assert len(data) <= J.capacity(h, w, 1 if grey else 3)


def test_bad_inputs_raise():
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((0, 4), np.uint8), np.zeros((2, 2, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            J.encode(bad)
    for q in (0, 101):
        with pytest.raises(ValueError):
            J.encode(np.zeros((4, 4), np.uint8), q)
    with pytest.raises(ValueError):
        J.capacity(8, 8, 2)


# ------------------------------------------------------------------------------------------ 2: fidelity against PIL's encoder
@pytest.mark.parametrize("grey", [False, True], ids=["bgr", "grey"])
@pytest.mark.parametrize("content", ["smooth", "noise"])
def test_fidelity_and_size_against_pils_own_file(content, grey):
    """PSNR of PIL's decode of our file >= PSNR of PIL's decode of PIL's file - 0.1 dB, and our length within 2 % of PIL's.
    Measured: the integer definitions (colour rows, slow-integer LLM DCT, half-away rounding) are libjpeg's, and the files
    come out byte for byte PIL's - 0.000 dB, 0 bytes - which is asserted as well."""
    img = C.smooth(61, 107, grey) if content == "smooth" else C.noise(61, 107, grey)
    for q in C.QUALITIES:
        ours, theirs = J.encode(img, q), C.pil_encode(img, q, J.RI)
        p_ours, p_theirs = C.psnr(C.decode(ours)[1], img), C.psnr(C.decode(theirs)[1], img)
        print("%s %s q=%d: PSNR %.3f dB (PIL %.3f dB), %d bytes (PIL %d)" % (content, "grey" if grey else "bgr", q, p_ours,
                                                                             p_theirs, len(ours), len(theirs)))
        assert p_ours >= p_theirs - 0.1
        assert abs(len(ours) - len(theirs)) <= 0.02 * len(theirs)
        assert J.scan_bytes(ours) == J.scan_bytes(theirs)
        assert ours == theirs


# ------------------------------------------------------------------------------------------ 3: structure
def restart_markers(data):
    """The RST markers of the scan, in order (a stuffed FF is followed by 00, never by D0..D7)."""
    scan = J.scan_bytes(data)
    return [scan[i + 1] - 0xD0 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]


@pytest.mark.parametrize("grey", [False, True], ids=["bgr", "grey"])
def test_restart_markers_and_capacity(grey):
    comps = 1 if grey else 3
    for (h, w) in C.SIZES + (C.MANY,):
        img = C.picture(h, w, grey)
        n = -(-(-(-h // 8) * -(-w // 8)) // J.RI)
        assert J.n_intervals(h, w) == n
        for q in (50, 100):
            data = J.encode(img, q)
            assert restart_markers(data) == [k % 8 for k in range(n - 1)], (h, w, q)
            assert len(data) <= J.capacity(h, w, comps)
    assert J.n_intervals(*C.MANY) >= 9
    for (h, w) in ((61, 107), C.MANY):
        data = J.encode(C.noise(h, w, grey), 100)
        assert len(data) <= J.capacity(h, w, comps)
        print("noise %dx%d %s at q=100: %d bytes of a capacity of %d" % (h, w, "grey" if grey else "bgr", len(data),
                                                                         J.capacity(h, w, comps)))
        assert C.decode(data)[1].shape == (h, w) + (() if grey else (3,))
    # the bound's terms, by hand: header 629 B in colour (2 + 18 + 2 * 69 + 19 + 2 * 216 + 6 + 14), 416 B a block, 2 B an interval
    assert J.header_bytes(3) == 629 and J.header_bytes(1) == 2 + 18 + 69 + 13 + 216 + 6 + 10
    assert J.capacity(8, 8, 3) == 629 + 3 * 416 + 2 and J.capacity(61, 107, 1) == J.header_bytes(1) + 8 * 14 * 416 + 2 * 4


# ------------------------------------------------------------------------------------------ 4: coverage
@pytest.mark.parametrize("grey", [False, True], ids=["bgr", "grey"])
def test_inputs_reach_the_rare_symbols(grey):
    h, w = C.COVERAGE_SIZE
    comps = 1 if grey else 3
    blocks = 15 * comps
    # a constant image: DC 0, then EOB, and nothing else
    sym = J.symbols(C.constant(h, w, grey, 128), 90)
    assert len(sym) == 2 * blocks and all((s.kind, s.rs) in (("dc", 0), ("ac", J.EOB)) for s in sym)
    # 8x8 blocks alternating 0 / 255 at quality 100: DC size category 11
    sym = J.symbols(C.checker(h, w, grey), 100)
    assert any(s.kind == "dc" and s.rs == 11 for s in sym)
    # the low-amplitude (7,7) cosine: ZRLs, and blocks without EOB
    sym = J.symbols(C.corner_cosine(h, w, grey), 50)
    luma = [s for s in sym if s.component == 0]
    assert sum(s.kind == "ac" and s.rs == J.ZRL for s in luma) == 3 * 15
    assert not any(s.kind == "ac" and s.rs == J.EOB for s in luma)
    assert sum(s.kind == "ac" and s.rs >> 4 == 14 for s in luma) == 15     # 62 zeros = 3 * 16 + 14 in front of coefficient 63
    # noise at quality 100: 16-bit AC codes, and a stuffed FF 00 in the scan
    img = C.noise(h, w, grey)
    sym = J.symbols(img, 100)
    long_codes = [{rs for rs, (_, bits) in J.huffman_codes(counts, syms).items() if bits == 16} for _, counts, syms in J.HUFFMAN]
    assert any(s.kind == "ac" and s.rs in long_codes[1 if s.component == 0 else 3] for s in sym)
    assert b"\xff\x00" in J.scan_bytes(J.encode(img, 100))
    assert {s.interval for s in sym} == {0}                                 # 15 MCUs: one interval
    assert {s.interval for s in J.symbols(C.picture(*C.MANY, grey), 50)} == set(range(13))
    for name, make, q in C.COVERAGE:
        assert C.decode(J.encode(make(h, w, grey), q))[1].shape == img.shape


# ------------------------------------------------------------------------------------------ 5: the literals
def test_dct_literals_equal_their_formula_and_colour_rows_sum():
    assert len(J.DCT_CONST) == 12 and set(J.DCT_CONST) == set(J.DCT_EXACT)
    for name, literal in J.DCT_CONST.items():
        assert abs(J.DCT_EXACT[name] - float(name)) < 1e-9, name           # the name is the value to nine places (one is cut, not rounded)
        assert literal == int(round(2 ** J.CONST_BITS * J.DCT_EXACT[name])), name
    assert [sum(row[:3]) for row in J.YCC] == [65536, 0, 0]
    assert J.YCC[0][3] == 1 << 15 and J.YCC[1][3] == J.YCC[2][3] == (128 << 16) + (1 << 15) - 1
    # the passes are a DCT: against the float definition, within the rounding of the two descales (< 1 of 8 units a pass)
    rng = np.random.default_rng(5)
    s = rng.integers(-128, 128, (4, 1, 8, 8)).astype(np.int32)
    f = J.fdct_1d(J.fdct_1d(s, True).swapaxes(-1, -2), False).swapaxes(-1, -2)
    c = np.array([[(math.sqrt(0.5) if u == 0 else 1.0) / 2.0 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)]
                  for u in range(8)])
    want = 8.0 * np.einsum("vy,mcyx,ux->mcvu", c, s.astype(np.float64), c)
    assert np.abs(f - want).max() < 2.0
    assert sorted(J.ZIGZAG) == list(range(64)) and J.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2)
    assert [t.tolist() for t in J.quant_tables(50)] == [list(b) for b in J.QBASE]
    assert all(int(t.min()) == 1 and int(t.max()) == 1 for t in J.quant_tables(100))
    assert all(int(t.max()) == 255 for t in J.quant_tables(1))
