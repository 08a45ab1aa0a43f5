"""Seeded inputs of the JPEG decoder tests, shared by the CPU test of the definition (tests/test_jpeg_read_cpu.py), the
sanitizer run of the entropy decoder on the host (tests/test_jpeg_entropy_host_cpu.py) and the GPU test of the kernels
(tests/test_gpu_jpeg_decode.py): files PIL writes of the frames of tests/jpeg_cases.py, and three damaged ones."""
import functools
import io
import struct

import numpy as np
from PIL import Image

import jpeg_cases as J
from util.jpeg_layout import HUFFMAN, huffman_codes

QUALITIES = (1, 50, 90, 100)
SIZES = J.SIZES + ((5, 5), (16, 5))
SUBSAMPLING = {"444": 0, "420": 2}


def pil_file(img, quality, sub="444", restart=0, optimize=False, **more):
    """PIL's file of a uint8 [H,W,3] BGR or [H,W] grey frame; ``restart`` counts MCUs."""
    b = io.BytesIO()
    im = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[..., ::-1]))
    im.save(b, "JPEG", quality=quality, subsampling=SUBSAMPLING[sub], optimize=optimize, restart_marker_blocks=restart, **more)
    return b.getvalue()


def pil_pixels(data):
    """PIL's decode: uint8 [H,W,3] BGR or [H,W]."""
    return J.decode(data)[1]


@functools.lru_cache(maxsize=None)
def cases():
    """[(id, file bytes)]"""
    out = []
    for h, w in SIZES:
        for q in QUALITIES:
            for kind in ("grey", "444", "420"):
                if kind == "420" and w < 5:
                    continue
                img = J.picture(h, w, kind == "grey")
                for ri in (0, 16):
                    out.append(("picture_%dx%d_%s_q%d_ri%d" % (h, w, kind, q, ri), pil_file(img, q, "444" if kind == "grey" else kind, ri)))
    for name, make, q in J.COVERAGE:
        for kind in ("grey", "444", "420"):
            out.append(("%s_%s_q%d" % (name, kind, q), pil_file(make(*J.COVERAGE_SIZE, kind == "grey"), q, "444" if kind == "grey" else kind)))
    for name, make, q in (("picture", J.picture, 90), ("noise", J.noise, 100)):
        img = make(*J.MANY)
        out.append(("%s_120x214_420_q%d_ri0" % (name, q), pil_file(img, q, "420")))
        out.append(("%s_120x214_420_q%d_ri16" % (name, q), pil_file(img, q, "420", 16)))
    # 15 x 27 MCUs in 13 intervals: the markers go round RST0..RST7 and on
    out.append(("picture_120x214_444_q90_ri32", pil_file(J.picture(*J.MANY), 90, "444", 32)))
    out.append(("picture_120x214_420_q90_optimize", pil_file(J.picture(*J.MANY), 90, "420", optimize=True)))
    return tuple(out)


def big_file():
    """One 480x854 4:2:0 frame at quality 92 (a DAVIS frame's shape)."""
    return pil_file(J.picture(480, 854), 92, "420")


# ---------------------------------------------------------------------------------------------- byte edits
def segments_of(data):
    """[(marker, offset of the 0xFF, payload offset, payload length)] up to and including SOS."""
    out, at = [], 2
    while True:
        marker, n = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        out.append((marker, at, at + 4, n - 2))
        at += 2 + n
        if marker == 0xDA:
            return out


def scan_start(data):
    s = segments_of(data)[-1]
    return s[2] + s[3]


def _bits(values):
    """[(value, bits)] -> bytes, padded with 1-bits, stuffed."""
    acc, n = 0, 0
    for v, b in values:
        acc, n = (acc << b) | v, n + b
    pad = -n % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    return acc.to_bytes((n + pad) // 8, "big").replace(b"\xff", b"\xff\x00")


def damaged_cut():
    """A scan cut in half (the EOI kept): status 1."""
    data = pil_file(J.picture(33, 47), 90, "444")
    at = scan_start(data)
    return data[:at + (len(data) - 2 - at) // 2] + b"\xff\xd9"


def damaged_code():
    """The luma AC table replaced by a shorter well-formed code (two symbols of one and two bits: the prefix 11 is
    unassigned), so that the stream runs into a prefix without a code: status 2."""
    data = pil_file(J.picture(33, 47, True), 90, "444")
    out = bytearray(data[:2])
    for marker, at, p, n in segments_of(data):
        seg = data[at:p + n]
        if marker == 0xC4 and data[p] == 0x10:
            payload = bytes([0x10, 1, 1] + [0] * 14 + [0x00, 0x01])
            seg = b"\xff\xc4" + struct.pack(">H", len(payload) + 2) + payload
        out += seg
    return bytes(out + data[scan_start(data):])


def damaged_run():
    """A grey 8x8 file whose scan is written by hand with the standard tables: DC 0, then the AC symbols 0xF0 0xF0 0xF0
    0xF1 - run 48 + 15 from position 1 puts the coefficient at position 64: status 3."""
    data = pil_file(J.constant(8, 8, True), 90, "444")
    _, counts, syms = HUFFMAN[1]                 # Annex K.3.2 luma AC; luma DC size 0 is the code 00
    codes = huffman_codes(counts, syms)
    zrl, f1 = codes[0xF0], codes[0xF1]
    scan = _bits([(0, 2), zrl, zrl, zrl, f1, (1, 1)])
    return data[:scan_start(data)] + scan + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def damaged():
    """[(id, file bytes, the status the definition states)]"""
    return (("cut", damaged_cut(), 1), ("code", damaged_code(), 2), ("run", damaged_run(), 3))
