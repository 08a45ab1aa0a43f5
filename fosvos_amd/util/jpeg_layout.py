"""The JPEG layout of the device encoder (csrc/jpeg.hip, fosvos_jpeg_encode), stated in numpy integers: the kernel is
tested byte for byte against ``encode``.  No float touches the data path, so "equal" means equal.

A uint8 [H,W,3] BGR frame (what ``ops.overlay`` writes) or a uint8 [H,W] grey one becomes a baseline sequential JFIF file

    SOI | APP0 (JFIF 1.01, no thumbnail) | DQT table 0 | DQT table 1 (colour) | SOF0 | DHT DC0 | DHT AC0 | DHT DC1 | DHT AC1
    (the last two for colour) | DRI | SOS | interval 0 | RST0 | interval 1 | RST1 | ... | interval n-1 | EOI

* Sampling 4:4:4: an MCU is one 8x8 block per component, Y Cb Cr interleaved; grey has the one component.  H or W that is
  no multiple of 8 replicates the last row / column into the padding.
* Colour: the 16-bit fixed-point rows ``YCC`` (libjpeg's), ``(r*R + g*G + b*B + offset) >> 16``; each row's coefficients
  sum to 65536, 0, 0, so grey in is grey out.  Samples are level-shifted by -128.
* Forward DCT, exact in int32: the Loeffler-Ligtenberg-Moschytz factorisation (12 multiplications a pass) with the 13-bit
  constants ``DCT_CONST[k] = round(2^13 * DCT_EXACT[k])``, in the form the IJG library's slow-integer DCT made the de facto
  definition (``fdct_1d`` below is the statement).  Row pass: outputs carry ``PASS1_BITS`` = 2 extra bits (outputs 0 and 4
  by a left shift, the others by a rounding right shift of 13 - 2); column pass: a rounding right shift of 2 (outputs 0
  and 4) or 13 + 2.  A coefficient F is 8 times the JPEG DCT value: ``FRAC_BITS`` = 3 fractional bits.  Bounds: row pass
  |input| <= 128, sums of 8 <= 1024, products < 2^26; column pass |input| <= 2^13, sums of 4 < 2^15, products < 2^30, sums
  of three products < 2^31.
* Quantisation: the Annex K tables scaled by the IJG quality rule; ``round-half-away(F / 8q)`` as
  ``sign(F) * ((|F| + 4q) // 8q)``.  AC coefficients are clamped to +-1023, the largest the baseline code has a size
  category for (the DCT of 8-bit samples stays below that; the clamp makes it a fact of the integers).  The DC coefficient
  is exactly round(sum(samples) / 8q), |DC| <= 1024, so a DC difference fits size category 11.
* With these definitions the files are byte for byte the ones PIL (libjpeg-turbo) writes with ``quality=q, subsampling=0,
  optimize=False, restart_marker_blocks=RI`` (tests/test_jpeg_layout_cpu.py asserts it on its inputs).
* Entropy coding with the standard tables of Annex K.3: DC as the difference to the previous block of the same component
  (0 at the start of every restart interval), AC as run/size symbols in zigzag order with ZRL (0xF0) for 16 zeros and EOB
  (0x00) unless coefficient 63 is non-zero.  Bits MSB first, 0x00 behind every 0xFF byte, an interval padded to the byte
  with 1-bits.
* Restart interval: ``RI`` MCUs in raster order, so an interval needs nothing from another; RST(k mod 8) stands behind
  interval k except the last.

``subsampling='4:2:0'`` (opt-in, colour only; a grey frame ignores it and gives the grey file above) halves both chroma
planes.  What changes, everything else being as above:

* An MCU is 16x16 pixels and six blocks in the order Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr (``MCU_COMPONENTS_420``); MCUs in
  raster order, ``ceil(W/16) x ceil(H/16)`` of them; SOF0 sampling bytes 0x22 0x11 0x11; the restart interval is ``RI_420``
  = 16 MCUs, again 96 blocks.
* Colour conversion per full-resolution pixel, the rows above.  The luma plane is edge-replicated to ``ceil(W/8)*8 x
  ceil(H/8)*8``.
* Chroma: the full-resolution Cb / Cr planes are edge-replicated to ``16*ceil(W/16)`` columns and to an EVEN number of rows
  (one more row for an odd H, no more); then ``out[y][x] = (p[2y][2x] + p[2y][2x+1] + p[2y+1][2x] + p[2y+1][2x+1] + bias)
  >> 2``, ``bias`` 1 for even x and 2 for odd x (libjpeg's h2v2 downsampler); then the ``ceil(H/2)`` rows of the HALVED plane
  are edge-replicated to ``8*ceil(H/16)`` rows.  So below the picture the last chroma row repeats, which for an even H is the
  mean of rows H-2 and H-1, not row H-1 alone (libjpeg pads the downsampler's output to the MCU row, not its input).
* Dummy luma blocks: a Y block of an MCU beyond ``ceil(W/8)`` block columns (W mod 16 in 1..8) or ``ceil(H/8)`` block rows (H
  mod 16 in 1..8) is not computed from pixels: all its AC coefficients are 0 and its quantised DC is that of the block in
  front of it in the MCU's coding order (libjpeg's coefficient controller; Y(0,0) is never a dummy, so in an MCU with a
  dummy row and column all four DCs are Y(0,0)'s).  It takes part in the DC prediction: its difference is 0.
* DC prediction per component over the blocks of an interval in coding order, so luma runs through the four blocks of an MCU.
* PIL was asked with ``quality=q, subsampling=2, optimize=False, restart_marker_blocks=RI_420`` (the argument counts MCUs)
  and these lines give its files byte for byte on the inputs of tests/jpeg420_cases.py
  (tests/test_jpeg420_layout_cpu.py).  One line had to follow PIL against the first reading of libjpeg: the rows of the
  chroma planes (above); replicating full-resolution rows to the 16-row MCU height differs for every even H that is no
  multiple of 16.
"""
import math
import struct
from collections import namedtuple
from typing import List, Tuple

import numpy as np

RI = 32                 # MCUs per restart interval: 96 blocks in colour, one workgroup of the kernel
RI_420 = 16             # the same with subsampling='4:2:0': 16 MCUs of six blocks
SUBSAMPLINGS = ('4:4:4', '4:2:0')
MCU_COMPONENTS_420 = (0, 0, 0, 0, 1, 2)   # the component of each block of a 4:2:0 MCU, in coding order
FRAC_BITS = 3           # fractional bits of a DCT coefficient before quantisation
AC_MAX = 1023

# (R, G, B, offset) of Y, Cb, Cr
YCC = ((19595, 38470, 7471, 32768),
       (-11059, -21709, 32768, (128 << 16) + 32767),
       (32768, -27439, -5329, (128 << 16) + 32767))

# sqrt(2) * combinations of c_k = cos(k pi / 16), and their 13-bit literals
def _c(k: int) -> float:
    return math.cos(k * math.pi / 16.0)


_R2 = math.sqrt(2.0)
DCT_EXACT = {'0.298631336': _R2 * (-_c(1) + _c(3) + _c(5) - _c(7)), '0.390180644': _R2 * (_c(3) - _c(5)),
             '0.541196100': _R2 * _c(6), '0.765366865': _R2 * (_c(2) - _c(6)), '0.899976223': _R2 * (_c(3) - _c(7)),
             '1.175875602': _R2 * _c(3), '1.501321110': _R2 * (_c(1) + _c(3) - _c(5) - _c(7)),
             '1.847759065': _R2 * (_c(2) + _c(6)), '1.961570560': _R2 * (_c(3) + _c(5)),
             '2.053119869': _R2 * (_c(1) + _c(3) - _c(5) + _c(7)), '2.562915447': _R2 * (_c(1) + _c(3)),
             '3.072711026': _R2 * (_c(1) + _c(3) + _c(5) - _c(7))}
DCT_CONST = {'0.298631336': 2446, '0.390180644': 3196, '0.541196100': 4433, '0.765366865': 6270, '0.899976223': 7373,
             '1.175875602': 9633, '1.501321110': 12299, '1.847759065': 15137, '1.961570560': 16069, '2.053119869': 16819,
             '2.562915447': 20995, '3.072711026': 25172}
CONST_BITS, PASS1_BITS = 13, 2

# zigzag position -> natural index (8 * row + column)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)

# Annex K.1 / K.2 (quality 50), natural order
QBASE = ((16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
          80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
          95, 98, 112, 100, 103, 99),
         (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
          99, 99) + (99,) * 32)

# Annex K.3: (class << 4 | id, the 16 code counts, the symbols in code order); DC0, AC0, DC1, AC1
_AC_SYMBOLS_0 = bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a4344'
    '45464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4'
    'b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')
_AC_SYMBOLS_1 = bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43'
    '4445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2'
    'b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')
HUFFMAN = ((0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
           (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), _AC_SYMBOLS_0),
           (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
           (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _AC_SYMBOLS_1))
ZRL, EOB = 0xF0, 0x00

Symbol = namedtuple('Symbol', 'kind rs component interval')   # kind 'dc' (rs = size category) or 'ac' (rs = run << 4 | size)


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """The two tables (natural order, int32 [64]) of the IJG quality rule."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError('jpeg_layout: quality must be 1..100, got {}'.format(quality))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.asarray(t, dtype=np.int64) * scale + 50) // 100, 1, 255).astype(np.int32) for t in QBASE)


def huffman_codes(counts, symbols) -> dict:
    """symbol -> (code, bits): the canonical assignment of Annex C."""
    out, code, k = {}, 0, 0
    for bits in range(1, 17):
        for _ in range(counts[bits - 1]):
            out[symbols[k]] = (code, bits)
            code += 1
            k += 1
        code <<= 1
    return out


def _check(img) -> np.ndarray:
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.size == 0 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
        raise ValueError('jpeg_layout: a non-empty uint8 [H,W,3] (BGR) or [H,W] array, got {} {}'.format(img.dtype, img.shape))
    if img.shape[0] > 65535 or img.shape[1] > 65535:
        raise ValueError('jpeg_layout: at most 65535 rows and columns, got {}'.format(img.shape))
    return img


def _is_420(components: int, subsampling: str) -> bool:
    """Whether the layout is the 4:2:0 one: a grey frame has one plane and ignores the argument."""
    if subsampling not in SUBSAMPLINGS:
        raise ValueError('jpeg_layout: subsampling must be one of {}, got {!r}'.format(SUBSAMPLINGS, subsampling))
    return subsampling == '4:2:0' and components == 3


def n_mcus(h: int, w: int, subsampling: str = '4:4:4') -> int:
    """MCUs of a frame (``subsampling`` is the layout's: a grey frame is '4:4:4' whatever was asked for)."""
    side = 16 if _is_420(3, subsampling) else 8
    return (-(-h // side)) * (-(-w // side))


def n_intervals(h: int, w: int, subsampling: str = '4:4:4') -> int:
    return -(-n_mcus(h, w, subsampling) // (RI_420 if _is_420(3, subsampling) else RI))


def header_bytes(components: int, subsampling: str = '4:4:4') -> int:
    """SOI .. SOS: 2 + APP0 18 + DQT 69 a table + SOF0 10 + 3 a component + DHT 33 + 183 a table pair + DRI 6 + SOS 8 + 2 a
    component.  The same for both samplings."""
    _is_420(components, subsampling)
    tables = 2 if components == 3 else 1
    return 2 + 18 + 69 * tables + 10 + 3 * components + 216 * tables + 6 + 8 + 2 * components


def capacity(h: int, w: int, components: int, subsampling: str = '4:4:4') -> int:
    """Upper bound of ``len(encode(img))`` for any image of this shape.  A block's 64 coefficients cost at most 26 bits each:
    DC <= 11 code bits + 11 value bits; a non-zero AC <= 16 + 10 (the clamp); a ZRL is 11 bits for 16 zero coefficients, EOB
    <= 4 bits for a zero coefficient 63.  An interval of b blocks is therefore at most 208 b bytes after the padding (208 b is
    whole), at most doubled by the stuffing: 416 bytes a block.  Plus the header, two bytes per interval (RST or EOI).
    4:2:0: the same per block, six blocks for every MCU of the padded 16x16 grid (dummy blocks counted as whole ones)."""
    if components not in (1, 3):
        raise ValueError('jpeg_layout: components must be 1 or 3, got {}'.format(components))
    sampled = _is_420(components, subsampling)
    layout = '4:2:0' if sampled else '4:4:4'
    return header_bytes(components) + 416 * n_mcus(h, w, layout) * (6 if sampled else components) + 2 * n_intervals(h, w, layout)


def _planes(img: np.ndarray) -> np.ndarray:
    """int32 [components, H, W]: Y Cb Cr of a BGR frame, or the grey plane."""
    if img.ndim == 3:
        b, g, r = (img[..., k].astype(np.int32) for k in range(3))
        return np.stack([(cr * r + cg * g + cb * b + off) >> 16 for cr, cg, cb, off in YCC])
    return img.astype(np.int32)[None]


def dummy_blocks(h: int, w: int) -> np.ndarray:
    """bool [MCUs, 6] of the 4:2:0 layout: the Y blocks beyond ceil(W/8) block columns or ceil(H/8) block rows."""
    mh, mw = -(-h // 16), -(-w // 16)
    bh, bw = -(-h // 8), -(-w // 8)
    out = np.zeros((mh, mw, 6), dtype=bool)
    for k in range(4):
        rows = 2 * np.arange(mh) + (k >> 1) >= bh
        cols = 2 * np.arange(mw) + (k & 1) >= bw
        out[:, :, k] = rows[:, None] | cols[None, :]
    return out.reshape(-1, 6)


def blocks(img, subsampling: str = '4:4:4') -> np.ndarray:
    """Level-shifted samples int32 [MCUs, blocks of an MCU, 8, 8] in raster MCU order: one block a component, or with 4:2:0
    the six of ``MCU_COMPONENTS_420`` (a dummy block holds the replicated pixels here; ``coefficients`` replaces it)."""
    img = _check(img)
    h, w = img.shape[:2]
    planes = _planes(img)
    if _is_420(planes.shape[0], subsampling):
        hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
        he = h + (h & 1)
        luma = np.pad(planes[0], ((0, hp - h), (0, wp - w)), mode='edge') - 128
        luma = luma.reshape(hp // 16, 2, 8, wp // 16, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(-1, 4, 8, 8)
        quad = np.pad(planes[1:], ((0, 0), (0, he - h), (0, wp - w)), mode='edge').reshape(2, he // 2, 2, wp // 2, 2).sum(axis=(2, 4))
        bias = 1 + (np.arange(wp // 2, dtype=np.int32) & 1)
        chroma = np.pad((quad + bias) >> 2, ((0, 0), (0, (hp - he) // 2), (0, 0)), mode='edge') - 128
        chroma = chroma.reshape(2, hp // 16, 8, wp // 16, 8).transpose(1, 3, 0, 2, 4).reshape(-1, 2, 8, 8)
        return np.concatenate([luma, chroma], axis=1).astype(np.int32)
    hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
    planes = np.pad(planes, ((0, 0), (0, hp - h), (0, wp - w)), mode='edge') - 128
    c = planes.shape[0]
    return planes.reshape(c, hp // 8, 8, wp // 8, 8).transpose(1, 3, 0, 2, 4).reshape(-1, c, 8, 8)


def fdct_1d(d: np.ndarray, first: bool) -> np.ndarray:
    """One pass of the DCT along the last axis (8 long), int32 in and out; ``first``: the row pass."""
    k = DCT_CONST
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2

    def descale(x, n):
        return (x + (1 << (n - 1))) >> n

    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        o[0], o[4] = descale(t10 + t11, PASS1_BITS), descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * k['0.541196100']
    o[2] = descale(z1 + t13 * k['0.765366865'], n)
    o[6] = descale(z1 - t12 * k['1.847759065'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * k['1.175875602']
    t4, t5, t6, t7 = t4 * k['0.298631336'], t5 * k['2.053119869'], t6 * k['3.072711026'], t7 * k['1.501321110']
    z1, z2 = -z1 * k['0.899976223'], -z2 * k['2.562915447']
    z3, z4 = z5 - z3 * k['1.961570560'], z5 - z4 * k['0.390180644']
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1).astype(np.int32)


def coefficients(img, quality: int = 90, subsampling: str = '4:4:4') -> np.ndarray:
    """Quantised coefficients int32 [MCUs, blocks of an MCU, 64] in zigzag order."""
    s = blocks(img, subsampling)                                              # [m, c, y, x]
    sampled = s.shape[1] == 6
    comps = MCU_COMPONENTS_420 if sampled else tuple(range(s.shape[1]))
    rows = fdct_1d(s, True)                                                   # [m, c, y, u]
    f = fdct_1d(rows.swapaxes(-1, -2), False).swapaxes(-1, -2)                # [m, c, v, u]
    f = f.reshape(s.shape[0], s.shape[1], 64)
    tables = quant_tables(quality)
    q = np.stack([tables[0 if c == 0 else 1] for c in comps]).astype(np.int32)[None] << FRAC_BITS
    mag = (np.abs(f) + (q >> 1)) // q
    out = np.where(f < 0, -mag, mag).astype(np.int32)
    out[..., 1:] = np.clip(out[..., 1:], -AC_MAX, AC_MAX)
    if sampled:
        dummy = dummy_blocks(*np.asarray(img).shape[:2])
        for k in range(1, 4):                                                 # in coding order: a copy may be copied on
            out[dummy[:, k], k, 1:] = 0
            out[dummy[:, k], k, 0] = out[dummy[:, k], k - 1, 0]
    return out[..., list(ZIGZAG)]


def _size(v: int) -> int:
    return int(abs(v)).bit_length()


def _scan(img, quality: int, subsampling: str = '4:4:4'):
    """Per restart interval the list of (kind, rs, component, value bits, number of value bits)."""
    coef = coefficients(img, quality, subsampling)
    n, c = coef.shape[:2]
    comps, ri = (MCU_COMPONENTS_420, RI_420) if c == 6 else (tuple(range(c)), RI)
    out = []
    for first in range(0, n, ri):
        rec, pred = [], [0] * 3
        for m in range(first, min(first + ri, n)):
            for j, k in enumerate(comps):
                z = coef[m, j].tolist()
                d = z[0] - pred[k]
                pred[k] = z[0]
                s = _size(d)
                rec.append(('dc', s, k, (d if d >= 0 else d - 1) & ((1 << s) - 1), s))
                run = 0
                for v in z[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        rec.append(('ac', ZRL, k, 0, 0))
                        run -= 16
                    s = _size(v)
                    rec.append(('ac', run << 4 | s, k, (v if v >= 0 else v - 1) & ((1 << s) - 1), s))
                    run = 0
                if run:
                    rec.append(('ac', EOB, k, 0, 0))
        out.append(rec)
    return out


def symbols(img, quality: int = 90, subsampling: str = '4:4:4') -> List[Symbol]:
    """The symbols the scan encodes, in order (for the tests: does an input reach ZRL, a block without EOB, ...)."""
    return [Symbol(kind, rs, k, i) for i, rec in enumerate(_scan(img, quality, subsampling)) for kind, rs, k, _, _ in rec]


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def header(h: int, w: int, components: int, quality: int, subsampling: str = '4:4:4') -> bytes:
    sampled = _is_420(components, subsampling)
    tables = quant_tables(quality)
    nt = 2 if components == 3 else 1
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(nt):
        out += _segment(0xDB, bytes([t]) + bytes(int(tables[t][z]) for z in ZIGZAG))
    out += _segment(0xC0, struct.pack('>BHHB', 8, h, w, components)
                    + b''.join(bytes([k + 1, 0x22 if sampled and k == 0 else 0x11, 0 if k == 0 else 1])
                               for k in range(components)))
    for tc_th, counts, syms in HUFFMAN[:2 * nt]:
        out += _segment(0xC4, bytes([tc_th]) + bytes(counts) + bytes(syms))
    out += _segment(0xDD, struct.pack('>H', RI_420 if sampled else RI))
    out += _segment(0xDA, bytes([components]) + b''.join(bytes([k + 1, 0x00 if k == 0 else 0x11]) for k in range(components))
                    + b'\x00\x3f\x00')
    assert len(out) == header_bytes(components)
    return out


def encode(img, quality: int = 90, subsampling: str = '4:4:4') -> bytes:
    """The JPEG file of a uint8 [H,W,3] BGR or [H,W] grey array in the layout above."""
    img = _check(img)
    h, w = img.shape[:2]
    components = 3 if img.ndim == 3 else 1
    codes = [huffman_codes(counts, syms) for _, counts, syms in HUFFMAN]
    out = bytearray(header(h, w, components, quality, subsampling))
    scan = _scan(img, quality, subsampling)
    for i, rec in enumerate(scan):
        acc, nbits = 0, 0
        for kind, rs, k, value, vbits in rec:
            code, bits = codes[(0 if k == 0 else 2) + (kind == 'ac')][rs]
            acc = ((acc << bits | code) << vbits) | value
            nbits += bits + vbits
        pad = -nbits % 8
        acc = (acc << pad) | ((1 << pad) - 1)
        data = acc.to_bytes((nbits + pad) // 8, 'big')
        out += data.replace(b'\xff', b'\xff\x00')
        out += bytes([0xFF, 0xD0 + i % 8]) if i + 1 < len(scan) else b'\xff\xd9'
    return bytes(out)


def segments(data: bytes) -> List[Tuple[int, bytes]]:
    """[(marker, payload)] of the segments in front of the scan, SOS included (for the tests)."""
    if data[:2] != b'\xff\xd8':
        raise ValueError('jpeg_layout.segments: no SOI')
    out, at = [], 2
    while True:
        if data[at] != 0xFF:
            raise ValueError('jpeg_layout.segments: no marker at {}'.format(at))
        marker, n = data[at + 1], struct.unpack('>H', data[at + 2:at + 4])[0]
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out


def scan_bytes(data: bytes) -> bytes:
    """The entropy-coded bytes between SOS and EOI (restart markers included)."""
    at = 2
    while data[at + 1] != 0xDA:
        at += 2 + struct.unpack('>H', data[at + 2:at + 4])[0]
    at += 2 + struct.unpack('>H', data[at + 2:at + 4])[0]
    if data[-2:] != b'\xff\xd9':
        raise ValueError('jpeg_layout.scan_bytes: no EOI')
    return data[at:-2]
