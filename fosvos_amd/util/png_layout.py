"""The PNG layout of the device encoder (csrc/png.hip, fosvos_png_encode), stated in plain numpy / stdlib: the kernel is
tested byte for byte against ``encode``, and the host path of ``experiment_helper.test_fast`` writes its files with it.

An 8-bit greyscale image uint8 [H,W] becomes

    signature | IHDR | IDAT(segment 0) | IDAT(segment 1) | ... | IDAT(final) | IEND

* The filtered stream is the H rows of (W+1) bytes a PNG decoder expects: filter byte 0 (None), then the row.
* The stream is cut into SEGMENTS of ``SEG_BYTES`` consecutive bytes (the last one shorter).  With filter None the rows
  mean nothing to the compressor, so a segment is a byte count, not a row count: every segment is the same amount of work,
  fits the kernel's LDS whatever the width, and never exceeds the 65535 bytes of one stored block.
* A segment is ONE deflate block (BFINAL = 0) with the fixed Huffman code.  A maximal run of L equal bytes inside the
  segment is: its first byte as a literal, then the remaining L-1 bytes as distance-1 matches of length 258 while 258 are
  left, then one match of the rest if the rest is >= 3, else the rest (1 or 2 bytes) as literals.  Runs stop at the segment
  end.  Huffman codes go MSB first, extra bits LSB first (RFC 1951).
* After the end-of-block code comes an empty stored block (3 header bits, zero padding to the byte, 00 00 FF FF), so the
  segment ends on a byte boundary and the segments concatenate bytewise.
* Where that fixed form would be LONGER than a stored block of the same bytes (5 + n bytes), the stored block is emitted.
* Every segment is an IDAT chunk of its own (length, 'IDAT', data, CRC-32); the first one starts with the zlib header
  78 01.  A last IDAT holds the final empty fixed block (03 00) and the Adler-32 of the whole filtered stream.

CRC-32 and Adler-32 come from ``zlib`` here; the kernel computes its own.

``encode(img, huffman='fitted')`` (opt-in) adds a third form of a segment: a dynamic-Huffman block (BTYPE = 10) whose
literal/length code is fitted to the segment.  Same segments, same tokens, same chunks; only the codes differ.
* The histogram of the segment's token symbols (literals 0..255, length symbols 257..285) plus ONE end-of-block symbol 256.
* Code lengths: the two-queue Huffman construction.  The used symbols sorted by (count, symbol) form the leaf queue, merged
  nodes join a second queue in the order they are made; each step takes the two lightest heads, the first and the second
  pick alike: the leaf where the leaf's weight <= the node's (a tie goes to the leaf), else the node.  A symbol's length is its
  depth.  While the deepest exceeds 15, every non-zero count c becomes (c + 1) // 2 and the tree is rebuilt.  A Huffman
  tree of >= 2 symbols is a complete code (Kraft sum exactly 1).  Codes are canonical (RFC 1951 3.2.2).
* HLIT covers the symbols up to the last used one (at least 257 codes).  HDIST = 0: the single distance code 0 has length
  1, so a match's distance (always 1) costs one 0 bit instead of five.
* The code-length code is NOT fitted: HCLEN = 19 and the complete assignment ``CL_LENGTHS`` (thirteen symbols of 4 bits,
  six of 5), written in the order ``CL_ORDER``.  The block header is therefore 3 + 5 + 5 + 4 + 57 = 74 constant-length bits.
* The sequence of the HLIT + 257 literal/length lengths followed by the one distance length, greedy from the left: a
  non-zero length is its own symbol (symbol 16 is never used); a maximal run of z zeros is symbol 18 (11..138 zeros, 7 extra
  bits) while at least 11 are left, then symbol 17 (3..10, 3 extra bits) if at least 3 are left, else the 1 or 2 zeros as
  symbol 0.
* End of block, the empty stored block and ``00 00 FF FF`` as in the fixed form.
* Per segment the shortest of {fitted, fixed, stored} is written; fixed or stored, by the rule above, unless fitted is
  strictly shorter.  So no segment, and no file, is longer than with ``huffman='fixed'``, and ``max_file_bytes`` holds.
"""
import struct
import zlib
from typing import List, Tuple

import numpy as np

SEG_BYTES = 4096
SIGNATURE = b'\x89PNG\r\n\x1a\n'
ZLIB_HEADER = b'\x78\x01'
SYNC_TAIL = b'\x00\x00\xff\xff'
MAX_MATCH = 258
N_LITLEN = 286                             # literal/length symbols 0..285
END_OF_BLOCK = 256
MAX_CODE_BITS = 15
MAX_ZERO_RUN = 138
HUFFMAN_MODES = ('fixed', 'fitted')
# the fixed code-length code of the fitted form: bits of code-length symbol 0..18 (13/16 + 6/32 = 1); the lengths 11..15 and
# the never-used repeat symbol 16 take the long codes
CL_LENGTHS = (4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 4, 4)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)   # RFC 1951 3.2.7
FITTED_HEADER_BITS = 3 + 5 + 5 + 4 + 3 * 19


def n_segments(h: int, w: int) -> int:
    return -(-(h * (w + 1)) // SEG_BYTES)


def max_file_bytes(h: int, w: int) -> int:
    """Upper bound of ``len(encode(img))`` for any uint8 [h,w] image: no segment is longer than its stored form (5 + n
    bytes), so the file is at most signature 8 + IHDR 25 + zlib header 2 + the n = h (w+1) filtered bytes + 17 bytes per
    segment (12 of the chunk, 5 of the stored block header) + the final IDAT 18 + IEND 12."""
    return 8 + 25 + 2 + h * (w + 1) + 17 * n_segments(h, w) + 18 + 12


def filtered_stream(img: np.ndarray) -> np.ndarray:
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.size == 0:
        raise ValueError('png_layout: a non-empty uint8 [H,W] array, got {} {}'.format(img.dtype, img.shape))
    h, w = img.shape
    rows = np.zeros((h, w + 1), dtype=np.uint8)
    rows[:, 1:] = img
    return rows.reshape(-1)


def _reverse_bits(code: np.ndarray, nbits: np.ndarray, width: int = 9) -> np.ndarray:
    out = np.zeros_like(code)
    for k in range(width):
        take = nbits > k
        out[take] |= ((code[take] >> (nbits[take] - 1 - k)) & 1) << k
    return out


def _parse(seg: np.ndarray):
    """(is_literal, is_match, match length) per byte position of one segment, by the run rule of the layout."""
    n = seg.size
    idx = np.arange(n, dtype=np.int64)
    start = np.ones(n, dtype=bool)
    start[1:] = seg[1:] != seg[:-1]
    starts = np.flatnonzero(start)
    ends = np.append(starts[1:], n)
    run = np.cumsum(start) - 1
    s, e = starts[run], ends[run]          # the run [s, e) each position belongs to
    k = idx - s                            # offset inside the run
    rem = e - s - 1                        # bytes of the run behind its first one
    j = k - 1                              # offset inside that remainder
    q, r = rem // MAX_MATCH, rem % MAX_MATCH
    in_rem = (k > 0) & (rem >= 3)
    blk, off = j // MAX_MATCH, j % MAX_MATCH
    full = in_rem & (blk < q)
    tail = in_rem & (blk == q)
    is_match = (full | (tail & (r >= 3))) & (off == 0)
    covered = (full | (tail & (r >= 3))) & (off != 0)
    is_literal = ~is_match & ~covered
    length = np.where(full, MAX_MATCH, r)
    return is_literal, is_match, length


def _length_symbols(length: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(symbol 257..285, number of extra bits, extra bits) of match lengths 3..258."""
    lm = length - 3
    eb = np.where(lm < 8, 0, np.floor(np.log2(np.maximum(lm, 1))).astype(np.int64) - 2)
    sym = np.where(lm < 8, 257 + lm, 261 + 4 * eb + ((lm >> eb) & 3))
    extra = lm & ((1 << eb) - 1)
    is258 = lm == MAX_MATCH - 3
    return np.where(is258, 285, sym), np.where(is258, 0, eb), np.where(is258, 0, extra)


def segment_tokens(seg: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(code, nbits) per byte position of one segment: the bits the position contributes to the fixed-Huffman block, LSB
    first, 0 bits where the byte is covered by a match that started earlier."""
    seg = np.asarray(seg, dtype=np.uint8)
    n = seg.size
    is_literal, is_match, length = _parse(seg)

    code = np.zeros(n, dtype=np.int64)
    nbits = np.zeros(n, dtype=np.int64)
    v = seg.astype(np.int64)
    lit_code = np.where(v < 144, 0x30 + v, 0x190 + v - 144)
    lit_bits = np.where(v < 144, 8, 9)
    code[is_literal] = _reverse_bits(lit_code[is_literal], lit_bits[is_literal])
    nbits[is_literal] = lit_bits[is_literal]

    sym, eb, extra = _length_symbols(length[is_match])
    sym_code = np.where(sym < 280, sym - 256, 0xC0 + sym - 280)
    sym_bits = np.where(sym < 280, 7, 8)
    code[is_match] = _reverse_bits(sym_code, sym_bits) | (extra << sym_bits)
    nbits[is_match] = sym_bits + eb + 5    # + the 5-bit distance code 0 (distance 1), all zeros
    return code, nbits


def segment_symbols(seg: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(symbol, number of extra bits, extra bits) per byte position of one segment: the literal/length symbol of the token
    that starts there (a literal 0..255 or a length symbol 257..285), -1 where an earlier match covers the byte."""
    seg = np.asarray(seg, dtype=np.uint8)
    is_literal, is_match, length = _parse(seg)
    sym = np.full(seg.size, -1, dtype=np.int64)
    eb = np.zeros(seg.size, dtype=np.int64)
    extra = np.zeros(seg.size, dtype=np.int64)
    sym[is_literal] = seg[is_literal]
    sym[is_match], eb[is_match], extra[is_match] = _length_symbols(length[is_match])
    return sym, eb, extra


def segment_histogram(seg: np.ndarray) -> np.ndarray:
    """Counts of the literal/length symbols 0..285 of one segment's tokens, the end of block (once) included."""
    sym = segment_symbols(seg)[0]
    counts = np.bincount(sym[sym >= 0], minlength=N_LITLEN).astype(np.int64)
    counts[END_OF_BLOCK] += 1
    return counts


def huffman_depths(counts) -> np.ndarray:
    """Depth of every symbol in the two-queue Huffman tree of ``counts`` (0 for a count of 0); at least two used symbols.
    Leaves in the order (count, symbol); of a leaf and a merged node of equal weight the leaf is taken first."""
    counts = [int(c) for c in counts]
    order = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    m = len(order)
    if m < 2:
        raise ValueError('png_layout.huffman_depths: at least two used symbols, got {}'.format(m))
    lw = [counts[s] for s in order]
    iw, lpar, ipar = [], [0] * m, []
    li = ii = 0
    for k in range(m - 1):
        w = 0
        for _pick in range(2):
            if li < m and (ii >= len(iw) or lw[li] <= iw[ii]):
                lpar[li], w, li = k, w + lw[li], li + 1
            else:
                ipar[ii], w, ii = k, w + iw[ii], ii + 1
        iw.append(w)
        ipar.append(-1)
    idepth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        idepth[k] = idepth[ipar[k]] + 1
    depths = np.zeros(len(counts), dtype=np.int64)
    for i, s in enumerate(order):
        depths[s] = idepth[lpar[i]] + 1
    return depths


def huffman_lengths(counts, max_bits: int = MAX_CODE_BITS) -> np.ndarray:
    """Code lengths of ``counts``: the tree's depths, the counts halved (rounding up) and the tree rebuilt while it is deeper
    than ``max_bits``."""
    counts = np.asarray(counts, dtype=np.int64).copy()
    while True:
        depths = huffman_depths(counts)
        if depths.max() <= max_bits:
            return depths
        counts = (counts + 1) // 2


def canonical_codes(lengths) -> np.ndarray:
    """The canonical Huffman codes (MSB first, as numbers) of code lengths, RFC 1951 3.2.2."""
    lengths = np.asarray(lengths, dtype=np.int64)
    bl_count = np.bincount(lengths, minlength=MAX_CODE_BITS + 2)
    bl_count[0] = 0
    code, next_code = 0, [0] * (len(bl_count) + 1)
    for bits in range(1, len(bl_count)):
        code = (code + int(bl_count[bits - 1])) << 1
        next_code[bits] = code
    codes = np.zeros(lengths.size, dtype=np.int64)
    for s in range(lengths.size):
        if lengths[s]:
            codes[s] = next_code[lengths[s]]
            next_code[lengths[s]] += 1
    return codes


def code_length_sequence(lengths) -> List[Tuple[int, int, int]]:
    """[(code-length symbol, extra bits, number of extra bits)] of a sequence of code lengths, by the greedy rule of the
    layout."""
    lengths = [int(v) for v in lengths]
    out, i = [], 0
    while i < len(lengths):
        if lengths[i]:
            out.append((lengths[i], 0, 0))
            i += 1
            continue
        z = 0
        while i + z < len(lengths) and lengths[i + z] == 0:
            z += 1
        i += z
        while z >= 11:
            t = min(z, MAX_ZERO_RUN)
            out.append((18, t - 11, 7))
            z -= t
        if z >= 3:
            out.append((17, z - 3, 3))
            z = 0
        out.extend([(0, 0, 0)] * z)
    return out


def fitted_lengths(seg: np.ndarray) -> np.ndarray:
    """The 286 literal/length code lengths of one segment's fitted block."""
    return huffman_lengths(segment_histogram(seg))


def segment_data_fitted(seg: np.ndarray) -> bytes:
    """Deflate bytes of one segment in the fitted form: the dynamic-Huffman block, then the empty stored block."""
    seg = np.asarray(seg, dtype=np.uint8)
    sym, eb, extra = segment_symbols(seg)
    lengths = fitted_lengths(seg)
    codes = _reverse_bits(canonical_codes(lengths), lengths, MAX_CODE_BITS)
    n_lit = max(257, int(np.flatnonzero(lengths)[-1]) + 1)
    cl_len = np.asarray(CL_LENGTHS, dtype=np.int64)
    cl_codes = _reverse_bits(canonical_codes(cl_len), cl_len)

    code, nbits = [4, n_lit - 257, 0, len(CL_ORDER) - 4], [3, 5, 5, 4]   # BFINAL 0, BTYPE 10; HLIT, HDIST, HCLEN
    for s in CL_ORDER:
        code.append(CL_LENGTHS[s])
        nbits.append(3)
    for s, x, xb in code_length_sequence(list(lengths[:n_lit]) + [1]):    # ... and the one distance code, of 1 bit
        code.append(int(cl_codes[s]) | (x << CL_LENGTHS[s]))
        nbits.append(CL_LENGTHS[s] + xb)
    at = sym >= 0
    is_match = (sym[at] > END_OF_BLOCK).astype(np.int64)
    tok_len = lengths[sym[at]]
    code = np.concatenate([np.asarray(code, dtype=np.int64), codes[sym[at]] | (extra[at] << tok_len),
                           [codes[END_OF_BLOCK]]])
    nbits = np.concatenate([np.asarray(nbits, dtype=np.int64), tok_len + eb[at] + is_match,   # + the distance: one 0 bit
                            [lengths[END_OF_BLOCK]]])
    total = int(nbits.sum()) + 3            # + the header of the empty stored block
    return _pack_bits(code, nbits, 0, total) + SYNC_TAIL


def _pack_bits(code: np.ndarray, nbits: np.ndarray, first_bit: int, total_bits: int) -> bytes:
    bits = np.zeros(-(-total_bits // 8) * 8, dtype=np.uint8)
    at = first_bit + np.cumsum(nbits) - nbits
    for k in range(int(nbits.max()) if nbits.size else 0):
        take = nbits > k
        bits[at[take] + k] = (code[take] >> k) & 1
    return np.packbits(bits, bitorder='little').tobytes()


def segment_data(seg: np.ndarray) -> Tuple[bytes, bool]:
    """(deflate bytes of one segment, whether they are the stored form)."""
    seg = np.asarray(seg, dtype=np.uint8)
    n = seg.size
    code, nbits = segment_tokens(seg)
    total = 3 + int(nbits.sum()) + 7 + 3   # block header, tokens, end of block, header of the empty stored block
    fixed_len = -(-total // 8) + 4
    if fixed_len > 5 + n:
        return b'\x00' + struct.pack('<HH', n, n ^ 0xffff) + seg.tobytes(), True
    body = bytearray(_pack_bits(code, nbits, 3, total))
    body[0] |= 2                           # BFINAL = 0, BTYPE = 01
    return bytes(body) + SYNC_TAIL, False


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def encode_segments(img: np.ndarray) -> List[Tuple[bytes, bool]]:
    stream = filtered_stream(img)
    return [segment_data(stream[at:at + SEG_BYTES]) for at in range(0, stream.size, SEG_BYTES)]


def segment_data_mode(seg: np.ndarray, huffman: str = 'fixed') -> Tuple[bytes, str]:
    """(deflate bytes of one segment, its form 'fixed' / 'stored' / 'fitted'): under ``huffman='fitted'`` the fitted form
    where it is strictly shorter than ``segment_data``'s choice."""
    if huffman not in HUFFMAN_MODES:
        raise ValueError('png_layout: huffman must be one of {}, got {!r}'.format(HUFFMAN_MODES, huffman))
    data, stored = segment_data(seg)
    if huffman == 'fitted':
        fitted = segment_data_fitted(seg)
        if len(fitted) < len(data):
            return fitted, 'fitted'
    return data, 'stored' if stored else 'fixed'


def encode_segment_forms(img: np.ndarray, huffman: str = 'fixed') -> List[Tuple[bytes, str]]:
    stream = filtered_stream(img)
    return [segment_data_mode(stream[at:at + SEG_BYTES], huffman) for at in range(0, stream.size, SEG_BYTES)]


def encode(img: np.ndarray, huffman: str = 'fixed') -> bytes:
    """The PNG file of a uint8 [H,W] array in the layout above."""
    img = np.asarray(img)
    stream = filtered_stream(img)
    h, w = img.shape
    parts = [SIGNATURE, _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0))]
    for s, (data, _form) in enumerate(encode_segment_forms(img, huffman)):
        parts.append(_chunk(b'IDAT', (ZLIB_HEADER if s == 0 else b'') + data))
    parts.append(_chunk(b'IDAT', b'\x03\x00' + struct.pack('>I', zlib.adler32(stream.tobytes()) & 0xffffffff)))
    parts.append(_chunk(b'IEND', b''))
    return b''.join(parts)


PLTE_BYTES = 12 + 768                     # the palette chunk of an indexed file: always 256 entries


def max_file_bytes_indexed(h: int, w: int) -> int:
    return max_file_bytes(h, w) + PLTE_BYTES


def encode_indexed(labels: np.ndarray, palette=None, huffman: str = 'fixed') -> bytes:
    """The palette PNG file of a uint8 [H,W] label map (fosvos_png_encode_indexed): the file of ``encode(labels, huffman)`` -
    same filtered stream, segments, segment forms, IDAT chunks, final IDAT and IEND - under an IHDR of colour type 3 (bit
    depth 8) and with ONE ``PLTE`` chunk of 768 bytes between IHDR and the first IDAT.  ``palette``: uint8 [256,3] RGB;
    None = ``object_merge.davis_palette()``."""
    if palette is None:
        from util import object_merge
        palette = object_merge.davis_palette()
    palette = np.asarray(palette)
    if palette.dtype != np.uint8 or palette.shape != (256, 3):
        raise ValueError('png_layout.encode_indexed: a uint8 [256,3] palette, got {} {}'.format(palette.dtype, palette.shape))
    grey = encode(labels, huffman)
    h, w = np.asarray(labels).shape
    first_idat = len(SIGNATURE) + 25
    return (SIGNATURE + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 3, 0, 0, 0)) + _chunk(b'PLTE', palette.tobytes())
            + grey[first_idat:])


def chunks(file: bytes) -> List[Tuple[bytes, bytes]]:
    """[(tag, data)] of a PNG file, CRCs checked."""
    if file[:8] != SIGNATURE:
        raise ValueError('png_layout.chunks: not a PNG signature')
    out, at = [], 8
    while at < len(file):
        n, = struct.unpack('>I', file[at:at + 4])
        tag, data = file[at + 4:at + 8], file[at + 8:at + 8 + n]
        crc, = struct.unpack('>I', file[at + 8 + n:at + 12 + n])
        if crc != zlib.crc32(tag + data) & 0xffffffff:
            raise ValueError('png_layout.chunks: bad CRC in {!r} at {}'.format(tag, at))
        out.append((tag, data))
        at += 12 + n
    return out
