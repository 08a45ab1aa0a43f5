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


def _reverse_bits(code: np.ndarray, nbits: np.ndarray) -> np.ndarray:
    out = np.zeros_like(code)
    for k in range(9):
        take = nbits > k
        out[take] |= ((code[take] >> (nbits[take] - 1 - k)) & 1) << k
    return out


def segment_tokens(seg: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(code, nbits) per byte position of one segment: the bits the position contributes to the fixed-Huffman block, LSB
    first, 0 bits where the byte is covered by a match that started earlier."""
    seg = np.asarray(seg, dtype=np.uint8)
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

    code = np.zeros(n, dtype=np.int64)
    nbits = np.zeros(n, dtype=np.int64)
    v = seg.astype(np.int64)
    lit_code = np.where(v < 144, 0x30 + v, 0x190 + v - 144)
    lit_bits = np.where(v < 144, 8, 9)
    code[is_literal] = _reverse_bits(lit_code[is_literal], lit_bits[is_literal])
    nbits[is_literal] = lit_bits[is_literal]

    lm = (length - 3)[is_match]
    eb = np.where(lm < 8, 0, np.floor(np.log2(np.maximum(lm, 1))).astype(np.int64) - 2)
    sym = np.where(lm < 8, 257 + lm, 261 + 4 * eb + ((lm >> eb) & 3))
    extra = lm & ((1 << eb) - 1)
    is258 = lm == MAX_MATCH - 3
    sym, eb, extra = np.where(is258, 285, sym), np.where(is258, 0, eb), np.where(is258, 0, extra)
    sym_code = np.where(sym < 280, sym - 256, 0xC0 + sym - 280)
    sym_bits = np.where(sym < 280, 7, 8)
    code[is_match] = _reverse_bits(sym_code, sym_bits) | (extra << sym_bits)
    nbits[is_match] = sym_bits + eb + 5    # + the 5-bit distance code 0 (distance 1), all zeros
    return code, nbits


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


def encode(img: np.ndarray) -> bytes:
    """The PNG file of a uint8 [H,W] array in the layout above."""
    img = np.asarray(img)
    stream = filtered_stream(img)
    h, w = img.shape
    parts = [SIGNATURE, _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0))]
    for s, (data, _stored) in enumerate(encode_segments(img)):
        parts.append(_chunk(b'IDAT', (ZLIB_HEADER if s == 0 else b'') + data))
    parts.append(_chunk(b'IDAT', b'\x03\x00' + struct.pack('>I', zlib.adler32(stream.tobytes()) & 0xffffffff)))
    parts.append(_chunk(b'IEND', b''))
    return b''.join(parts)


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
