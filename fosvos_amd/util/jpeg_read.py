"""The JPEG files the device decoder (csrc/jpeg_decode.hip, fosvos_jpeg_decode) takes and the pixels it makes of them, stated
in numpy integers: the kernels are tested byte for byte against ``decode``, and ``decode`` byte for byte against PIL
(libjpeg-turbo) on the inputs of tests/jpeg_read_cases.py.  No float touches the data path.

``probe`` parses the markers and answers with a ``Plan``, or with ``None`` for every file the device path does not take
(``None`` is the host path's signal, never an error).  It takes baseline sequential files (SOF0, 8 bits) with one scan that
interleaves all components, grey or three components sampled 1x1,1x1,1x1 ('4:4:4') or 2x2,1x1,1x1 ('4:2:0'), 8-bit
quantisation tables, and refuses

* any other SOF, 12-bit samples, 16-bit quantisation tables, a table a component selects but the file does not define;
* more than one scan, a scan that leaves a component out or reorders them, spectral selection other than 0..63, a
  successive-approximation byte other than 0;
* any other sampling factors (4:2:2, 4:4:0, 4:1:1, ...), and 4:2:0 with ``width < 5``: libjpeg-turbo smooths the chroma of
  a 4:2:0 file only where a chroma row has more than two samples and replicates below;
* an APP14 "Adobe" segment (the colour transform is then the segment's), and three components without a JFIF APP0 whose
  ids are not 1, 2, 3 (libjpeg then guesses the colour space from the ids);
* a DHT that is no well-formed prefix code: more than 256 symbols, a payload shorter than its counts, more codes of a
  length than are left (Kraft sum above 1), or a DC symbol above 15.  A code may leave prefixes unassigned, as the standard
  tables do; a stream that reaches one decodes to status 2;
* restart markers that do not run RST0..RST7 cyclically with one marker between any two intervals of DRI MCUs and none
  elsewhere, any other marker or a 0xFF 0xFF pair inside the entropy data;
* structural damage: no SOI, a segment length past the end, no SOF or SOS, no EOI behind the scan, zero height or width.

Inside entropy data a 0xFF byte is followed by 0x00 or by a marker, so the restart markers are found by a byte search and
the ``segments`` table has one row per restart interval (one row for the scan where there is no DRI): (byte offset of the
entropy data, byte length, first MCU, MCU count).  A segment needs nothing from another: it starts on a byte with the DC
predictors at 0.

``coefficients`` is the entropy decode.  Blocks are stored component by component, each in raster order of the component's
padded block grid (``block_layout``): an MCU of the ``mh x mw`` MCU grid holds, at 4:2:0, luma blocks (2 my + j // 2,
2 mx + j % 2) for j = 0..3 of a ``2 mh x 2 mw`` grid, then block (my, mx) of Cb and of Cr; otherwise block (my, mx) of every
component.  Per segment: stuffing removed (0xFF 0x00 -> 0xFF), bits MSB first; a symbol is the code of its component's DC or
AC table, followed by the value bits; EXTEND as in the standard; a DC difference adds to the component's predictor (32-bit
wrap, stored as int16); AC symbols run through zigzag positions 1..63: 0x00 ends the block, 0xF0 skips 16 positions, any
other ``run << 4 | size`` skips ``run`` and stores one coefficient.  After a skip the position must still be <= 63, else the
segment ends with status 3 (so a 0xF0 that leaves no room for a coefficient is an error too; libjpeg lets it pass, no
encoder writes it).  Status codes of a segment:

    0  ok
    1  the segment's bytes ran out before its MCUs did (bits beyond the last byte read as 0; the status is raised by the
       first symbol - code and value bits - that consumes one, before anything else about that symbol is looked at)
    2  no code matches within 16 bits
    3  a coefficient index beyond 63
    5  (set by ``reconstruct``) some ``coefficient x quant`` lies outside +-32767: libjpeg-turbo's SIMD and C inverse DCTs
       differ on such files, so the device path does not claim them

A segment stops at its first error: the block the error falls in and every later block of the segment stay zero.  A file's
status is the smallest non-zero status of its segments.

``reconstruct``: ``x = coef * quant`` (an ``x`` outside +-32767 raises status 5 and counts as 0), the inverse DCT below
(libjpeg's slow-integer one: the 13-bit constants of jpeg_layout.DCT_CONST, a column pass descaled by 11 bits, a row pass by
18, 32-bit wrap-around arithmetic), the sample a function of ``v & 1023``; 4:2:0 chroma through libjpeg's "fancy" h2v2
upsampling of the real ceil(H/2) x ceil(W/2) samples (never the block padding); libjpeg's 16-bit fixed-point YCbCr -> RGB
rows; the output uint8 [H,W,3] BGR (``read_bgr``'s order) or [H,W] grey.
"""
import functools
import struct
from collections import namedtuple
from typing import List, Optional, Tuple

import numpy as np

from util.jpeg_layout import DCT_CONST, ZIGZAG

SUBSAMPLINGS = ('4:4:4', '4:2:0')
OK, E_BYTES, E_CODE, E_INDEX, E_RANGE = 0, 1, 2, 3, 5

# quant: per component an int32 [64] in natural order; dht: {(class, id): 16 counts + symbols} of the tables the scan selects;
# dc_tables / ac_tables: per component the table id; scan: (first byte of the entropy data, offset of the EOI marker);
# segments: int32 [n, 4] rows (byte offset, byte length, first MCU, MCU count)
Plan = namedtuple('Plan', 'height width components subsampling restart_interval quant dht dc_tables ac_tables scan segments')


# ------------------------------------------------------------------------------------------ probe
def _dht_ok(cls: int, payload: bytes) -> bool:
    counts, syms = payload[:16], payload[16:]
    if sum(counts) > 256 or sum(counts) != len(syms):
        return False
    code = 0
    for bits in range(1, 17):
        code += counts[bits - 1]
        if code > (1 << bits):
            return False
        code <<= 1
    return not (cls == 0 and any(s > 15 for s in syms))


def n_mcus(height: int, width: int, components: int, subsampling: str) -> Tuple[int, int]:
    """(rows, columns) of the MCU grid."""
    side = 16 if (components == 3 and subsampling == '4:2:0') else 8
    return -(-height // side), -(-width // side)


def probe(data: bytes) -> Optional[Plan]:
    """The plan of a file the device path takes, ``None`` for every other (see the module text)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b'\xff\xd8':
        return None
    at = 2
    qt, dht = {}, {}
    frame = None
    ri = 0
    jfif = False
    while True:
        if at + 4 > n or data[at] != 0xFF:
            return None
        marker = data[at + 1]
        if marker == 0xFF:                      # fill byte in front of a marker
            at += 1
            continue
        if marker in (0x01, 0xD8, 0xD9) or 0xD0 <= marker <= 0xD7:
            return None
        size = struct.unpack('>H', data[at + 2:at + 4])[0]
        if size < 2 or at + 2 + size > n:
            return None
        body = data[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0 or tq > 3 or k + 65 > len(body):
                    return None
                t = np.zeros(64, dtype=np.int32)
                t[list(ZIGZAG)] = np.frombuffer(body[k + 1:k + 65], dtype=np.uint8)
                qt[tq] = t
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    return None
                cls, tid = body[k] >> 4, body[k] & 15
                total = sum(body[k + 1:k + 17])
                if cls > 1 or tid > 3 or k + 17 + total > len(body):
                    return None
                dht[(cls, tid)] = body[k + 1:k + 17 + total]
                k += 17 + total
        elif marker == 0xC0:
            if frame is not None or len(body) < 6:
                return None
            precision, h, w, nc = struct.unpack('>BHHB', body[:6])
            if precision != 8 or h == 0 or w == 0 or nc not in (1, 3) or len(body) != 6 + 3 * nc:
                return None
            frame = (h, w, [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(nc)])
        elif 0xC1 <= marker <= 0xCF:            # any other SOF, DAC (DHT 0xC4 is handled above)
            return None
        elif marker == 0xDD:
            if len(body) != 2:
                return None
            ri = struct.unpack('>H', body)[0]
        elif marker == 0xE0:
            jfif = jfif or body[:5] == b'JFIF\x00'
        elif marker == 0xEE:
            if body[:5] == b'Adobe':
                return None
        elif marker == 0xDA:
            break
    if frame is None:
        return None
    h, w, comps = frame
    nc = len(comps)
    if len(body) != 4 + 2 * nc or body[0] != nc or body[1 + 2 * nc:] != b'\x00\x3f\x00':
        return None
    factors = tuple(c[1] for c in comps)
    if nc == 1:
        if factors[0] != 0x11:                  # one component: libjpeg ignores the factors, the device path keeps to 1x1
            return None
        sub = '4:4:4'
    elif factors == (0x11, 0x11, 0x11):
        sub = '4:4:4'
    elif factors == (0x22, 0x11, 0x11):
        sub = '4:2:0'
    else:
        return None
    if nc == 3 and not jfif and tuple(c[0] for c in comps) != (1, 2, 3):
        return None
    if sub == '4:2:0' and w < 5:
        return None
    dc_t, ac_t, used = [], [], {}
    for i in range(nc):
        cid, tables = body[1 + 2 * i], body[2 + 2 * i]
        td, ta = tables >> 4, tables & 15
        if cid != comps[i][0] or td > 3 or ta > 3 or (0, td) not in dht or (1, ta) not in dht or comps[i][2] not in qt:
            return None
        dc_t.append(td)
        ac_t.append(ta)
        used[(0, td)] = dht[(0, td)]
        used[(1, ta)] = dht[(1, ta)]
    if len(set(c[0] for c in comps)) != nc or not all(_dht_ok(k[0], v) for k, v in used.items()):
        return None
    # the entropy data: every 0xFF in it is followed by 0x00 or starts a marker
    start = at
    b = np.frombuffer(data, dtype=np.uint8, offset=start)
    ff = np.flatnonzero((b[:-1] == 0xFF) & (b[1:] != 0x00)) if b.size > 1 else np.zeros(0, dtype=np.int64)
    mh, mw = n_mcus(h, w, nc, sub)
    total = mh * mw
    n_seg = -(-total // ri) if ri else 1
    if ff.size < n_seg:
        return None
    marks = ff[:n_seg]
    if np.any(np.diff(marks) < 2):              # 0xFF 0xFF
        return None
    codes = b[marks + 1]
    if codes[-1] != 0xD9 or np.any(codes[:-1] != 0xD0 + (np.arange(n_seg - 1) & 7)):
        return None
    begin = np.concatenate([[0], marks[:-1] + 2])
    seg = np.stack([begin + start, marks - begin, np.arange(n_seg) * (ri if ri else total),
                    np.minimum(ri if ri else total, total - np.arange(n_seg) * (ri if ri else total))], axis=1)
    return Plan(h, w, nc, sub, ri, tuple(qt[c[2]].copy() for c in comps), used, tuple(dc_t), tuple(ac_t),
                (start, start + int(marks[-1])), seg.astype(np.int32))


# ------------------------------------------------------------------------------------------ entropy decode
def block_layout(plan) -> Tuple[int, List[Tuple[int, int, int]]]:
    """(blocks of a file, per component (first block, block rows, block columns) of its padded grid)."""
    mh, mw = n_mcus(plan.height, plan.width, plan.components, plan.subsampling)
    out, first = [], 0
    for c in range(plan.components):
        f = 2 if (plan.subsampling == '4:2:0' and c == 0) else 1
        out.append((first, f * mh, f * mw))
        first += f * mh * f * mw
    return first, out


def mcu_blocks(plan, m: int) -> List[Tuple[int, int]]:
    """[(component, block index)] of MCU ``m`` in coding order."""
    mh, mw = n_mcus(plan.height, plan.width, plan.components, plan.subsampling)
    _, grids = block_layout(plan)
    my, mx = divmod(m, mw)
    out = []
    for c, (first, _, cols) in enumerate(grids):
        if cols == 2 * mw and plan.subsampling == '4:2:0' and c == 0:
            out += [(0, first + (2 * my + (j >> 1)) * cols + 2 * mx + (j & 1)) for j in range(4)]
        else:
            out.append((c, first + my * cols + mx))
    return out


@functools.lru_cache(maxsize=64)
def _lut(payload: bytes) -> list:
    """16-bit prefix -> length << 8 | symbol, 0 where no code matches (the canonical assignment of Annex C)."""
    lut = np.zeros(1 << 16, dtype=np.int32)
    code, k = 0, 16
    for bits in range(1, 17):
        for _ in range(payload[bits - 1]):
            lo = code << (16 - bits)
            lut[lo:lo + (1 << (16 - bits))] = bits << 8 | payload[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def _wrap(v: int, bits: int) -> int:
    half = 1 << (bits - 1)
    return ((v + half) & ((1 << bits) - 1)) - half


def _segment(plan, data: bytes, row, coef: np.ndarray) -> int:
    off, length, first, count = (int(v) for v in row)
    seg = data[off:off + length].replace(b'\xff\x00', b'\xff')
    total_bits = 8 * len(seg)
    seg += bytes(16)
    nseg = len(seg)
    dc = [_lut(plan.dht[(0, t)]) for t in plan.dc_tables]
    ac = [_lut(plan.dht[(1, t)]) for t in plan.ac_tables]
    acc, nb, at = 0, 0, 0
    pred = [0] * plan.components
    zz = ZIGZAG
    for m in range(first, first + count):
        for c, index in mcu_blocks(plan, m):
            blk = [0] * 64
            k = 0
            lut = dc[c]
            while k < 64:
                while nb < 32:
                    acc = ((acc << 8) | (seg[at] if at < nseg else 0)) & 0xFFFFFFFFFFFFFFFF
                    at += 1
                    nb += 8
                e = lut[(acc >> (nb - 16)) & 0xFFFF]
                if e == 0:
                    return E_CODE
                nb -= e >> 8
                rs = e & 255
                s = rs & 15
                v = 0
                if s:
                    nb -= s
                    v = (acc >> nb) & ((1 << s) - 1)
                    if v < (1 << (s - 1)):
                        v -= (1 << s) - 1
                if 8 * at - nb > total_bits:
                    return E_BYTES
                if k == 0:
                    pred[c] = _wrap(pred[c] + v, 32)
                    v = pred[c]
                    lut = ac[c]
                elif s == 0:
                    if rs != 0xF0:
                        break
                    k += 16
                    if k > 63:
                        return E_INDEX
                    continue
                else:
                    k += rs >> 4
                    if k > 63:
                        return E_INDEX
                blk[zz[k]] = _wrap(v, 16)
                k += 1
            coef[index] = blk
    return OK


def coefficients(plan, data: bytes) -> Tuple[np.ndarray, int]:
    """(int16 [blocks, 64] in natural order, status) of the file ``plan`` was probed from."""
    data = bytes(data)
    total, _ = block_layout(plan)
    coef = np.zeros((total, 64), dtype=np.int16)
    status = OK
    for row in plan.segments:
        st = _segment(plan, data, row, coef)
        if st and (status == OK or st < status):
            status = st
    return coef, status


# ------------------------------------------------------------------------------------------ what the kernels are sent
TABLES_BYTES = 2384
SAMPLING_CODE = {'4:4:4': 444, '4:2:0': 420}


def pack_tables(plan, seg_first: int, seg_count: int) -> bytes:
    """The per-file record of fosvos_jpeg_decode (include/fosvos_hip.h): quant uint8 [3][64], dc_slot [3], ac_slot [3], two
    unused bytes, int32 first row and row count in the call's segment table, eight slots (class * 4 + id) of 272 bytes with
    the DHT payloads as they stand in the file."""
    q = b''.join(bytes(t.astype(np.uint8)) for t in plan.quant).ljust(192, b'\0')
    dc = bytes(plan.dc_tables).ljust(3, b'\0')
    ac = bytes(4 + t for t in plan.ac_tables).ljust(3, b'\0')
    slots = b''.join(plan.dht.get((s >> 2, s & 3), b'').ljust(272, b'\0') for s in range(8))
    out = q + dc + ac + b'\0\0' + struct.pack('<ii', seg_first, seg_count) + slots
    assert len(out) == TABLES_BYTES
    return out


# ------------------------------------------------------------------------------------------ reconstruction
def idct_1d(d: np.ndarray, shift: int) -> np.ndarray:
    """One pass of the inverse DCT along the last axis (8 long), int32 in and out, wrap-around arithmetic."""
    k = DCT_CONST
    d = [d[..., i].astype(np.int32) for i in range(8)]
    z1 = (d[2] + d[6]) * np.int32(k['0.541196100'])
    t2 = z1 - d[6] * np.int32(k['1.847759065'])
    t3 = z1 + d[2] * np.int32(k['0.765366865'])
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    e0, e3, e1, e2 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * np.int32(k['1.175875602'])
    a0, a1 = a0 * np.int32(k['0.298631336']), a1 * np.int32(k['2.053119869'])
    a2, a3 = a2 * np.int32(k['3.072711026']), a3 * np.int32(k['1.501321110'])
    z1, z2 = z1 * np.int32(-k['0.899976223']), z2 * np.int32(-k['2.562915447'])
    z3, z4 = z3 * np.int32(-k['1.961570560']) + z5, z4 * np.int32(-k['0.390180644']) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [e0 + a3, e1 + a2, e2 + a1, e3 + a0, e3 - a0, e2 - a1, e1 - a2, e0 - a3]
    return np.stack([(v + np.int32(1 << (shift - 1))) >> shift for v in out], -1).astype(np.int32)


def samples(coef: np.ndarray, quant: np.ndarray) -> Tuple[np.ndarray, bool]:
    """(uint8 [blocks, 8, 8], whether some coefficient x quant left +-32767) of int16 [blocks, 64] coefficients."""
    x = coef.astype(np.int32) * quant.astype(np.int32)[None]
    bad = np.abs(x) > 32767
    x = np.where(bad, 0, x).astype(np.int32).reshape(-1, 8, 8)
    with np.errstate(over='ignore'):
        cols = idct_1d(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)      # down every column
        v = idct_1d(cols, 18) & 1023                                  # along every row
    out = np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))
    return out.astype(np.uint8), bool(bad.any())


def upsample_420(plane: np.ndarray, height: int, width: int) -> np.ndarray:
    """int32 [height, width] of the int [ceil(height/2), ceil(width/2)] chroma plane (libjpeg's h2v2 fancy upsampling)."""
    ch, cw = plane.shape
    p = plane.astype(np.int32)
    r = np.arange(2 * ch) >> 1
    far = np.clip(np.where(np.arange(2 * ch) & 1, r + 1, r - 1), 0, ch - 1)
    s = 3 * p[r] + p[far]                                              # [2 ch, cw]
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int32)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:height, :width]


def reconstruct(plan, coef: np.ndarray) -> Tuple[np.ndarray, int]:
    """(uint8 [H,W,3] BGR or [H,W], 5 where some coefficient x quant left +-32767 else 0) of ``coefficients``' blocks."""
    h, w = plan.height, plan.width
    _, grids = block_layout(plan)
    planes, bad = [], False
    for c, (first, rows, cols) in enumerate(grids):
        s, b = samples(coef[first:first + rows * cols], plan.quant[c])
        bad = bad or b
        planes.append(s.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8).astype(np.int32))
    status = E_RANGE if bad else OK
    if plan.components == 1:
        return np.ascontiguousarray(planes[0][:h, :w]).astype(np.uint8), status
    y = planes[0][:h, :w]
    if plan.subsampling == '4:2:0':
        ch, cw = -(-h // 2), -(-w // 2)
        cb, cr = (upsample_420(p[:ch, :cw], h, w) - 128 for p in planes[1:])
    else:
        cb, cr = (p[:h, :w] - 128 for p in planes[1:])
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8), status


def decode(data: bytes) -> Tuple[Optional[np.ndarray], int]:
    """(pixels, status) of a file ``probe`` takes; (None, -1) of any other.  The pixels of a non-zero status are not PIL's."""
    plan = probe(data)
    if plan is None:
        return None, -1
    coef, status = coefficients(plan, data)
    img, st5 = reconstruct(plan, coef)
    return img, status if status else st5
