"""Measuring how the picture moved between two frames, and moving a mask along with it, stated in numpy: full-search block
matching on the frames' luma and a per-block warp of a mask.  It makes the temporal gate of util/mask_components.py
(``CleanOptions.temporal_radius``) follow a moving camera: the seed of frame t is what frame t - 1 kept, WARPED along the
estimated motion, instead of that mask at the same pixel coordinates.  The reference has no such step; these definitions ARE
the bytes of csrc/motion.hip (``ops.motion_luma``, ``ops.motion_estimate``, ``ops.motion_warp``), compared with exact equality.
Everything is integer arithmetic.

Options (``fosvos_hip.options.MotionOptions``, or anything with these attributes; ``Params`` here holds the defaults):
``block`` in {8, 16}, ``search`` in 1..16, ``zero_bias`` in 0..255.

``luma``: the net's input float32 [3,H,W] (BGR minus MEANVAL) -> uint8 [H,W].  ``g = mask_crf.guide_levels(image)`` takes the
frame's bytes back (a NaN gives 0; an averaged ``net_size`` image rounds); ``Y = (29 g[0] + 150 g[1] + 77 g[2] + 128) >> 8``.

``estimate(prev, cur)``: block ``(by, bx)`` owns the pixels P of its ``block x block`` square that lie in the frame (ragged edge
blocks are smaller).  A candidate ``d = (dy, dx)`` in ``[-search, search]^2`` is valid iff ``P + d`` lies wholly inside the
frame - an invalid one is skipped, never clamped; ``(0, 0)`` is always valid.  ``SAD(d) = sum over P of |cur[p] - prev[p + d]|``;
``score(d) = SAD(d) + (d != 0 ? (zero_bias |P|) >> 4 : 0)``.  The winner is the smallest ``(score, dy^2 + dx^2, dy, dx)`` in
lexicographic order - as ONE integer, ``KEY`` below.  ``field`` holds the winner's ``(dy, dx)``, ``cost`` its unbiased SAD.
Sign convention: ``cur[p] ~ prev[p + field]`` - the vector points from a pixel of the current frame to where it was.

``warp(mask, field)``: ``out[y, x] = mask[y + dy, x + dx] != 0`` with ``(dy, dx) = field[y // block, x // block]``; a source pixel
outside the frame gives 0, whatever int8 values the field holds.  It carries the previous frame's mask into the current
frame's coordinates.

numpy only: importable anywhere.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from util import mask_components, mask_crf

BLOCKS = (8, 16)
MAX_SEARCH = 16
MAX_ZERO_BIAS = 255
LUMA_WEIGHTS = (29, 150, 77)   # of the image's planes in their order, B G R; they sum to 256
# the key of a candidate: score << 22 | (dy^2 + dx^2) << 12 | (dy + 16) << 6 | (dx + 16), every field wide enough for its
# values: dx + 16 and dy + 16 in 0..32 (6 bits), dy^2 + dx^2 <= 512 (10 bits); SAD <= 255 * 256 = 65280 and the bias
# <= (255 * 256) >> 4 = 4080, so score < 2^17 and the key < 2^39
KEY_DX_BITS, KEY_DY_BITS, KEY_D2_BITS = 6, 6, 10
KEY_D2_SHIFT = KEY_DX_BITS + KEY_DY_BITS
KEY_SCORE_SHIFT = KEY_D2_SHIFT + KEY_D2_BITS


class Params(NamedTuple):
    """The defaults (the design's, unmeasured on real sequences); ``fosvos_hip.options.MotionOptions`` has the same fields."""
    block: int = 16
    search: int = 8
    zero_bias: int = 8


def check_options(options=None, **given) -> Params:
    """The options as ``Params`` of ints, or ValueError with the range.  ``given``: fields that replace the options'."""
    o = Params() if options is None else options
    got = {}
    for name, lo, hi in (("block", min(BLOCKS), max(BLOCKS)), ("search", 1, MAX_SEARCH), ("zero_bias", 0, MAX_ZERO_BIAS)):
        v = given[name] if given.get(name) is not None else getattr(o, name)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
        got[name] = int(v)
    if got["block"] not in BLOCKS:
        raise ValueError("block must be one of %s, got %r" % (BLOCKS, got["block"]))
    return Params(**got)


def grid(h: int, w: int, block: int):
    """(Hb, Wb): the blocks of an ``h x w`` frame."""
    return -(-int(h) // int(block)), -(-int(w) // int(block))


def key(score, d2, dy, dx):
    """The candidate's place in the order as one integer (int64 arrays or ints)."""
    return (score << KEY_SCORE_SHIFT) | (d2 << KEY_D2_SHIFT) | ((dy + MAX_SEARCH) << KEY_DX_BITS) | (dx + MAX_SEARCH)


def luma(image: np.ndarray) -> np.ndarray:
    """float32 [3,H,W] -> uint8 [H,W], or [N,3,H,W] -> [N,H,W]."""
    image = np.asarray(image)
    if image.ndim == 4:
        if image.shape[0] == 0:
            raise ValueError("image must be a non-empty float32 [N,3,H,W], got %s" % (image.shape,))
        return np.ascontiguousarray(np.stack([luma(image[k]) for k in range(image.shape[0])]))
    g = mask_crf.guide_levels(image).astype(np.int32)
    y = (LUMA_WEIGHTS[0] * g[0] + LUMA_WEIGHTS[1] * g[1] + LUMA_WEIGHTS[2] * g[2] + 128) >> 8
    return np.ascontiguousarray(y.astype(np.uint8))


def _planes(prev, cur):
    prev, cur = np.asarray(prev), np.asarray(cur)
    if prev.dtype != np.uint8 or cur.dtype != np.uint8:
        raise ValueError("estimate: uint8 luma planes, got %s and %s" % (prev.dtype, cur.dtype))
    if prev.shape != cur.shape or cur.ndim not in (2, 3) or cur.size == 0:
        raise ValueError("estimate: two non-empty planes [H,W] or [N,H,W] of one shape, got %s and %s" % (prev.shape, cur.shape))
    return prev, cur


def estimate_loop(prev_y, cur_y, block: Optional[int] = None, search: Optional[int] = None, zero_bias: Optional[int] = None,
                  options=None):
    """``estimate`` as a plain loop over the blocks and the candidates, the module's text line by line."""
    o = check_options(options, block=block, search=search, zero_bias=zero_bias)
    prev, cur = _planes(prev_y, cur_y)
    if cur.ndim == 3:
        both = [estimate_loop(prev[k], cur[k], options=o) for k in range(cur.shape[0])]
        return np.stack([f for f, _ in both]), np.stack([c for _, c in both])
    h, w = cur.shape
    hb, wb = grid(h, w, o.block)
    p, c = prev.astype(np.int64), cur.astype(np.int64)
    field = np.zeros((hb, wb, 2), dtype=np.int8)
    cost = np.zeros((hb, wb), dtype=np.int32)
    for by in range(hb):
        for bx in range(wb):
            y0, x0 = by * o.block, bx * o.block
            y1, x1 = min(h, y0 + o.block), min(w, x0 + o.block)
            area = (y1 - y0) * (x1 - x0)
            best = None
            for dy in range(-o.search, o.search + 1):
                for dx in range(-o.search, o.search + 1):
                    if y0 + dy < 0 or y1 + dy > h or x0 + dx < 0 or x1 + dx > w:
                        continue
                    sad = int(np.abs(c[y0:y1, x0:x1] - p[y0 + dy:y1 + dy, x0 + dx:x1 + dx]).sum())
                    score = sad + ((o.zero_bias * area) >> 4 if (dy, dx) != (0, 0) else 0)
                    cand = (score, dy * dy + dx * dx, dy, dx, sad)
                    if best is None or cand < best:
                        best = cand
            field[by, bx] = best[2], best[3]
            cost[by, bx] = best[4]
    return field, cost


def estimate(prev_y, cur_y, block: Optional[int] = None, search: Optional[int] = None, zero_bias: Optional[int] = None,
             options=None):
    """uint8 planes [H,W] or [N,H,W] -> (field int8 [.., Hb, Wb, 2], cost int32 [.., Hb, Wb]).  Vectorised over the pixels and
    the blocks, sequential over the candidates; ``estimate_loop`` is its check."""
    o = check_options(options, block=block, search=search, zero_bias=zero_bias)
    prev, cur = _planes(prev_y, cur_y)
    h, w = cur.shape[-2:]
    hb, wb = grid(h, w, o.block)
    lead = cur.shape[:-2]
    p, c = prev.astype(np.int32), cur.astype(np.int32)
    ys, xs = np.arange(hb) * o.block, np.arange(wb) * o.block
    ye, xe = np.minimum(ys + o.block, h), np.minimum(xs + o.block, w)
    bias = (o.zero_bias * ((ye - ys)[:, None] * (xe - xs)[None, :]).astype(np.int64)) >> 4
    never = np.int64(1) << 62
    best = np.full(lead + (hb, wb), never, dtype=np.int64)
    best_sad = np.zeros(lead + (hb, wb), dtype=np.int64)
    diff = np.zeros(lead + (h, w), dtype=np.int32)
    for dy in range(-o.search, o.search + 1):
        ylo, yhi = max(0, -dy), min(h, h - dy)   # the rows y whose source row y + dy exists
        ok_y = (ys + dy >= 0) & (ye + dy <= h)
        for dx in range(-o.search, o.search + 1):
            xlo, xhi = max(0, -dx), min(w, w - dx)
            ok = ok_y[:, None] & ((xs + dx >= 0) & (xe + dx <= w))[None, :]
            if not ok.any():
                continue
            diff[...] = 0
            np.abs(c[..., ylo:yhi, xlo:xhi] - p[..., ylo + dy:yhi + dy, xlo + dx:xhi + dx], out=diff[..., ylo:yhi, xlo:xhi])
            sad = np.add.reduceat(np.add.reduceat(diff, ys, axis=-2), xs, axis=-1).astype(np.int64)
            score = sad + (bias if (dy, dx) != (0, 0) else 0)
            k = np.where(ok, key(score, np.int64(dy * dy + dx * dx), np.int64(dy), np.int64(dx)), never)
            better = k < best
            best = np.where(better, k, best)
            best_sad = np.where(better, sad, best_sad)
    field = np.empty(lead + (hb, wb, 2), dtype=np.int8)
    field[..., 0] = ((best >> KEY_DX_BITS) & ((1 << KEY_DY_BITS) - 1)) - MAX_SEARCH
    field[..., 1] = (best & ((1 << KEY_DX_BITS) - 1)) - MAX_SEARCH
    return field, np.ascontiguousarray(best_sad.astype(np.int32))


def warp(mask: np.ndarray, field: np.ndarray, block: int) -> np.ndarray:
    """uint8 or bool [H,W] and int8 [Hb,Wb,2] -> uint8 [H,W] of 0 and 1.  The source index is formed in wide integers and
    tested against the frame before anything is read, so no field can reach outside the mask."""
    mask, field = np.asarray(mask), np.asarray(field)
    if mask.ndim != 2 or mask.dtype not in (np.uint8, np.bool_) or mask.size == 0:
        raise ValueError("warp: a non-empty uint8 or bool [H,W] mask, got %s %s" % (mask.dtype, mask.shape))
    if block not in BLOCKS:
        raise ValueError("block must be one of %s, got %r" % (BLOCKS, block))
    h, w = mask.shape
    if field.dtype != np.int8 or field.shape != grid(h, w, block) + (2,):
        raise ValueError("warp: the field of a %s mask at block %d is int8 %s, got %s %s"
                         % (mask.shape, block, grid(h, w, block) + (2,), field.dtype, field.shape))
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    d = field[y // block, x // block].astype(np.int64)
    sy, sx = y + d[..., 0], x + d[..., 1]
    inside = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    src = mask[np.where(inside, sy, 0), np.where(inside, sx, 0)] != 0
    return np.ascontiguousarray((inside & src).astype(np.uint8))


def _clean_rules(clean):
    radius = getattr(clean, "temporal_radius", None)
    if radius is None:
        raise ValueError("the motion-compensated gate is the temporal gate's: set clean.temporal_radius")
    return dict(radius=radius, min_area=clean.min_area, largest=clean.largest, fill=clean.fill)


def gate_sequence(images, logits, seed, clean, motion=None, prev_luma: Optional[np.ndarray] = None,
                  prev_kept: Optional[np.ndarray] = None):
    """The chain of ``mask_components.clean_sequence`` with its seed carried along the estimated motion.  images float32
    [N,3,H,W] (the net's input), logits float32 [N,H,W], ``clean``: a CleanOptions with ``temporal_radius``, ``motion``: a
    MotionOptions (None: the defaults) -> (cleaned float32 [N,H,W], kept bool [N,H,W]).  Frame 0 is gated by ``seed`` ([H,W]
    or None) as given; frame t > 0 by ``warp(kept[t-1], estimate(luma(images[t-1]), luma(images[t])))``.  To continue across
    groups pass the luma plane and the kept mask of the frame before as ``prev_luma`` / ``prev_kept`` (both or neither):
    frame 0 is then gated like every other frame and ``seed`` must be None."""
    o = check_options(motion)
    rules = _clean_rules(clean)
    images, logits = np.asarray(images), np.asarray(logits)
    if logits.ndim != 3 or logits.dtype != np.float32 or logits.shape[0] == 0:
        raise ValueError("gate_sequence: float32 [N,H,W] logits, got %s %s" % (logits.dtype, logits.shape))
    n, h, w = logits.shape
    if images.shape != (n, 3, h, w):
        raise ValueError("gate_sequence: images must be %s, got %s" % ((n, 3, h, w), images.shape))
    if (prev_luma is None) != (prev_kept is None):
        raise ValueError("gate_sequence: prev_luma and prev_kept come together")
    if prev_luma is not None and seed is not None:
        raise ValueError("gate_sequence: a seed belongs to a sequence's first frame; prev_luma / prev_kept continue one")
    planes = luma(images)
    out = np.empty_like(logits)
    kept = np.zeros(logits.shape, dtype=bool)
    before_y, before_kept = prev_luma, prev_kept
    for t in range(n):
        if before_y is not None:
            field, _ = estimate(before_y, planes[t], options=o)
            seed = warp(np.asarray(before_kept).astype(np.uint8), field, o.block)
        one, k = mask_components.clean_sequence(logits[t:t + 1], seed, chain=True, **rules)
        out[t], kept[t] = one[0], k[0]
        before_y, before_kept = planes[t], kept[t]
    return out, kept


def track(frames, seed, clean, motion=None, reseed=None):
    """The stream's chain, the byte-for-byte reference of ``FrameSegmenter(clean=, motion=)``: ``frames`` is a sequence of
    ``(image float32 [3,H,W], logits float32 [H,W])`` - what the net saw and what it answered, in submission order -,
    ``seed`` the mask handed to the constructor or None, ``reseed`` a dict {index: mask} of ``seed(mask)`` calls made before
    frame ``index`` was submitted.  A hand-set seed gates the next frame unwarped and the motion starts again from that
    frame.  Returns (cleaned float32 [N,H,W], kept bool [N,H,W])."""
    reseed = reseed or {}
    outs, kepts = [], []
    before_y = before_kept = None
    for t, (image, logits) in enumerate(frames):
        image, logits = np.asarray(image), np.asarray(logits)
        if t in reseed:
            seed, before_y, before_kept = reseed[t], None, None
        out, kept = gate_sequence(image[None], logits[None], seed if before_y is None else None, clean, motion,
                                  before_y, before_kept)
        outs.append(out[0])
        kepts.append(kept[0])
        before_y, before_kept = luma(image), kept[0]
    return np.stack(outs), np.stack(kepts)
