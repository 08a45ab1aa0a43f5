"""One-shot augmentation that moves the object against its background (after Lucid Data Dreaming, Khoreva et al.), stated in
numpy.  The annotated frame is cut in two - the object, and the frame with the object painted out -, the two are warped
independently, the illumination is changed and they are composed again.  The reference has no such step: these definitions ARE
the bits of csrc/lucid.hip (``fosvos_hip.ops.lucid_sample``), compared with exact equality.

``fill_background(frame, mask, dilate, smooth)``: the frame with the object painted out, integers only, once per sample on the
host.  ``hole`` is ``mask != 0`` max-filtered over the (2 dilate + 1)^2 square (clipped at the border), ``valid`` the rest.
Push: per channel S_0 = frame * valid and N_0 = valid; level l + 1 has ceil(H_l / 2) x ceil(W_l / 2) cells whose S and N are the
sums over the up to four children (2y..2y+1, 2x..2x+1) that exist, up to 1 x 1.  Pull: at the top F = (2S + N) // (2N); going
down F_l = (2 S_l + N_l) // (2 N_l) where N_l > 0, else F_{l+1}[y // 2, x // 2].  F_0 is the fill; a valid pixel comes out as
its own byte ((2v + 1) // 2 = v).  Smooth: ``smooth`` Jacobi iterations in which every hole pixel becomes
(sum of its 3 x 3 neighbourhood of the previous iterate, border replicated, + 4) // 9 and valid pixels never change.
An empty hole or an empty ``valid`` returns a copy of the frame.  The bytes of the frame inside the hole are never read.

``warp_affine_bilinear(arr, M, object=None)``: custom_transforms.warp_affine's coordinate arithmetic with four taps - the same
fp64 sx, sy and floor, the fractions as fp32, weights 1 - f and f in fp32, the taps row-outer / column-inner as
acc = acc + val * (wy[j] * wx[i]) from +0.0, every product rounded before its add, val = 0 for a tap outside the source.  With
``object`` (bool [H,W]) it also returns n, the number of taps that lie inside the source AND on the object.

``compose(frame, background, mask, img_lut, gt_lut, flip, M_bg, M_fg, gain, bias)`` -> (image f32 [H,W,3], gt f32 [H,W]):
``flip`` mirrors the three byte arrays first; B = warp_affine(img_lut[background], M_bg), Fg = warp_affine(img_lut[frame], M_fg),
gt = warp_affine(gt_lut[mask], M_fg) (nearest); alpha from the four bilinear taps of ``mask != 0`` through M_fg: 0 where n == 0,
1 where n == 4, else the bilinear sum.  out = B where alpha == 0, Fg where alpha == 1, else B + alpha * (Fg - B) in fp32 with
the subtraction, the product and the sum each rounded; then out * gain[c] + bias[c], two fp32 roundings.  The two exact ends
are part of the definition: they let a kernel skip one of the two 16-tap gathers.  ``M_fg = None`` is no object (an empty or
hidden annotation): alpha = 0 everywhere and gt = 0.

``LucidDream(options)``: ``draw(rng)`` takes eleven ``rng.random()`` calls in the order of ``DRAWS`` (each lo + (hi - lo) u);
``matrices(draws, box, size)`` turns them into (M_bg, M_fg, gain, bias).  ``box`` is ``mask_box`` of the (flipped) mask:
(x0, y0, x1, y1), inclusive pixel indices, or None.  M_bg rotates and zooms about (w / 2, h / 2); M_fg about the box's centre
((x0 + x1) / 2, (y0 + y1) / 2), with fg_shift_x * box_w and fg_shift_y * box_h (box_w = x1 - x0 + 1) added to its translation
column; gain[c] = float32(contrast * tint_c), bias[c] = float32(brightness), c over the frame's three channels in storage order.
"""
from collections import namedtuple

import numpy as np

from dataloaders.custom_transforms import rotation_matrix, warp_affine

MAX_DILATE = 31   # fosvos_hip/limits.py: LUCID_MAX_DILATE
MAX_SMOOTH = 16   # fosvos_hip/limits.py: LUCID_MAX_SMOOTH

DRAWS = ("bg_rot", "bg_zoom", "fg_rot", "fg_zoom", "fg_shift_x", "fg_shift_y", "contrast", "tint_b", "tint_g", "tint_r",
         "brightness")
Draws = namedtuple("Draws", DRAWS)


# ------------------------------------------------------------------------------------------ the filled background
def dilated_hole(mask: np.ndarray, dilate: int) -> np.ndarray:
    """``mask != 0`` max-filtered over the (2 dilate + 1)^2 square, clipped at the border (the square is separable)."""
    hole = np.asarray(mask) != 0
    h, w = hole.shape
    for axis, n in ((0, h), (1, w)):
        grown = hole.copy()
        for d in range(1, min(int(dilate), n - 1) + 1):
            lo = [slice(None)] * 2
            hi = [slice(None)] * 2
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            grown[tuple(lo)] |= hole[tuple(hi)]
            grown[tuple(hi)] |= hole[tuple(lo)]
        hole = grown
    return hole


def push_pyramid(frame: np.ndarray, valid: np.ndarray):
    """[(S_l int64 [H_l,W_l,3], N_l int64 [H_l,W_l])] from level 0 up to 1 x 1."""
    s = frame.astype(np.int64) * valid[..., None]
    n = valid.astype(np.int64)
    levels = [(s, n)]
    while n.shape != (1, 1):
        h, w = n.shape
        ph, pw = h + (h & 1), w + (w & 1)  # children that do not exist add nothing
        s2 = np.zeros((ph, pw, 3), np.int64)
        n2 = np.zeros((ph, pw), np.int64)
        s2[:h, :w], n2[:h, :w] = s, n
        s = s2.reshape(ph // 2, 2, pw // 2, 2, 3).sum(axis=(1, 3))
        n = n2.reshape(ph // 2, 2, pw // 2, 2).sum(axis=(1, 3))
        levels.append((s, n))
    return levels


def pull_pyramid(levels):
    """[F_l int64 [H_l,W_l,3]] for every level of ``push_pyramid`` (F_0 first); the top must hold a valid pixel."""
    s, n = levels[-1]
    fills = [(2 * s + n[..., None]) // (2 * n[..., None])]
    for s, n in reversed(levels[:-1]):
        h, w = n.shape
        above = fills[0][np.arange(h)[:, None] // 2, np.arange(w)[None, :] // 2]
        own = (2 * s + n[..., None]) // (2 * np.maximum(n, 1)[..., None])
        fills.insert(0, np.where((n > 0)[..., None], own, above))
    return fills


def fill_background(frame: np.ndarray, mask: np.ndarray, dilate: int, smooth: int) -> np.ndarray:
    frame, mask = np.asarray(frame), np.asarray(mask)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.size == 0:
        raise ValueError("fill_background: a non-empty uint8 [H,W,3] frame, got %s %s" % (frame.dtype, frame.shape))
    if mask.dtype != np.uint8 or mask.shape != frame.shape[:2]:
        raise ValueError("fill_background: the mask of a %s frame is uint8 %s, got %s %s"
                         % (frame.shape, frame.shape[:2], mask.dtype, mask.shape))
    for name, v, hi in (("dilate", dilate, MAX_DILATE), ("smooth", smooth, MAX_SMOOTH)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
            raise ValueError("fill_background: %s must be an integer in 0..%d, got %r" % (name, hi, v))
    hole = dilated_hole(mask, dilate)
    valid = ~hole
    if not hole.any() or not valid.any():
        return frame.copy()
    fill = pull_pyramid(push_pyramid(frame, valid))[0]
    for _ in range(int(smooth)):
        p = np.pad(fill, ((1, 1), (1, 1), (0, 0)), mode="edge")
        h, w = hole.shape
        total = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
        fill = np.where(hole[..., None], (total + 4) // 9, fill)
    return np.ascontiguousarray(fill.astype(np.uint8))


# ------------------------------------------------------------------------------------------ the composition
def _source_coordinates(h: int, w: int, M):
    """warp_affine's own: the inverse of M in fp64 and every output pixel's (sx, sy)."""
    inv = np.linalg.inv(np.vstack([np.asarray(M, dtype=np.float64), [0.0, 0.0, 1.0]]))
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2], inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2]


def warp_affine_bilinear(arr: np.ndarray, M, object=None):
    arr = np.asarray(arr)
    if arr.ndim != 2 or arr.dtype != np.float32:
        raise ValueError("warp_affine_bilinear: a float32 [H,W] array, got %s %s" % (arr.dtype, arr.shape))
    h, w = arr.shape
    sx, sy = _source_coordinates(h, w, M)
    bx, by = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = (sx - bx).astype(np.float32), (sy - by).astype(np.float32)
    wx, wy = (np.float32(1) - fx, fx), (np.float32(1) - fy, fy)
    out = np.zeros((h, w), dtype=np.float32)
    n = np.zeros((h, w), dtype=np.int64)
    for j in range(2):
        yy = by + j
        for i in range(2):
            xx = bx + i
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
            val = np.where(ok, arr[yc, xc], np.float32(0.0))
            out = out + val * (wy[j] * wx[i])
            if object is not None:
                n += ok & np.asarray(object, dtype=bool)[yc, xc]
    assert out.dtype == np.float32
    return out if object is None else (out, n)


def object_alpha(mask: np.ndarray, M_fg) -> np.ndarray:
    """float32 [H,W]: how much of the (already flipped) object covers every output pixel; exactly 0 and exactly 1 at the ends."""
    obj = np.asarray(mask) != 0
    alpha, n = warp_affine_bilinear(obj.astype(np.float32), M_fg, object=obj)
    alpha = np.where(n == 4, np.float32(1.0), alpha)
    return np.where(n == 0, np.float32(0.0), alpha).astype(np.float32)


def compose(frame, background, mask, img_lut, gt_lut, flip, M_bg, M_fg, gain, bias):
    frame, background, mask = np.asarray(frame), np.asarray(background), np.asarray(mask)
    img_lut, gt_lut = np.asarray(img_lut, dtype=np.float32), np.asarray(gt_lut, dtype=np.float32)
    gain, bias = np.asarray(gain, dtype=np.float32), np.asarray(bias, dtype=np.float32)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or background.dtype != np.uint8 or \
            background.shape != frame.shape or mask.dtype != np.uint8 or mask.shape != frame.shape[:2]:
        raise ValueError("compose: uint8 frame and background [H,W,3] and mask [H,W], got %s, %s and %s"
                         % (frame.shape, background.shape, mask.shape))
    if img_lut.shape != (256, 3) or gt_lut.shape != (256,) or gain.shape != (3,) or bias.shape != (3,):
        raise ValueError("compose: img_lut [256,3], gt_lut [256], three gains and three biases")
    if flip:
        frame, background, mask = frame[:, ::-1], background[:, ::-1], mask[:, ::-1]
    chans = np.arange(3)[None, None, :]
    h, w = mask.shape
    B = warp_affine(img_lut[background, chans], M_bg)
    if M_fg is None:
        out, gt = B, np.zeros((h, w), dtype=np.float32)
    else:
        Fg = warp_affine(img_lut[frame, chans], M_fg)
        gt = warp_affine(gt_lut[mask], M_fg)
        alpha = object_alpha(mask, M_fg)[..., None]
        mixed = B + alpha * (Fg - B)
        out = np.where(alpha == 0, B, np.where(alpha == 1, Fg, mixed))
    out = out * gain[None, None, :] + bias[None, None, :]
    assert out.dtype == np.float32 and gt.dtype == np.float32
    return np.ascontiguousarray(out), np.ascontiguousarray(gt)


# ------------------------------------------------------------------------------------------ the draws
def mask_box(mask: np.ndarray):
    """(x0, y0, x1, y1), inclusive, of ``mask != 0``; None for an empty mask."""
    obj = np.asarray(mask) != 0
    if not obj.any():
        return None
    ys, xs = np.flatnonzero(obj.any(axis=1)), np.flatnonzero(obj.any(axis=0))
    return int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])


def mirrored_box(box, w: int):
    """``mask_box`` of the mirrored mask."""
    return None if box is None else (w - 1 - box[2], box[1], w - 1 - box[0], box[3])


class LucidDream(object):
    """The eleven draws of one composition and what they mean; ``options``: a fosvos_hip.options.LucidOptions, or anything
    with its eight range attributes."""

    RANGES = ("bg_rots", "bg_scales", "fg_rots", "fg_scales", "fg_shift", "fg_shift", "contrast", "tint", "tint", "tint",
              "brightness")

    def __init__(self, options):
        self.ranges = tuple(tuple(float(v) for v in getattr(options, name)) for name in self.RANGES)

    def draw(self, rng) -> Draws:
        return Draws(*[lo + (hi - lo) * rng.random() for lo, hi in self.ranges])

    def matrices(self, draws, box, size):
        d = Draws(*draws)
        h, w = size
        m_bg = rotation_matrix((w / 2, h / 2), d.bg_rot, d.bg_zoom)
        m_fg = None
        if box is not None:
            x0, y0, x1, y1 = box
            m_fg = rotation_matrix(((x0 + x1) / 2, (y0 + y1) / 2), d.fg_rot, d.fg_zoom)
            m_fg[0, 2] += d.fg_shift_x * (x1 - x0 + 1)
            m_fg[1, 2] += d.fg_shift_y * (y1 - y0 + 1)
        gain = np.array([d.contrast * d.tint_b, d.contrast * d.tint_g, d.contrast * d.tint_r], dtype=np.float32)
        bias = np.full(3, d.brightness, dtype=np.float32)
        return m_bg, m_fg, gain, bias
