"""Edge-aware upsampling of the stream's logits, on the host in numpy: the (fast) guided filter (He, Sun, Tang 2013; He, Sun
2015) with the frame itself as the guide.  In a small window around every net pixel a linear model ``logit ~ a guide + b``
is fitted between the net's output and the picture the net saw; ``a`` and ``b`` are smoothed, interpolated up to the frame's
size - they, not the logits - and applied to the full-resolution pixel.  The mask's edge then lies where the frame's edge
lies, not where the net's coarse pixels end.

These functions are the project's statement of that arithmetic, as util/frame_resample.py is for the plain upsampling.  The
HIP kernels (csrc/guided.hip: fosvos_guided_coefficients; csrc/stream.hip: fosvos_overlay_guided) are compared with them -
bit for bit for the coefficient maps and the boolean modes, everywhere but within 1e-9 of a rounding boundary for the soft
modes.  So that a kernel can match: every float64 operation below is ONE correctly rounded IEEE operation, the order of every
addition is fixed, and nothing is contracted into a fused multiply-add.

Inputs per frame: ``image`` float32 [3,Hn,Wn], exactly what the prep made for the net; ``logits`` float32 [Hn,Wn]; ``radius``
r, an integer in 1..8; ``eps``, a finite float64 in [1e-3, 1e9]; ``clip``, a finite float64 in (0, 1e4].

Guide and target at the net's size:
* ``g = f64(image[0]) + f64(image[1]) + f64(image[2])`` - exact: three float32 values in float64.
* ``p = min(max(f64(logit), -clip), clip)``, and a NaN logit gives ``-clip``: "NaN is never object".  +-inf and the cleaning's
  fill are clipped the same way, so every later value is finite.

Window of (y, x): rows ``max(0, y-r) .. min(Hn-1, y+r)``, columns ``max(0, x-r) .. min(Wn-1, x+r)``; ``n`` is its pixel count,
the integer product of the two extents as float64.

Box sum ``B(v)``, in a fixed order, direct (no running sum, no integral image; at most 17 terms a pass):
* ``V[y][x] = ((0.0 + v[ya][x]) + v[ya+1][x]) + ...`` over the window's rows, ascending;
* ``S[y][x] = ((0.0 + V[y][xa]) + V[y][xa+1]) + ...`` over its columns, ascending.

Fit: ``Sg = B(g)``, ``Sp = B(p)``, ``Sgp = B(g*p)``, ``Sgg = B(g*g)`` (each product one rounded multiply);
``num = n*Sgp - Sg*Sp``; ``den = (n*Sgg - Sg*Sg) + (eps*n)*n``; ``a = num / den``; ``b = (Sp - a*Sg) / n``.  These are the
textbook ``cov / (var + eps)`` and ``mean_p - a mean_g`` with numerator and denominator scaled by ``n*n``: sums instead of
means keep the window's pixel count out of every intermediate rounding but the last division.  ``den > 0`` for every input:
the variance term's rounding error is about ``1e-11 n*n`` at this guide's magnitude (``|g| <= 765``) against ``eps n*n >=
1e-3 n*n``.

Smooth: ``abar = B(a) / n``, ``bbar = B(b) / n``; ``coeff = [abar, bbar]``, float64 [2,Hn,Wn].

Apply at the frame's size: ``frame_resample.taps`` in both axes, in ``logits_up``'s order, on the two float64 maps: ``A`` is
``4 Hf Wf`` times the interpolated ``abar``, ``Bv`` likewise of ``bbar``.  The full-resolution guide of the (mirrored) frame
pixel is ``I = (f64(byte0) - m0) + (f64(byte1) - m1) + (f64(byte2) - m2)``, ``m_c = f64(f32(MEANVAL[c]))`` - exact.  ``v = (A*I)
+ Bv``.  The boolean mask is ``v >= 0``; the soft modes take ``x = v / f64(4 Hf Wf)`` into the float64 sigmoid, blend,
truncation and rounding of util/frame_overlay.py.  ``Hn == Hf`` and ``Wn == Wf`` are allowed: the taps are then the identity
and the filter still snaps the mask to the frame's edges.  ``mirror``: the prep mirrored the frame, the logits are in
mirrored order and the paint reads the mirrored pixel - the result is the result on the flipped frame.
"""
import math

import numpy as np

from dataloaders.davis_2016 import MEANVAL
from util import frame_overlay as F
from util import frame_resample as R

MAX_RADIUS = 8
EPS_RANGE = (1e-3, 1e9)
MAX_CLIP = 1e4


def check_params(radius, eps, clip):
    """(radius, float64 eps, float64 clip), or ValueError with the range."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError("radius must be an integer in 1..%d, got %r" % (MAX_RADIUS, radius))
    for name, v in (("eps", eps), ("clip", clip)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
    if not EPS_RANGE[0] <= eps <= EPS_RANGE[1]:
        raise ValueError("eps must be in [%g, %g], got %r" % (EPS_RANGE[0], EPS_RANGE[1], eps))
    if not 0.0 < clip <= MAX_CLIP:
        raise ValueError("clip must be in (0, %g], got %r" % (MAX_CLIP, clip))
    return int(radius), np.float64(eps), np.float64(clip)


# ---------------------------------------------------------------------------------------------- at the net's size
def window_count(h: int, w: int, r: int) -> np.ndarray:
    """float64 [h,w]: ``n``, the pixel count of every window, from the indices."""
    y, x = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    ny = np.minimum(h - 1, y + r) - np.maximum(0, y - r) + 1
    nx = np.minimum(w - 1, x + r) - np.maximum(0, x - r) + 1
    return (ny[:, None] * nx[None, :]).astype(np.float64)


def _sum_axis0(v: np.ndarray, r: int) -> np.ndarray:
    """The window's rows added in ascending order onto 0.0.  Row offset d meets output row y at source row y + d; over d
    ascending every y adds its rows ya .. yb in turn."""
    h = v.shape[0]
    out = np.zeros_like(v)
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(h, h - d)
        if lo < hi:
            out[lo:hi] = out[lo:hi] + v[lo + d:hi + d]
    return out


def box_sum(v: np.ndarray, r: int) -> np.ndarray:
    """``B(v)`` of a float64 [h,w] map: rows first, then columns, each ascending from 0.0."""
    v = np.asarray(v)
    if v.dtype != np.float64 or v.ndim != 2:
        raise ValueError("box_sum takes a float64 [h,w] map, got %s %s" % (v.dtype, v.shape))
    return np.ascontiguousarray(_sum_axis0(np.ascontiguousarray(_sum_axis0(v, r).T), r).T)


def guide_and_target(image: np.ndarray, logits: np.ndarray, clip):
    """(g, p) float64 [Hn,Wn]."""
    image, logits = np.asarray(image), np.asarray(logits)
    if image.dtype != np.float32 or image.ndim != 3 or image.shape[0] != 3 or image.size == 0:
        raise ValueError("image must be a non-empty float32 [3,Hn,Wn], got %s %s" % (image.dtype, image.shape))
    if logits.dtype != np.float32 or logits.shape != image.shape[1:]:
        raise ValueError("logits must be float32 %s, got %s %s" % (image.shape[1:], logits.dtype, logits.shape))
    clip = np.float64(clip)
    g = (image[0].astype(np.float64) + image[1].astype(np.float64)) + image[2].astype(np.float64)
    x = logits.astype(np.float64)
    with np.errstate(invalid="ignore"):
        p = np.where(x >= -clip, x, -clip)   # a NaN compares false: -clip
        p = np.where(p <= clip, p, clip)
    return g, p


def fit(image: np.ndarray, logits: np.ndarray, radius, eps, clip):
    """(a, b, den) float64 [Hn,Wn]: the linear model of every window, and the denominator it divided by."""
    r, eps, clip = check_params(radius, eps, clip)
    g, p = guide_and_target(image, logits, clip)
    n = window_count(g.shape[0], g.shape[1], r)
    sg, sp, sgp, sgg = box_sum(g, r), box_sum(p, r), box_sum(g * p, r), box_sum(g * g, r)
    num = n * sgp - sg * sp
    den = (n * sgg - sg * sg) + (eps * n) * n
    a = num / den
    b = (sp - a * sg) / n
    return a, b, den


def coefficients(image: np.ndarray, logits: np.ndarray, radius=4, eps=400.0, clip=6.0) -> np.ndarray:
    """float32 [3,Hn,Wn] image and float32 [Hn,Wn] logits -> float64 [2,Hn,Wn] = [abar, bbar]."""
    a, b, _ = fit(image, logits, radius, eps, clip)
    n = window_count(a.shape[0], a.shape[1], int(radius))
    return np.ascontiguousarray(np.stack([box_sum(a, int(radius)) / n, box_sum(b, int(radius)) / n]))


# ---------------------------------------------------------------------------------------------- at the frame's size
def _check_coeff(coeff) -> np.ndarray:
    coeff = np.asarray(coeff)
    if coeff.dtype != np.float64 or coeff.ndim != 3 or coeff.shape[0] != 2 or coeff.size == 0:
        raise ValueError("coeff must be a non-empty float64 [2,Hn,Wn], got %s %s" % (coeff.dtype, coeff.shape))
    return coeff


def map_up(m: np.ndarray, hf: int, wf: int) -> np.ndarray:
    """float64 [Hn,Wn] -> float64 [Hf,Wf]: ``4 Hf Wf`` times the interpolated map, ``frame_resample.logits_up`` on float64."""
    hn, wn = m.shape
    R.check_sizes(hf, wf, hn, wn)
    y0, y1, wy0, wy1 = R.taps(hn, hf)
    x0, x1, wx0, wx1 = R.taps(wn, wf)
    top = m[y0][:, x0] * wx0 + m[y0][:, x1] * wx1
    bot = m[y1][:, x0] * wx0 + m[y1][:, x1] * wx1
    return np.ascontiguousarray(top * wy0[:, None] + bot * wy1[:, None])


def frame_guide(img_u8: np.ndarray, mirror: bool = False) -> np.ndarray:
    """uint8 [Hf,Wf,3] -> float64 [Hf,Wf]: ``I`` of the (mirrored) frame."""
    img = F.mirrored(img_u8, mirror).astype(np.float64)
    m = np.array(MEANVAL, dtype=np.float32).astype(np.float64)
    return np.ascontiguousarray(((img[:, :, 0] - m[0]) + (img[:, :, 1] - m[1])) + (img[:, :, 2] - m[2]))


def refined_up(coeff: np.ndarray, img_u8: np.ndarray, mirror: bool = False) -> np.ndarray:
    """float64 [Hf,Wf]: ``v``, ``4 Hf Wf`` times the refined logit of every frame pixel."""
    coeff = _check_coeff(coeff)
    hf, wf = F.check_frame(img_u8).shape[:2]
    return map_up(coeff[0], hf, wf) * frame_guide(img_u8, mirror) + map_up(coeff[1], hf, wf)


def prediction_guided(coeff: np.ndarray, img_u8: np.ndarray, mirror: bool = False, boolean_mask: bool = True) -> np.ndarray:
    """float64 [Hf,Wf] in [0, 1]."""
    v = refined_up(coeff, img_u8, mirror)
    if boolean_mask:
        return np.where(v >= 0, 1.0, 0.0)
    hf, wf = v.shape
    return 1.0 / (1.0 + np.exp(-(v / np.float64(4 * hf * wf))))


def overlay_guided(img_u8: np.ndarray, coeff: np.ndarray, mirror: bool = False, boolean_mask: bool = True, color: str = 'r',
                   alpha: float = 1.0) -> np.ndarray:
    """``frame_resample.overlay_scaled`` with the refined logits: uint8 [Hf,Wf,3]."""
    c, alpha = F.check_color(color), F.check_alpha(alpha)
    img = F.mirrored(img_u8, mirror)
    p = prediction_guided(coeff, img_u8, mirror, boolean_mask)
    out = np.array(img, copy=True)
    v = img[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
    out[:, :, c] = np.trunc(np.minimum(v, 255.0)).astype(np.uint8)
    return out


def mask_bytes_guided(img_u8: np.ndarray, coeff: np.ndarray, mirror: bool = False, boolean_mask: bool = True) -> np.ndarray:
    """``frame_resample.mask_bytes_scaled`` with the refined logits: uint8 [Hf,Wf].  The frame is read here too."""
    p = prediction_guided(coeff, img_u8, mirror, boolean_mask)
    if boolean_mask:
        return (p * 255.0).astype(np.uint8)
    return (255 * p + 0.5).astype(np.uint8)


def apply_guided(img_u8: np.ndarray, image: np.ndarray, logits: np.ndarray, mirror: bool = False, overlay_on: bool = True,
                 boolean_mask: bool = True, color: str = 'r', alpha: float = 1.0, radius=4, eps=400.0, clip=6.0) -> np.ndarray:
    """What a FrameSegmenter with ``refine`` returns for this frame, the image its prep made of it ([3,Hn,Wn] or [1,3,Hn,Wn])
    and these logits."""
    image = np.asarray(image)
    if image.ndim == 4 and image.shape[0] == 1:
        image = image[0]
    coeff = coefficients(image, logits, radius, eps, clip)
    if overlay_on:
        return overlay_guided(img_u8, coeff, mirror, boolean_mask, color, alpha)
    F.check_color(color), F.check_alpha(alpha)
    return mask_bytes_guided(img_u8, coeff, mirror, boolean_mask)
