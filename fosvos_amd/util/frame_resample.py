"""Streaming inference with the net at a size of its own, on the host in numpy: the frame is area-averaged down to the net's
size in front of the net, and the net's logits are interpolated back up to the frame's size behind it.

These functions are the project's statement of that arithmetic, as util/frame_overlay.py is for the unscaled path.  The HIP
kernels (csrc/stream.hip: fosvos_frame_prep_scaled, fosvos_overlay_scaled) are compared with them - bit for bit for the prep
and the boolean modes, everywhere but within 1e-9 of a rounding boundary for the soft modes.

Sizes are the frame's (Hf, Wf) and the net's (Hn, Wn), ``1 <= Hn <= Hf <= 8192`` and ``1 <= Wn <= Wf <= 8192``.

Downscale: the exact area average, in integers.
* Along one axis with ``n_src`` source and ``n_dst`` output samples, ``w[j][s] = max(0, min((s+1) n_dst, (j+1) n_src) -
  max(s n_dst, j n_src))``: the overlap of source pixel ``s`` with output pixel ``j`` in units of ``1 / n_dst`` source pixel.
  Every row sums to ``n_src``.
* ``S[i][j][c] = sum_y sum_x wy[i][y] wx[j][x] byte[y][x][c]``, an integer of at most ``255 Hf Wf``.
* ``image[c][i][j] = float32(float64(S) / float64(Hf Wf)) - float32(MEANVAL[c])``: one float64 division, one rounding to
  float32, one float32 subtraction.
* ``mirror`` flips the frame first; the weights are symmetric, so the result is the flipped result.

Upsample: bilinear at half-pixel centres, clamped at the borders, with integer weights.
* Along one axis ``num = (2 x + 1) n_src - n_dst``, ``i0 = num // (2 n_dst)``, ``r = num % (2 n_dst)``; ``num < 0``: ``i0 = 0,
  r = 0``; ``i0 >= n_src - 1``: ``i0 = n_src - 1, r = 0``; ``i1 = min(i0 + 1, n_src - 1)``; the weights are ``w0 = 2 n_dst - r``
  and ``w1 = r`` as float64.
* In float64 and in exactly this order: ``top = a[y0][x0] wx0 + a[y0][x1] wx1``, ``bot = a[y1][x0] wx0 + a[y1][x1] wx1``,
  ``v = top wy0 + bot wy1``.  ``v`` is ``4 Hf Wf`` times the interpolated logit.
* The boolean mask is ``v >= 0`` (no division; both zeros count as object).  The soft modes use ``x = v / float64(4 Hf Wf)``
  and then the float64 sigmoid, blend, truncation and rounding of util/frame_overlay.py.
"""
import numpy as np

from dataloaders.davis_2016 import MEANVAL
from util import frame_overlay as F

MAX_SIDE = 8192


def check_sizes(hf: int, wf: int, hn: int, wn: int) -> None:
    for v in (hf, wf, hn, wn):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("sizes must be integers, got %r" % (v,))
    if not (1 <= hn <= hf <= MAX_SIDE and 1 <= wn <= wf <= MAX_SIDE):
        raise ValueError("need 1 <= Hn <= Hf <= %d and 1 <= Wn <= Wf <= %d, got frame %s and net %s"
                         % (MAX_SIDE, MAX_SIDE, (hf, wf), (hn, wn)))


# ---------------------------------------------------------------------------------------------- downscale
def box_weights(n_src: int, n_dst: int) -> np.ndarray:
    """int64 [n_dst, n_src]: the overlap of [s n_dst, (s+1) n_dst) with [j n_src, (j+1) n_src)."""
    s = np.arange(n_src, dtype=np.int64)[None, :]
    j = np.arange(n_dst, dtype=np.int64)[:, None]
    return np.maximum(np.minimum((s + 1) * n_dst, (j + 1) * n_src) - np.maximum(s * n_dst, j * n_src), 0)


def area_sums(img_u8: np.ndarray, hn: int, wn: int) -> np.ndarray:
    """uint8 [Hf,Wf,3] -> int64 [Hn,Wn,3]: ``Hn Wn`` times the area sum of every output pixel (``Hf Wf`` times its mean)."""
    img = F.check_frame(img_u8)
    hf, wf, _ = img.shape
    check_sizes(hf, wf, hn, wn)
    rows = np.tensordot(box_weights(hf, hn), img.astype(np.int64), axes=(1, 0))   # [Hn,Wf,3]
    return np.ascontiguousarray(np.tensordot(rows, box_weights(wf, wn), axes=(1, 1)).transpose(0, 2, 1))


def prepare_frame_scaled(img_u8: np.ndarray, hn: int, wn: int, mirror: bool = False) -> np.ndarray:
    """uint8 [Hf,Wf,3] -> float32 [1,3,Hn,Wn]: the net's input at the net's size."""
    img = F.mirrored(img_u8, mirror)
    hf, wf, _ = img.shape
    s = area_sums(img, hn, wn)
    x = (s.astype(np.float64) / np.float64(hf * wf)).astype(np.float32) - np.array(MEANVAL, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1)[np.newaxis])


# ---------------------------------------------------------------------------------------------- upsample
def taps(n_src: int, n_dst: int):
    """(i0, i1, w0, w1) of every output sample: int64 indices, float64 weights that sum to ``2 n_dst``."""
    x = np.arange(n_dst, dtype=np.int64)
    num = (2 * x + 1) * n_src - n_dst
    i0, r = num // (2 * n_dst), num % (2 * n_dst)
    low = num < 0
    i0[low], r[low] = 0, 0
    high = i0 >= n_src - 1
    i0[high], r[high] = n_src - 1, 0
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, (2 * n_dst - r).astype(np.float64), r.astype(np.float64)


def logits_up(logits_f32: np.ndarray, hf: int, wf: int) -> np.ndarray:
    """float32 [Hn,Wn] -> float64 [Hf,Wf]: ``4 Hf Wf`` times the interpolated logits."""
    logits = np.asarray(logits_f32)
    if logits.dtype != np.float32 or logits.ndim != 2:
        raise ValueError("logits must be float32 [Hn,Wn], got %s %s" % (logits.dtype, logits.shape))
    hn, wn = logits.shape
    check_sizes(hf, wf, hn, wn)
    y0, y1, wy0, wy1 = taps(hn, hf)
    x0, x1, wx0, wx1 = taps(wn, wf)
    a = logits.astype(np.float64)
    top = a[y0][:, x0] * wx0 + a[y0][:, x1] * wx1
    bot = a[y1][:, x0] * wx0 + a[y1][:, x1] * wx1
    return np.ascontiguousarray(top * wy0[:, None] + bot * wy1[:, None])  # (fancy indexing leaves the columns first)


def prediction_scaled(logits_f32: np.ndarray, hf: int, wf: int, boolean_mask: bool = True) -> np.ndarray:
    """float32 [Hn,Wn] logits -> float64 [Hf,Wf] in [0, 1]."""
    v = logits_up(logits_f32, hf, wf)
    if boolean_mask:
        return np.where(v >= 0, 1.0, 0.0)
    return 1.0 / (1.0 + np.exp(-(v / np.float64(4 * hf * wf))))


def overlay_scaled(img_u8: np.ndarray, logits: np.ndarray, mirror: bool = False, boolean_mask: bool = True, color: str = 'r',
                   alpha: float = 1.0) -> np.ndarray:
    """``frame_overlay.overlay`` with logits of the net's size: uint8 [Hf,Wf,3]."""
    c, alpha = F.check_color(color), F.check_alpha(alpha)
    img = F.mirrored(img_u8, mirror)
    p = prediction_scaled(logits, img.shape[0], img.shape[1], boolean_mask)
    out = np.array(img, copy=True)
    v = img[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
    out[:, :, c] = np.trunc(np.minimum(v, 255.0)).astype(np.uint8)
    return out


def mask_bytes_scaled(logits: np.ndarray, hf: int, wf: int, boolean_mask: bool = True) -> np.ndarray:
    """``frame_overlay.mask_bytes`` at the frame's size: uint8 [Hf,Wf]."""
    p = prediction_scaled(logits, hf, wf, boolean_mask)
    if boolean_mask:
        return (p * 255.0).astype(np.uint8)
    return (255 * p + 0.5).astype(np.uint8)


def apply_scaled(img_u8: np.ndarray, logits: np.ndarray, mirror: bool = False, overlay_on: bool = True,
                 boolean_mask: bool = True, color: str = 'r', alpha: float = 1.0) -> np.ndarray:
    """What a FrameSegmenter with ``net_size`` returns for this frame and these logits."""
    if overlay_on:
        return overlay_scaled(img_u8, logits, mirror, boolean_mask, color, alpha)
    F.check_color(color), F.check_alpha(alpha)
    hf, wf = F.check_frame(img_u8).shape[:2]
    return mask_bytes_scaled(logits, hf, wf, boolean_mask)
