"""Following the object in a stream, on the host in numpy: the net looks at a WINDOW of the frame around the last mask, area-
averaged to the net's size, and its logits are painted back into that window.  The window of frame t + 1 comes from the logits
of frame t.

These functions are the project's statement of that arithmetic, as util/frame_resample.py is for the whole frame, whose
``box_weights`` and ``taps`` they reuse.  The HIP kernels (csrc/stream.hip: fosvos_frame_prep_window, fosvos_overlay_window,
fosvos_window_next) are compared with them - bit for bit for the prep, the boolean modes and the windows, everywhere but within
1e-9 of a rounding boundary for the soft modes.  Everything is in integers.

Windows.  A window is ``(y0, x0, Hw, Ww)`` as int32, in the coordinates of the picture the net sees and the segmenter returns
(after ``mirror``).  With frames of [Hf,Wf] and a net of [Hn,Wn] it is VALID when ``Hn <= Hw <= Hf``, ``Wn <= Ww <= Wf``,
``0 <= y0 <= Hf - Hw`` and ``0 <= x0 <= Wf - Ww``.  Any other window - negative or overflowing values included - IS READ AS THE
WHOLE FRAME ``(0, 0, Hf, Wf)``: ``sanitize`` is the first thing every function here does with a window, and every kernel.

* ``prepare_frame_window``: ``frame_resample.prepare_frame_scaled`` of the window's pixels - weights ``box_weights(Hw, Hn)``
  and ``box_weights(Ww, Wn)``, one float64 division by ``Hw Ww``, one rounding to float32, one float32 subtraction of the mean.
* ``logits_up_window``: inside the window ``frame_resample.logits_up(logits, Hw, Ww)``, ``4 Hw Ww`` times the interpolated
  logit.  Outside it nothing is object: the boolean mask is 0 and the soft prediction exactly 0.0.
* ``overlay_window``, ``mask_bytes_window``, ``apply_window``: the ``*_scaled`` functions with that prediction; the paint
  rules are util/frame_overlay.py's.
* ``ladder``: the ``levels + 1`` window sizes ``Hn + (Hf - Hn) k // levels`` (and the widths likewise), k = 0..levels.
* ``next_window``: the window for the next frame, see there.  There is no hysteresis between levels.
* ``track``: a segmenter's loop with ``roi``.
"""
import numpy as np

from util import frame_overlay as F
from util import frame_resample as R

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
MAX_LEVELS = 64
MAX_PAD = 4095
MAX_PERMILLE = 4000


# ---------------------------------------------------------------------------------------------- windows
def sanitize(window, hf: int, wf: int, hn: int, wn: int):
    """The window as four Python ints: itself where it is valid, else the whole frame."""
    R.check_sizes(hf, wf, hn, wn)
    w = np.asarray(window)
    if w.shape != (4,) or w.dtype.kind not in "iu":
        raise ValueError("a window is four integers (y0, x0, Hw, Ww), got %r" % (window,))
    y0, x0, hw, ww = (int(v) for v in w)
    for v in (y0, x0, hw, ww):
        if not INT32_MIN <= v <= INT32_MAX:
            raise ValueError("a window holds int32 values, got %r" % (window,))
    if hn <= hw <= hf and wn <= ww <= wf and 0 <= y0 <= hf - hw and 0 <= x0 <= wf - ww:
        return y0, x0, hw, ww
    return 0, 0, hf, wf


def ladder(hf: int, wf: int, hn: int, wn: int, levels: int):
    """The ``levels + 1`` window sizes [(Hw_k, Ww_k)]: level 0 is the net's size, level ``levels`` the whole frame."""
    R.check_sizes(hf, wf, hn, wn)
    _check_levels(levels)
    return [(hn + (hf - hn) * k // levels, wn + (wf - wn) * k // levels) for k in range(levels + 1)]


def _check_levels(levels) -> None:
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError("levels must be an integer in 1..%d, got %r" % (MAX_LEVELS, levels))


def _check_margin(margin_permille, min_pad) -> None:
    for v, top, name in ((margin_permille, MAX_PERMILLE, "margin_permille"), (min_pad, MAX_PAD, "min_pad")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= top:
            raise ValueError("%s must be an integer in 0..%d, got %r" % (name, top, v))


# ---------------------------------------------------------------------------------------------- in front of the net
def prepare_frame_window(img_u8: np.ndarray, window, hn: int, wn: int, mirror: bool = False) -> np.ndarray:
    """uint8 [Hf,Wf,3] -> float32 [1,3,Hn,Wn]: the net's input, the window of the (mirrored) frame at the net's size."""
    img = F.mirrored(img_u8, mirror)
    y0, x0, hw, ww = sanitize(window, img.shape[0], img.shape[1], hn, wn)
    return R.prepare_frame_scaled(np.ascontiguousarray(img[y0:y0 + hw, x0:x0 + ww]), hn, wn, False)


# ---------------------------------------------------------------------------------------------- behind the net
def logits_up_window(logits_f32: np.ndarray, window, hf: int, wf: int):
    """float32 [Hn,Wn] -> (float64 [Hf,Wf], bool [Hf,Wf]): ``4 Hw Ww`` times the interpolated logits inside the window (0.0
    outside, where the value means nothing), and the map of what is inside."""
    logits = np.asarray(logits_f32)
    if logits.dtype != np.float32 or logits.ndim != 2:
        raise ValueError("logits must be float32 [Hn,Wn], got %s %s" % (logits.dtype, logits.shape))
    y0, x0, hw, ww = sanitize(window, hf, wf, logits.shape[0], logits.shape[1])
    v = np.zeros((hf, wf), dtype=np.float64)
    inside = np.zeros((hf, wf), dtype=bool)
    v[y0:y0 + hw, x0:x0 + ww] = R.logits_up(logits, hw, ww)
    inside[y0:y0 + hw, x0:x0 + ww] = True
    return v, inside


def prediction_window(logits_f32: np.ndarray, window, hf: int, wf: int, boolean_mask: bool = True) -> np.ndarray:
    """float32 [Hn,Wn] logits -> float64 [Hf,Wf] in [0, 1]; exactly 0.0 outside the window."""
    v, inside = logits_up_window(logits_f32, window, hf, wf)
    _, _, hw, ww = sanitize(window, hf, wf, logits_f32.shape[0], logits_f32.shape[1])
    if boolean_mask:
        return np.where(inside & (v >= 0), 1.0, 0.0)
    return np.where(inside, 1.0 / (1.0 + np.exp(-(v / np.float64(4 * hw * ww)))), 0.0)


def overlay_window(img_u8: np.ndarray, logits: np.ndarray, window, mirror: bool = False, boolean_mask: bool = True,
                   color: str = 'r', alpha: float = 1.0) -> np.ndarray:
    """``frame_resample.overlay_scaled`` with the logits painted into the window: uint8 [Hf,Wf,3]."""
    c, alpha = F.check_color(color), F.check_alpha(alpha)
    img = F.mirrored(img_u8, mirror)
    p = prediction_window(logits, window, img.shape[0], img.shape[1], boolean_mask)
    out = np.array(img, copy=True)
    v = img[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
    out[:, :, c] = np.trunc(np.minimum(v, 255.0)).astype(np.uint8)
    return out


def mask_bytes_window(logits: np.ndarray, window, hf: int, wf: int, boolean_mask: bool = True) -> np.ndarray:
    """``frame_resample.mask_bytes_scaled`` with the logits painted into the window: uint8 [Hf,Wf]."""
    p = prediction_window(logits, window, hf, wf, boolean_mask)
    if boolean_mask:
        return (p * 255.0).astype(np.uint8)
    return (255 * p + 0.5).astype(np.uint8)


def apply_window(img_u8: np.ndarray, logits: np.ndarray, window, mirror: bool = False, overlay_on: bool = True,
                 boolean_mask: bool = True, color: str = 'r', alpha: float = 1.0) -> np.ndarray:
    """What a FrameSegmenter with ``roi`` returns for this frame, these logits and this window."""
    if overlay_on:
        return overlay_window(img_u8, logits, window, mirror, boolean_mask, color, alpha)
    F.check_color(color), F.check_alpha(alpha)
    hf, wf = F.check_frame(img_u8).shape[:2]
    return mask_bytes_window(logits, window, hf, wf, boolean_mask)


# ---------------------------------------------------------------------------------------------- the next window
def next_window(logits_f32: np.ndarray, window, hf: int, wf: int, levels: int = 8, margin_permille: int = 250,
                min_pad: int = 16, net_size=None):
    """The window for the next frame from this frame's logits (after any cleaning) and this frame's window:

    1. the bounding rows ``i_min..i_max`` and columns ``j_min..j_max`` of ``logits >= 0`` on the net's map (a NaN is never
       object, -0.0 is: the rule of ``merge_objects``);
    2. no such pixel: the whole frame - a lost object is looked for everywhere;
    3. the box in the frame, through the sanitised window: ``by0 = y0 + i_min Hw // Hn``, ``by1 = y0 + ((i_max + 1) Hw + Hn
       - 1) // Hn``, ``bx0`` and ``bx1`` likewise;
    4. ``pad = min_pad + (margin_permille max(by1 - by0, bx1 - bx0) + 999) // 1000``;
    5. ``need_h = min(Hf, by1 - by0 + 2 pad)``, ``need_w`` likewise;
    6. ``k`` = the smallest level of the ladder with ``Hw_k >= need_h`` and ``Ww_k >= need_w``;
    7. ``y0' = clamp((by0 + by1 - Hw_k) // 2, 0, Hf - Hw_k)`` with floor division, ``x0'`` likewise.

    ``net_size``: the ladder's smallest size where it is not the map's own (``window_of_mask``: a map of the frame's size)."""
    logits = np.asarray(logits_f32)
    if logits.dtype != np.float32 or logits.ndim != 2:
        raise ValueError("logits must be float32 [Hn,Wn], got %s %s" % (logits.dtype, logits.shape))
    hm, wm = logits.shape
    hn, wn = (hm, wm) if net_size is None else net_size
    sizes = ladder(hf, wf, hn, wn, levels)
    _check_margin(margin_permille, min_pad)
    y0, x0, hw, ww = sanitize(window, hf, wf, hm, wm)
    obj = logits >= 0
    if not obj.any():
        return 0, 0, hf, wf
    rows, cols = np.flatnonzero(obj.any(axis=1)), np.flatnonzero(obj.any(axis=0))
    i_min, i_max, j_min, j_max = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    by0, by1 = y0 + i_min * hw // hm, y0 + ((i_max + 1) * hw + hm - 1) // hm
    bx0, bx1 = x0 + j_min * ww // wm, x0 + ((j_max + 1) * ww + wm - 1) // wm
    pad = min_pad + (margin_permille * max(by1 - by0, bx1 - bx0) + 999) // 1000
    need_h, need_w = min(hf, by1 - by0 + 2 * pad), min(wf, bx1 - bx0 + 2 * pad)
    hk, wk = next((h, w) for h, w in sizes if h >= need_h and w >= need_w)
    ny0 = min(max((by0 + by1 - hk) // 2, 0), hf - hk)
    nx0 = min(max((bx0 + bx1 - wk) // 2, 0), wf - wk)
    return ny0, nx0, hk, wk


def window_of_mask(mask, hn: int, wn: int, levels: int = 8, margin_permille: int = 250, min_pad: int = 16):
    """``next_window`` applied to an annotation: a bool or uint8 [Hf,Wf] mask (non-zero = object) in the coordinates of the
    picture the net sees; the ladder is the one of a net of [Hn,Wn]."""
    mask = np.asarray(mask)
    if mask.dtype not in (np.uint8, np.bool_) or mask.ndim != 2:
        raise ValueError("a uint8 or bool [H,W] mask, got %s %s" % (mask.dtype, mask.shape))
    hf, wf = mask.shape
    as_logits = np.where(mask != 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    return next_window(as_logits, (0, 0, hf, wf), hf, wf, levels, margin_permille, min_pad, net_size=(hn, wn))


def track(frames, net_fn, hn: int, wn: int, mirror: bool = False, overlay_on: bool = True, boolean_mask: bool = True,
          color: str = 'r', alpha: float = 1.0, levels: int = 8, margin_permille: int = 250, min_pad: int = 16, window=None,
          clean_fn=None):
    """A segmenter's loop with ``roi``: ``net_fn(float32 [1,3,Hn,Wn]) -> float32 [Hn,Wn]`` logits, ``clean_fn(logits) ->
    logits`` the optional cleaning.  Frame 0 starts from ``window`` (None: the whole frame; ``window_of_mask`` of an
    annotation); every later frame's window comes from the logits of the frame before, after the cleaning.  Returns (the
    outputs, the window every frame used, the window the next frame would use)."""
    outs, used = [], []
    for img in frames:
        hf, wf = F.check_frame(img).shape[:2]
        if window is None:
            window = (0, 0, hf, wf)
        window = sanitize(window, hf, wf, hn, wn)
        logits = np.ascontiguousarray(net_fn(prepare_frame_window(img, window, hn, wn, mirror)), dtype=np.float32)
        if clean_fn is not None:
            logits = clean_fn(logits)
        outs.append(apply_window(img, logits, window, mirror, overlay_on, boolean_mask, color, alpha))
        used.append(window)
        window = next_window(logits, window, hf, wf, levels, margin_permille, min_pad)
    return outs, used, window
