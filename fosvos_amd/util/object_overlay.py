"""Several objects in streaming inference, on the host in numpy: the logits of the K per-object nets of one frame become a
label map, and the label map a palette overlay on the frame.

These functions are the byte-for-byte references of the HIP kernels (csrc/stream.hip: fosvos_overlay_objects,
fosvos_overlay_objects_scaled), as util/frame_overlay.py and util/frame_resample.py are for the single-object ones; they are
built from those modules' functions and from util/object_merge.py.  There are no soft modes: several objects are always
decided by the arg-max, so every comparison with the kernels is exact equality.

* ``labels``: object k is VALID where its value is ``>= 0`` (a NaN never is, ``-0.0`` is); no valid object: label 0;
  otherwise 1 + the lowest k among the valid ones that hold the largest value (``object_merge.merge_labels``).  With a frame
  size ``(hf, wf)`` the values are ``frame_resample.logits_up`` of every map: float64, ``4 Hf Wf`` times the bilinear
  logit.  That positive common factor does not change the order, so it is never divided out.
* ``overlay``: the (mirrored) frame; a pixel of label k > 0 gets, per BGR channel c, the colour ``col = palette[k][2 - c]``
  (the palette is RGB) blended in float64, one operation at a time: ``v = float64(b) + alpha * (float64(col) - float64(b))``,
  ``out = uint8(trunc(v + 0.5))``.  alpha 0 is the frame, alpha 1 the pure colour, both exactly.

This is NOT the single-object overlay with more colours: ``frame_overlay.overlay`` ADDS ``alpha * 255`` to one channel,
clamps, and takes any ``alpha >= 0``; here all three channels are BLENDED towards a palette colour and ``alpha`` is a finite
number in [0, 1].
"""
import math

import numpy as np

from util import frame_overlay as F
from util import frame_resample as R
from util import object_merge as M


def check_alpha(alpha) -> float:
    """A finite number in [0, 1] (unlike ``frame_overlay.check_alpha``, which takes any alpha >= 0: that overlay adds, this
    one blends)."""
    alpha = float(alpha)
    if not (math.isfinite(alpha) and 0.0 <= alpha <= 1.0):
        raise ValueError("palette overlay alpha must be a finite number in [0, 1], got %r" % (alpha,))
    return alpha


def check_palette(palette) -> np.ndarray:
    """uint8 [256,3] RGB; None is the DAVIS palette."""
    if palette is None:
        return M.davis_palette()
    if not isinstance(palette, np.ndarray) or palette.dtype != np.uint8 or palette.shape != (256, 3):
        raise ValueError("a palette must be a uint8 numpy array [256,3], got %s %s"
                         % (getattr(palette, 'dtype', type(palette)), getattr(palette, 'shape', None)))
    return palette


def _maps(logits):
    maps = [np.asarray(m) for m in logits]
    if not 1 <= len(maps) <= M.MAX_OBJECTS:
        raise ValueError("%d logit maps, outside [1, %d]" % (len(maps), M.MAX_OBJECTS))
    for m in maps:
        if m.dtype != np.float32 or m.ndim != 2 or m.shape != maps[0].shape or m.size == 0:
            raise ValueError("the logits are K float32 maps of one shape [Hn,Wn], got %s %s" % (m.dtype, m.shape))
    return maps


def labels(logits, hf=None, wf=None) -> np.ndarray:
    """K float32 maps [Hn,Wn] (1 <= K <= ``object_merge.MAX_OBJECTS``) -> uint8 [H,W] labels; with ``hf, wf`` at the frame's
    size [Hf,Wf], decided on the maps interpolated up to it in float64 (``frame_resample.logits_up``)."""
    maps = _maps(logits)
    if (hf is None) != (wf is None):
        raise ValueError("hf and wf are the frame's size: give both or neither")
    if hf is None:
        return M.merge_labels(np.stack(maps)[:, np.newaxis])[0]
    v = np.stack([R.logits_up(m, hf, wf) for m in maps])       # float64 [K,Hf,Wf]
    valid = v >= 0                                             # (False for NaN)
    best = np.argmax(np.where(valid, v, -np.inf), axis=0)      # the first of equal maxima: the lowest k
    return np.where(valid.any(axis=0), best + 1, 0).astype(np.uint8)


def overlay(img_u8: np.ndarray, logits, mirror: bool = False, palette=None, alpha: float = 0.5, hf=None, wf=None) -> np.ndarray:
    """The (mirrored) frame with every labelled pixel blended towards its object's palette colour: uint8 [H,W,3] (BGR).
    ``alpha`` is a finite number in [0, 1] - NOT the single-object overlay's, which adds to one channel and takes
    alpha > 1.  ``hf, wf`` (the frame's own size) say that the logits are at a net's size of their own."""
    alpha, palette = np.float64(check_alpha(alpha)), check_palette(palette)
    img = F.mirrored(img_u8, mirror)
    if hf is not None and (hf, wf) != img.shape[:2]:
        raise ValueError("hf, wf must be the frame's size %s, got %s" % (img.shape[:2], (hf, wf)))
    lab = labels(logits, hf, wf)
    if lab.shape != img.shape[:2]:
        raise ValueError("the labels are %s, the frame is %s" % (lab.shape, img.shape[:2]))
    b = img.astype(np.float64)
    col = palette[lab][:, :, ::-1].astype(np.float64)          # RGB -> the frame's BGR
    v = b + alpha * (col - b)
    painted = np.trunc(v + 0.5).astype(np.uint8)
    return np.where((lab > 0)[:, :, np.newaxis], painted, img)


def apply(img_u8: np.ndarray, logits, mirror: bool = False, overlay_on: bool = True, palette=None, alpha: float = 0.5,
          hf=None, wf=None) -> np.ndarray:
    """What an ObjectSegmenter returns for this frame and these logits: the overlay, or the label map."""
    if overlay_on:
        return overlay(img_u8, logits, mirror, palette, alpha, hf, wf)
    check_alpha(alpha), check_palette(palette)
    lab = labels(logits, hf, wf)
    if lab.shape != F.check_frame(img_u8).shape[:2]:
        raise ValueError("the labels are %s, the frame is %s" % (lab.shape, img_u8.shape[:2]))
    return lab
