"""The per-frame arithmetic of streaming inference, on the host in numpy: what happens to a raw camera frame in front of
the net and to the net's logits behind it (reference: src/run_webcam.py:81-133, ``apply_network``).

These functions are the project's statement of that arithmetic.  The HIP kernels (csrc/stream.hip: fosvos_frame_prep,
fosvos_overlay) are compared with them - bit for bit for the prep and the boolean modes, everywhere but within 1e-9 of a
rounding boundary for the soft modes - and ``run_webcam`` writes what they define.

A frame is uint8 [H,W,3] in BGR order, as a camera (or ``cv2.imread``) delivers it.  With ``mirror`` it is flipped left to
right first (``cv2.flip(img, 1)``); the net then sees the flipped frame, so its logits already are in output order.

* ``prepare_frame``: ``float32(byte) - float32(MEANVAL[c])``, HWC -> [1,3,H,W].
* ``prediction``: boolean ``1.0 where logit >= 0 else 0.0`` (``+0.0`` and ``-0.0`` both count as object, as in
  ``davis_measures`` / fosvos_jf_counts); soft ``1 / (1 + exp(-float64(x)))``.
* ``overlay``: channel ``c`` of ``color`` becomes ``uint8(trunc(min(float64(byte_c) + (float64(alpha) * 255.0) * p, 255.0)))``;
  the other two channels are the (mirrored) input bytes.
* ``mask_bytes`` (no overlay): boolean 0 / 255; soft ``uint8(255 * p + 0.5)``.

Deviations from the reference, on purpose:
* The reference takes the sigmoid in float32 and tests ``>= 0.5``.  The float32 sigmoid rounds to exactly 0.5 for logits in
  about (-2**-24, 0) as well, so its mask also holds those few negative logits; here the mask is ``logit >= 0``, the same
  one the scorer counts.  The soft overlay is taken in float64 throughout; the reference's float32 sigmoid moves a byte by
  one level at most.
* Without overlay the reference shows the float prediction itself (``cv2.imshow`` of values in [0, 1]); here the output is
  bytes, so that every mode yields a uint8 frame that can be copied, written and compared.
"""
import math

import numpy as np

from dataloaders.davis_2016 import MEANVAL

COLOR_CHANNEL = {'b': 0, 'g': 1, 'r': 2}
# the op's modes (include/fosvos_hip.h, fosvos_overlay): (overlay, boolean_mask) -> mode
MODES = {(True, True): 0, (True, False): 1, (False, True): 2, (False, False): 3}


def check_frame(img_u8) -> np.ndarray:
    if not isinstance(img_u8, np.ndarray) or img_u8.dtype != np.uint8:
        raise ValueError("a frame must be a uint8 numpy array, got %s" % (getattr(img_u8, 'dtype', type(img_u8)),))
    if img_u8.ndim != 3 or img_u8.shape[2] != 3 or img_u8.size == 0:
        raise ValueError("a frame must be a non-empty [H,W,3], got %s" % (img_u8.shape,))
    return img_u8


def check_alpha(alpha) -> float:
    alpha = float(alpha)
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError("overlay alpha must be a finite number >= 0, got %r" % (alpha,))
    return alpha


def check_color(color) -> int:
    if color not in COLOR_CHANNEL:
        raise ValueError("overlay color must be one of 'r', 'g', 'b', got %r" % (color,))
    return COLOR_CHANNEL[color]


def _check_logits(logits, shape) -> np.ndarray:
    logits = np.asarray(logits)
    if logits.dtype != np.float32 or logits.shape != tuple(shape):
        raise ValueError("logits must be float32 %s, got %s %s" % (tuple(shape), logits.dtype, logits.shape))
    return logits


def mirrored(img_u8: np.ndarray, mirror: bool) -> np.ndarray:
    return check_frame(img_u8)[:, ::-1] if mirror else check_frame(img_u8)


def prepare_frame(img_u8: np.ndarray, mirror: bool = False) -> np.ndarray:
    """uint8 [H,W,3] -> float32 [1,3,H,W]: the net's input."""
    img = mirrored(img_u8, mirror)
    x = img.astype(np.float32) - np.array(MEANVAL, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(2, 0, 1)[np.newaxis])


def prediction(logits: np.ndarray, boolean_mask: bool = True) -> np.ndarray:
    """float32 [H,W] logits -> float64 [H,W] in [0, 1]."""
    logits = np.asarray(logits)
    if logits.dtype != np.float32 or logits.ndim != 2:
        raise ValueError("logits must be float32 [H,W], got %s %s" % (logits.dtype, logits.shape))
    if boolean_mask:
        return np.where(logits >= 0, 1.0, 0.0)
    return 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))


def overlay(img_u8: np.ndarray, logits: np.ndarray, mirror: bool = False, boolean_mask: bool = True, color: str = 'r',
            alpha: float = 1.0) -> np.ndarray:
    """The (mirrored) frame with the prediction added to one colour channel: uint8 [H,W,3]."""
    c, alpha = check_color(color), check_alpha(alpha)
    img = mirrored(img_u8, mirror)
    p = prediction(_check_logits(logits, img.shape[:2]), boolean_mask)
    out = np.array(img, copy=True)
    v = img[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
    out[:, :, c] = np.trunc(np.minimum(v, 255.0)).astype(np.uint8)
    return out


def mask_bytes(logits: np.ndarray, boolean_mask: bool = True) -> np.ndarray:
    """The prediction alone as a greyscale image: uint8 [H,W]."""
    p = prediction(logits, boolean_mask)
    if boolean_mask:
        return (p * 255.0).astype(np.uint8)
    return (255 * p + 0.5).astype(np.uint8)


def apply(img_u8: np.ndarray, logits: np.ndarray, mirror: bool = False, overlay_on: bool = True, boolean_mask: bool = True,
          color: str = 'r', alpha: float = 1.0) -> np.ndarray:
    """What a FrameSegmenter returns for this frame and these logits."""
    if overlay_on:
        return overlay(img_u8, logits, mirror, boolean_mask, color, alpha)
    check_color(color), check_alpha(alpha)
    return mask_bytes(_check_logits(logits, check_frame(img_u8).shape[:2]), boolean_mask)
