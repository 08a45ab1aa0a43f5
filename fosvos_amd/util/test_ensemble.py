"""Test-time ensemble of the test pass, on the host in numpy: the net sees the frame mirrored and at a few other sizes, and its
answers are averaged back on the frame's grid (the last step of OSVOS-family evaluation; OnAVOS's published pipeline ends
with it).

These functions are the project's statement of that arithmetic.  The HIP kernels (csrc/ensemble.hip: fosvos_ensemble_views,
fosvos_ensemble_merge) are compared with them bit for bit, and the CPU branch of ``experiment_helper._ensemble_logits`` calls
them.  The taps of the resampling are util/frame_resample.taps, reused and not copied.

Views.  A view is ``(scale, flip)``.  ``view_sizes(h, w, scale) = (max(1, floor(h scale + 0.5)), max(1, floor(w scale + 0.5)))``
in Python floats.  ``views(flip, scales)`` lists, for each scale in the given order, ``(s, False)`` and then, with ``flip``,
``(s, True)``.  At most ``MAX_VIEWS`` views, scales in ``SCALE_RANGE``, every side of a view in ``1..MAX_SIDE``.

Resampling ``a`` float32 [H,W] to [ho,wo]: bilinear at half-pixel centres, clamped at the borders, with integer weights.
* ``(y0, y1, wy0, wy1) = taps(H, ho)`` and ``(x0, x1, wx0, wx1) = taps(W, wo)``; the formula serves ``n_src > n_dst`` as well
  (indices in range, the first weight positive, the second not negative, the two sum to ``2 n_dst``).
* In float64 and in exactly this order: ``top = a[y0][x0] wx0 + a[y0][x1] wx1``, ``bot = a[y1][x0] wx0 + a[y1][x1] wx1``,
  ``v = top wy0 + bot wy1``, and the result is ``v / float64(4 ho wo)``: one division.

Making the views of ``image`` float32 [N,3,H,W]: ``src`` is the image, mirrored along W where the view is flipped.  A view of
the frame's own size is ``src`` itself (a copy); any other is ``float32(resample(src[n][c], Hs, Ws))``.  The view
``(1.0, False)`` is the input itself.

Merging the V logit maps float32 [N,1,Hs_k,Ws_k] back on [H,W]: per view, in list order, ``u_k = float64(a)`` for a map of the
frame's own size and ``u_k = resample(a, H, W)`` otherwise, mirrored back along W where the view was flipped; ``acc = u_0``,
then ``acc += u_k`` for k = 1..V-1; the result is ``float32(acc / float64(V))``.  Non-finite values go through as IEEE
arithmetic gives them: a NaN reaches every output pixel one of whose four taps touches it, also where the tap's weight is 0.
"""
import math

import numpy as np

from util.frame_resample import taps

MAX_VIEWS = 8
SCALE_RANGE = (0.25, 4.0)
MAX_SIDE = 8192


def view_sizes(h: int, w: int, scale) -> tuple:
    return max(1, int(math.floor(h * float(scale) + 0.5))), max(1, int(math.floor(w * float(scale) + 0.5)))


def views(flip: bool, scales) -> list:
    out = []
    for s in scales:
        out.append((s, False))
        if flip:
            out.append((s, True))
    return out


def check_views(view_list, h: int, w: int) -> list:
    """The views as a list of ``(float scale, bool flip)``; raises ValueError where the list or a view's size is out of range."""
    view_list = list(view_list)
    if not 1 <= len(view_list) <= MAX_VIEWS:
        raise ValueError("{} views, outside [1, {}]".format(len(view_list), MAX_VIEWS))
    out = []
    for v in view_list:
        try:
            scale, flip = v
        except (TypeError, ValueError):
            raise ValueError("a view must be (scale, flip), got {!r}".format(v)) from None
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not SCALE_RANGE[0] <= scale <= SCALE_RANGE[1]:
            raise ValueError("a view's scale must be a number in [{:g}, {:g}], got {!r}".format(*SCALE_RANGE, scale))
        if not isinstance(flip, (bool, np.bool_)):
            raise ValueError("a view's flip must be a bool, got {!r}".format(flip))
        hs, ws = view_sizes(h, w, scale)
        if not (1 <= hs <= MAX_SIDE and 1 <= ws <= MAX_SIDE):
            raise ValueError("the view of scale {!r} of a {} frame is {}, sides outside 1..{}".format(
                scale, (h, w), (hs, ws), MAX_SIDE))
        out.append((float(scale), bool(flip)))
    return out


def resample(a_f32: np.ndarray, ho: int, wo: int) -> np.ndarray:
    """float32 [H,W] -> float64 [ho,wo]."""
    a = np.asarray(a_f32)
    if a.dtype != np.float32 or a.ndim != 2:
        raise ValueError("resample takes a float32 [H,W] map, got %s %s" % (a.dtype, a.shape))
    y0, y1, wy0, wy1 = taps(a.shape[0], ho)
    x0, x1, wx0, wx1 = taps(a.shape[1], wo)
    a = a.astype(np.float64)
    with np.errstate(invalid='ignore'):  # inf x 0 and inf - inf are NaN, as the arithmetic has it: nothing to warn about
        top = a[y0][:, x0] * wx0 + a[y0][:, x1] * wx1
        bot = a[y1][:, x0] * wx0 + a[y1][:, x1] * wx1
        v = top * wy0[:, None] + bot * wy1[:, None]
        return np.ascontiguousarray(v / np.float64(4 * ho * wo))


def make_views(image_f32: np.ndarray, view_list) -> list:
    """float32 [N,3,H,W] -> one float32 [N,3,Hs,Ws] per view."""
    image = np.asarray(image_f32)
    if image.dtype != np.float32 or image.ndim != 4:
        raise ValueError("make_views takes a float32 [N,C,H,W] image, got %s %s" % (image.dtype, image.shape))
    n, c, h, w = image.shape
    out = []
    for scale, flip in check_views(view_list, h, w):
        src = image[..., ::-1] if flip else image
        hs, ws = view_sizes(h, w, scale)
        if (hs, ws) == (h, w):
            out.append(np.array(src, dtype=np.float32, order='C', copy=True))
            continue
        view = np.empty((n, c, hs, ws), dtype=np.float32)
        for i in range(n):
            for j in range(c):
                view[i, j] = resample(np.ascontiguousarray(src[i, j]), hs, ws).astype(np.float32)
        out.append(view)
    return out


def merge(logits, view_list, h: int, w: int) -> np.ndarray:
    """The V maps float32 [N,1,Hs_k,Ws_k] of the views -> float32 [N,1,H,W]."""
    view_list = check_views(view_list, h, w)
    logits = [np.asarray(a) for a in logits]
    if len(logits) != len(view_list):
        raise ValueError("{} maps for {} views".format(len(logits), len(view_list)))
    n = logits[0].shape[0] if logits[0].ndim == 4 else 0
    acc = None
    for a, (scale, flip) in zip(logits, view_list):
        want = (n, 1) + view_sizes(h, w, scale)
        if a.dtype != np.float32 or a.shape != want:
            raise ValueError("the map of view {!r} must be float32 {}, got {} {}".format((scale, flip), want, a.dtype, a.shape))
        if a.shape[2:] == (h, w):
            u = a.astype(np.float64)
        else:
            u = np.stack([resample(np.ascontiguousarray(a[i, 0]), h, w)[None] for i in range(n)])
        if flip:
            u = u[..., ::-1]
        with np.errstate(invalid='ignore'):
            acc = np.array(u, dtype=np.float64, order='C', copy=True) if acc is None else acc + u
    return (acc / np.float64(len(view_list))).astype(np.float32)
