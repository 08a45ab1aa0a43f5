"""Online adaptation of the test pass (as in OnAVOS): pseudo-labels from the net's own output, and a class-balanced loss
that ignores pixels.  These functions are the definitions, in numpy, of what the kernels of csrc/adapt.hip and the void form
of csrc/loss.hip compute; the tests compare ``far_from`` and ``adapt_labels`` with exact equality.

  far_from       fosvos_distance_gate         "further than `distance` from every set pixel", integer arithmetic
  adapt_labels   fosvos_adapt_labels          positives / negatives / void of one frame
  cbce_void      fosvos_cbce_loss_frames_void the class-balanced loss over the valid pixels, float64
  cbce_void_torch                             the same as a torch-autograd expression (CPU stand-in nets)

No torch at import and no library load: importable anywhere.
"""
from __future__ import division

import numpy as np

MAX_DISTANCE = 4095  # what the kernels take (uint16 column distances saturated at distance + 1)


def _check_mask(mask, what):
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype not in (np.uint8, np.bool_):
        raise ValueError('{}: mask must be a uint8 or bool [H,W] array, got {} {}'.format(what, mask.dtype, mask.shape))
    return mask


def _check_distance(distance, what, name='distance'):
    if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, np.integer)) \
            or not 0 <= distance <= MAX_DISTANCE:
        raise ValueError('{}: {} must be an integer in 0..{}, got {!r}'.format(what, name, MAX_DISTANCE, distance))
    return int(distance)


def far_from(mask, distance, invert=False):
    """uint8 [H,W]: 1 at p iff every set pixel q has ``(py - qy)**2 + (px - qx)**2 > distance**2``, where q is set when
    ``(mask[q] != 0) != invert``.  No set pixel: all 1 (vacuously true).  Only pixels inside the frame count, so
    ``far_from(mask, e, invert=True)`` is the erosion of ``mask`` by the Euclidean disk of radius ``e`` with the frame border
    not eating into it.

    Computed exactly in integers by the separation the kernels use: g[y,x] = the vertical distance to the nearest set pixel
    of column x (saturated at distance + 1), then p is near iff some x' has ``(x - x')**2 + g[y,x']**2 <= distance**2``."""
    mask = _check_mask(mask, 'far_from')
    d = _check_distance(distance, 'far_from')
    h, w = mask.shape
    s = (mask != 0) != bool(invert)
    cap = d + 1
    g = np.full((h, w), cap, dtype=np.int64)
    run = np.full(w, cap, dtype=np.int64)
    for y in range(h):
        run = np.where(s[y], 0, np.minimum(run + 1, cap))
        g[y] = run
    run = np.full(w, cap, dtype=np.int64)
    for y in range(h - 1, -1, -1):
        run = np.where(s[y], 0, np.minimum(run + 1, cap))
        g[y] = np.minimum(g[y], run)
    near = np.zeros((h, w), dtype=bool)
    g2, d2 = g * g, d * d
    for dx in range(-min(d, w - 1), min(d, w - 1) + 1):
        # pixel x looks at x' = x + dx
        if dx >= 0:
            near[:, :w - dx] |= dx * dx + g2[:, dx:] <= d2
        else:
            near[:, -dx:] |= dx * dx + g2[:, :w + dx] <= d2
    return (~near).astype(np.uint8)


def adapt_labels(logits, last_mask, pos_logit, neg_distance, erode=0):
    """(label float32 [H,W], void uint8 [H,W], counts int64 [3] = {positives, negatives, void}) of one frame.

    ``core = far_from(last_mask, erode, invert=True)`` (the mask eroded) if ``erode > 0``, else ``last_mask != 0``.
    ``far = far_from(core, neg_distance)`` if the core has a set pixel, else all 0: an empty core names no negatives (as an
    empty seed gates nothing in util/mask_components.py) - otherwise one empty mask would teach the net that nothing is the
    object.  A far pixel is a negative (label 0, void 0) whatever its logit: that is how a distant confident blob becomes a
    hard negative.  Elsewhere ``logits >= float32(pos_logit)`` is a positive (label 1, void 0; a NaN never is, +inf is,
    equality counts).  The rest is void (label 0, void 1)."""
    logits = np.asarray(logits)
    if logits.ndim != 2 or logits.dtype != np.float32:
        raise ValueError('adapt_labels: logits must be a float32 [H,W] array, got {} {}'.format(logits.dtype, logits.shape))
    last_mask = _check_mask(last_mask, 'adapt_labels')
    if last_mask.shape != logits.shape:
        raise ValueError('adapt_labels: last_mask is {}, the logits are {}'.format(last_mask.shape, logits.shape))
    neg_distance = _check_distance(neg_distance, 'adapt_labels', 'neg_distance')
    erode = _check_distance(erode, 'adapt_labels', 'erode')
    threshold = np.float32(pos_logit)
    if np.isnan(threshold):
        raise ValueError('adapt_labels: pos_logit is NaN')
    core = far_from(last_mask, erode, invert=True) if erode > 0 else (last_mask != 0).astype(np.uint8)
    far = far_from(core, neg_distance).astype(bool) if core.any() else np.zeros(core.shape, dtype=bool)
    with np.errstate(invalid='ignore'):
        pos = ~far & (logits >= threshold)
    void = ~far & ~pos
    counts = np.array([int(pos.sum()), int(far.sum()), int(void.sum())], dtype=np.int64)
    return pos.astype(np.float32), void.astype(np.uint8), counts


def _pixel_terms(x):
    """The per-pixel terms of the class-balanced loss in float64: l(x, y) = max(x, 0) - x y + log(1 + exp(-|x|)) split
    into its y = 1 and y = 0 values, and sigmoid(x)."""
    soft = np.log1p(np.exp(-np.abs(x)))
    relu = np.maximum(x, 0.0)
    e = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return relu - x + soft, relu + soft, sig


def cbce_void(logits, label, void, size_average=True):
    """(loss, gradient) in float64 of the class-balanced cross entropy over the valid pixels: ``valid = void == 0``,
    ``y = label >= 0.5``, n_pos and n_neg counted over valid pixels only, n_tot = n_pos + n_neg,
    ``loss = n_neg / n_tot * sum_{valid, y} l + n_pos / n_tot * sum_{valid, not y} l`` (divided by n_tot under
    ``size_average``), gradient ``n_neg / n_tot * (sigmoid - 1)`` on valid positives, ``n_pos / n_tot * sigmoid`` on valid
    negatives and exactly +0.0 on void pixels, whose logits (a NaN too) are never looked at.  ``n_tot == 0``: loss 0,
    gradient 0.  With ``void`` all zero this is the reference's loss (src/layers/osvos_layers.py:17-44).

    This is deliberately NOT upstream OSVOS-PyTorch's ``void_pixels`` variant: that one masks the void pixels out of the two
    sums but still counts them among the negatives when it balances the classes."""
    x = np.asarray(logits, dtype=np.float64)
    valid = np.asarray(void) == 0
    y = np.asarray(label) >= 0.5
    if not x.shape == valid.shape == y.shape:
        raise ValueError('cbce_void: logits {}, label {} and void {} differ in shape'.format(x.shape, y.shape, valid.shape))
    pos, neg = valid & y, valid & ~y
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    n_tot = n_pos + n_neg
    grad = np.zeros(x.shape, dtype=np.float64)
    if n_tot == 0:
        return 0.0, grad
    xs = np.where(valid, x, 0.0)  # a void pixel's logit is replaced before anything is computed from it
    l_pos, l_neg, sig = _pixel_terms(xs)
    w_pos, w_neg = n_neg / n_tot, n_pos / n_tot
    loss = w_pos * l_pos[pos].sum() + w_neg * l_neg[neg].sum()
    grad[pos] = w_pos * (sig[pos] - 1.0)
    grad[neg] = w_neg * sig[neg]
    if size_average:
        loss /= n_tot
        grad /= n_tot
    return float(loss), grad


def cbce_void_torch(output, label, void=None, size_average=True):
    """``cbce_void`` as a torch expression that autograd differentiates (the CPU stand-in nets of the tests; the product
    path is the HIP kernel).  ``void`` None: no pixel is ignored."""
    import torch
    y = label >= 0.5
    valid = torch.ones_like(y) if void is None else (void == 0)
    pos, neg = valid & y, valid & ~y
    n_pos, n_neg = pos.sum().to(output.dtype), neg.sum().to(output.dtype)
    n_tot = n_pos + n_neg
    if float(n_tot) == 0:
        return (output * 0).sum()
    x = torch.where(valid, output, torch.zeros_like(output))
    soft = torch.log1p(torch.exp(-x.abs()))
    relu = torch.clamp(x, min=0)
    zero = torch.zeros_like(x)
    loss = n_neg / n_tot * torch.where(pos, relu - x + soft, zero).sum() \
        + n_pos / n_tot * torch.where(neg, relu + soft, zero).sum()
    return loss / n_tot if size_average else loss
