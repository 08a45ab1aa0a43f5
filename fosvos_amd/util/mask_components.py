"""Cleaning a mask by its shape, stated in numpy: the 8-connected components of ``logits >= 0``, the small ones dropped, the
largest kept or only those near what was kept in the frame before.  The reference has no such step; these definitions ARE the
bytes of csrc/components.hip (``ops.component_roots``, ``ops.clean_components``), compared with exact equality.

numpy only: importable anywhere.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from util import davis_measures

MAX_RADIUS = 63
DEFAULT_FILL = -100.0


def logits_mask(logits: np.ndarray) -> np.ndarray:
    """The single-object rule: ``logits >= 0``.  NaN is background, -0.0 is foreground."""
    with np.errstate(invalid='ignore'):
        return np.asarray(logits) >= 0


def component_roots(mask: np.ndarray) -> np.ndarray:
    """int32 [H,W]: -1 on the background, else the smallest raster index ``y * W + x`` of the pixel's 8-connected
    component.  The labelling is unique.  (Union-find over the horizontal runs of the rows, in raster order, so a set's
    representative is its first run and that run's first pixel is the component's smallest index.)"""
    mask = np.asarray(mask).astype(bool)
    if mask.ndim != 2:
        raise ValueError('component_roots: a [H,W] mask, got {}'.format(mask.shape))
    h, w = mask.shape
    padded = np.zeros((h, w + 2), dtype=np.int8)
    padded[:, 1:-1] = mask
    edges = np.diff(padded, axis=1)
    ys, starts = np.nonzero(edges == 1)      # run k covers columns starts[k] .. ends[k] - 1 of row ys[k]
    ends = np.nonzero(edges == -1)[1]
    parent = list(range(len(ys)))

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    row_first = np.searchsorted(ys, np.arange(h + 1))  # the runs of row y are row_first[y] .. row_first[y + 1] - 1
    for y in range(1, h):
        a, a_end = row_first[y - 1], row_first[y]
        for k in range(row_first[y], row_first[y + 1]):
            while a < a_end and ends[a] < starts[k]:  # ends[a] - 1 < starts[k] - 1: wholly left of the run's reach
                a += 1
            j = a
            while j < a_end and starts[j] <= ends[k]:  # starts[j] <= ends[k] - 1 + 1: touches, diagonals included
                ra, rb = find(j), find(k)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
                j += 1
    roots = np.full((h, w), -1, dtype=np.int32)
    if len(ys):
        rep = np.array([find(k) for k in range(len(ys))])
        value = (ys[rep].astype(np.int64) * w + starts[rep]).astype(np.int32)
        lengths = ends - starts
        flat = np.repeat(ys.astype(np.int64) * w + starts, lengths) + \
            (np.arange(lengths.sum()) - np.repeat(np.cumsum(lengths) - lengths, lengths))
        roots.ravel()[flat] = np.repeat(value, lengths)
    return roots


def dilate_disk(seed: np.ndarray, radius: int) -> np.ndarray:
    """``davis_measures.dilate(seed, radius)``, computed as the union over dy of the rows spread left and right by
    floor(sqrt(r*r - dy*dy)): the same set without the disk's ~ 3 r*r shifts."""
    seed = np.asarray(seed).astype(bool)
    h, w = seed.shape
    r = int(radius)
    out = np.zeros((h, w), dtype=bool)
    for dy in range(-r, r + 1):
        half = 0
        while (half + 1) ** 2 <= r * r - dy * dy:
            half += 1
        lo, hi = max(0, -dy), min(h, h - dy)  # the output rows y whose source row y + dy exists
        if lo >= hi:
            continue
        # inclusive prefix sums of the source rows, half + 1 zeros in front and half behind: the sum over the columns
        # x - half .. x + half is csum[x + 2 half + 1] - csum[x]
        csum = np.zeros((hi - lo, w + 2 * half + 1), dtype=np.int32)
        csum[:, half + 1:half + 1 + w] = seed[lo + dy:hi + dy]
        np.cumsum(csum, axis=1, out=csum)
        out[lo:hi] |= (csum[:, 2 * half + 1:] - csum[:, :w]) > 0
    return out


def _check_rules(radius, min_area) -> None:
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= radius <= MAX_RADIUS:
        raise ValueError('radius {!r} outside [0, {}]'.format(radius, MAX_RADIUS))
    if isinstance(min_area, bool) or int(min_area) != min_area or min_area < 0:
        raise ValueError('min_area {!r} must be an integer >= 0'.format(min_area))


def keep_components(mask: np.ndarray, seed: Optional[np.ndarray] = None, radius: int = 0, min_area: int = 0,
                    largest: bool = False) -> np.ndarray:
    """bool [H,W]: the pixels of the components that stay.  A component is eligible when its area is >= ``min_area`` and -
    with the gate on - it has a pixel inside ``davis_measures.dilate(seed, radius)``.  The gate is off when ``seed`` is None
    or has no set pixel (the object was lost in the frame before and is taken up again from nothing).  ``largest`` keeps only
    the eligible component of the largest area, on equal areas the one with the smaller root."""
    _check_rules(radius, min_area)
    mask = np.asarray(mask).astype(bool)
    roots = component_roots(mask)
    h, w = mask.shape
    flat = roots.ravel()
    fg = flat >= 0
    area = np.bincount(flat[fg], minlength=h * w)
    eligible = (area > 0) & (area >= int(min_area))
    if seed is not None:
        seed = np.asarray(seed).astype(bool)
        if seed.shape != mask.shape:
            raise ValueError('keep_components: the seed is {}, the mask {}'.format(seed.shape, mask.shape))
        if seed.any():
            near = dilate_disk(seed, int(radius)).ravel()
            touched = np.zeros(h * w, dtype=bool)
            touched[flat[fg & near]] = True
            eligible &= touched
    if largest and eligible.any():
        best = np.where(eligible, area, -1)
        winner = int(np.argmax(best))  # the first maximum: the smaller root
        eligible = np.zeros_like(eligible)
        eligible[winner] = True
    kept = np.zeros(h * w, dtype=bool)
    kept[fg] = eligible[flat[fg]]
    return kept.reshape(h, w)


def check_fill(fill) -> float:
    """``fill`` must be finite and < 0: the overlay interpolates logits, and a tap of weight 0 on an infinity is a NaN."""
    fill = float(fill)
    if not np.isfinite(fill) or not fill < 0:
        raise ValueError('fill must be finite and negative, got {!r}'.format(fill))
    if abs(fill) > float(np.finfo(np.float32).max):
        raise ValueError('fill must be finite as a float32, got {!r}'.format(fill))
    return fill


def clean_logits(logits: np.ndarray, kept: np.ndarray, fill: float = DEFAULT_FILL) -> np.ndarray:
    """float32 [H,W]: a foreground pixel (``logits >= 0``) that was not kept becomes ``fill``; every other value passes bit
    for bit, NaN payloads and signed zeros included."""
    fill = check_fill(fill)
    logits = np.asarray(logits)
    if logits.dtype != np.float32:
        raise ValueError('clean_logits: float32 logits, got {}'.format(logits.dtype))
    kept = np.asarray(kept).astype(bool)
    if kept.shape != logits.shape:
        raise ValueError('clean_logits: kept is {}, the logits {}'.format(kept.shape, logits.shape))
    out = logits.copy()
    out[logits_mask(logits) & ~kept] = np.float32(fill)
    return out


def clean_sequence(logits: np.ndarray, seed0: Optional[np.ndarray] = None, radius: int = 0, min_area: int = 0,
                   largest: bool = False, chain: bool = True, fill: float = DEFAULT_FILL):
    """logits float32 [N,H,W] -> (cleaned float32 [N,H,W], kept bool [N,H,W]).  ``chain=True``: frame 0 is gated by
    ``seed0`` ([H,W] or None), frame n by the kept mask of frame n - 1 (an empty one gates nothing).  ``chain=False``: frame
    n is gated by ``seed0[n]`` ([N,H,W]), or by nothing."""
    logits = np.asarray(logits)
    if logits.ndim != 3 or logits.dtype != np.float32:
        raise ValueError('clean_sequence: float32 [N,H,W] logits, got {} {}'.format(logits.dtype, logits.shape))
    n = logits.shape[0]
    if seed0 is not None:
        seed0 = np.asarray(seed0)
        want = logits.shape[1:] if chain else logits.shape
        if chain and seed0.shape == (1,) + tuple(want):
            seed0 = seed0[0]
        if seed0.shape != tuple(want):
            raise ValueError('clean_sequence: the seed must be {}, got {}'.format(tuple(want), seed0.shape))
    out = np.empty_like(logits)
    kept = np.zeros(logits.shape, dtype=bool)
    seed = seed0 if chain else None
    for i in range(n):
        if not chain:
            seed = None if seed0 is None else seed0[i]
        kept[i] = keep_components(logits_mask(logits[i]), seed, radius, min_area, largest)
        out[i] = clean_logits(logits[i], kept[i], fill)
        if chain:
            seed = kept[i]
    return out, kept
