"""The two DAVIS 2016 measures of a segmented sequence, on the host in numpy: region similarity J (mask IoU) and contour
accuracy F (boundary F-measure), and the per-sequence statistics (mean, recall, decay) the benchmark reports.

The reference delegates evaluation to an outside toolkit (src/eval/README.md) and holds no copy of it, and that toolkit is
not available to this project either.  These functions are therefore the project's own statement of the protocol
(Perazzi et al., "A Benchmark Dataset and Evaluation Methodology for Video Object Segmentation", CVPR 2016): toolkit parity
unpinned.  ``jf_counts_numpy`` is written the plain way - boolean arrays, the disk as a loop over its offsets on a
zero-padded array - because it is both the CPU fallback of ``experiment_helper.test_scored`` and the yardstick of the HIP
kernel (fosvos_jf_counts), which packs bits and decomposes the disk into spans: the two share no technique.

Counts of a frame, int64 [6]: inter, union, n_pred_b, n_gt_b, match_pred, match_gt (see ``jf_counts_numpy``).
"""
import math
from typing import Dict, Sequence, Tuple

import numpy as np

COUNT_NAMES = ('inter', 'union', 'n_pred_b', 'n_gt_b', 'match_pred', 'match_gt')
BOUND_TH = 0.008  # the boundary tolerance as a share of the image diagonal


def default_radius(h: int, w: int) -> int:
    """ceil(0.008 * diagonal): 8 at 480x854."""
    return int(math.ceil(BOUND_TH * math.sqrt(h * h + w * w)))


def boundary_map(mask: np.ndarray) -> np.ndarray:
    """bool [H,W]: the pixels whose right, lower or lower-right neighbour differs (the toolkit's seg2bmap at the mask's
    own size).  The last row compares to the right only, the last column downwards only, the corner is never set."""
    s = np.asarray(mask).astype(bool)
    h, w = s.shape
    b = np.zeros((h, w), dtype=bool)
    b[:-1, :-1] = (s[:-1, :-1] != s[:-1, 1:]) | (s[:-1, :-1] != s[1:, :-1]) | (s[:-1, :-1] != s[1:, 1:])
    b[-1, :-1] = s[-1, :-1] != s[-1, 1:]
    b[:-1, -1] = s[:-1, -1] != s[1:, -1]
    return b


def disk_offsets(radius: int):
    """Every (dy, dx) with dy*dy + dx*dx <= radius*radius."""
    r = int(radius)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def disk_half_widths(radius: int):
    """The disk as a union of horizontal spans: for dy = -radius..radius the half-width floor(sqrt(r*r - dy*dy)).  This is
    the decomposition the HIP kernel dilates with; ``dilate`` below does not use it."""
    r = int(radius)
    return [math.isqrt(r * r - dy * dy) for dy in range(-r, r + 1)]


def dilate(m: np.ndarray, radius: int) -> np.ndarray:
    """``m`` dilated by the disk of ``radius``; pixels outside the image count as unset."""
    m = np.asarray(m).astype(bool)
    h, w = m.shape
    r = int(radius)
    padded = np.zeros((h + 2 * r, w + 2 * r), dtype=bool)
    padded[r:r + h, r:r + w] = m
    out = np.zeros((h, w), dtype=bool)
    for dy, dx in disk_offsets(r):
        out |= padded[r + dy:r + dy + h, r + dx:r + dx + w]
    return out


def jf_counts_numpy(pred_mask: np.ndarray, gt_mask: np.ndarray, radius: int) -> np.ndarray:
    """int64 [6] for the predicted mask A and the ground truth B (anything non-zero is object):
    |A and B|, |A or B|, |bmap(A)|, |bmap(B)|, |bmap(A) and dil(bmap(B), radius)|, |bmap(B) and dil(bmap(A), radius)|."""
    a, b = np.asarray(pred_mask).astype(bool), np.asarray(gt_mask).astype(bool)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError('jf_counts_numpy: two [H,W] masks of one size, got {} and {}'.format(a.shape, b.shape))
    if radius < 1:
        raise ValueError('jf_counts_numpy: radius {} < 1'.format(radius))
    ba, bb = boundary_map(a), boundary_map(b)
    return np.array([(a & b).sum(), (a | b).sum(), ba.sum(), bb.sum(), (ba & dilate(bb, radius)).sum(),
                     (bb & dilate(ba, radius)).sum()], dtype=np.int64)


def jf_from_counts(counts) -> Tuple[np.ndarray, np.ndarray]:
    """counts [...,6] -> (J, F), fp64 arrays of the leading shape.  J = inter / union (1 when both masks are empty).
    F = 2PR / (P + R) of the boundary precision P = match_pred / n_pred_b and recall R = match_gt / n_gt_b, with the
    toolkit's conventions for empty boundaries: both empty P = R = 1; only the predicted one P = 1, R = 0; only the
    ground truth's P = 0, R = 1."""
    c = np.asarray(counts, dtype=np.float64)
    if c.shape[-1] != 6:
        raise ValueError('jf_from_counts: [...,6] counts, got {}'.format(c.shape))
    inter, union, npb, ngb, mp, mg = [c[..., k] for k in range(6)]
    j = np.where(union == 0, 1.0, inter / np.where(union == 0, 1.0, union))
    pred_empty, gt_empty = npb == 0, ngb == 0
    p = np.where(pred_empty, 1.0, np.where(gt_empty, 0.0, mp / np.where(pred_empty, 1.0, npb)))
    r = np.where(gt_empty, 1.0, np.where(pred_empty, 0.0, mg / np.where(gt_empty, 1.0, ngb)))
    f = np.where(p + r == 0, 0.0, 2 * p * r / np.where(p + r == 0, 1.0, p + r))
    return j, f


def sequence_statistics(values: Sequence[float]) -> Dict[str, float]:
    """mean / recall / decay over the per-frame values of ONE sequence, first and last frame left out (frame 0 is given,
    the last frame is not scored; fewer than 3 frames: all of them).  recall = share of values > 0.5; decay = mean of the
    first quarter minus mean of the last, quarters cut at ids = round(linspace(1, n, 5) + 1e-10) - 1, quarter i =
    values[ids[i] : ids[i+1] + 1]."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if v.size >= 3:
        v = v[1:-1]
    if v.size == 0:
        return {'mean': float('nan'), 'recall': float('nan'), 'decay': float('nan')}
    n = v.size
    ids = (np.round(np.linspace(1, n, 5) + 1e-10) - 1).astype(np.int64)
    quarters = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return {'mean': float(v.mean()), 'recall': float((v > 0.5).mean()),
            'decay': float(quarters[0].mean() - quarters[3].mean())}
