"""Several objects a sequence (DAVIS 2017 style), stated in plain numpy: one net per object is fine-tuned on "this object
against everything else", all K nets run on every frame, and each pixel goes to the object whose net answers highest, or to
the background when no net claims it.  The functions here are the byte-for-byte references of the HIP kernels
(fosvos_merge_objects, fosvos_jf_counts_labels) and the host path of ``experiment_helper.test_objects``, as
util/davis_measures.py, util/png_layout.py and util/frame_overlay.py are for theirs.

Label maps are uint8 [H,W]: 0 = background, k = object k (1 <= k <= K <= 16).  J and F are taken per object, on the masks
``labels == k``; a run's mean is over objects.  Like the single-object measures this is the project's own statement of the
protocol: toolkit parity unpinned.
"""
from typing import Sequence

import numpy as np

from util import davis_measures

MAX_OBJECTS = 16


def merge_labels(logits) -> np.ndarray:
    """logits float32 [K,N,H,W] (or K arrays [N,H,W]) -> uint8 [N,H,W].  Per pixel: object k is VALID where its logit is
    >= 0 (the mask rule of the single-object pass: a NaN is never valid, -0.0 is).  No valid object: label 0.  Otherwise
    1 + k*, k* the lowest k among the valid ones that hold the largest logit (so equal logits, +inf twice included, go to
    the lowest id).  For K = 1 this is the mask ``logits >= 0``."""
    x = np.stack([np.asarray(m, dtype=np.float32) for m in logits]) if not isinstance(logits, np.ndarray) \
        else np.asarray(logits, dtype=np.float32)
    if x.ndim != 4 or not 1 <= x.shape[0] <= MAX_OBJECTS:
        raise ValueError('merge_labels: logits [K,N,H,W] with 1 <= K <= {}, got {}'.format(MAX_OBJECTS, x.shape))
    valid = x >= 0                                       # (False for NaN)
    masked = np.where(valid, x, -np.inf).astype(np.float32)
    best = np.argmax(masked, axis=0)                     # the first of equal maxima: the lowest k
    return np.where(valid.any(axis=0), best + 1, 0).astype(np.uint8)


def jf_counts_labels_numpy(pred_labels: np.ndarray, gt_labels: np.ndarray, n_objects: int, radius: int) -> np.ndarray:
    """int64 [n_objects, 6]: row k - 1 is ``davis_measures.jf_counts_numpy(pred == k, gt == k, radius)``.  Label values above
    ``n_objects`` belong to no object."""
    pred, gt = np.asarray(pred_labels), np.asarray(gt_labels)
    if pred.ndim != 2 or pred.shape != gt.shape:
        raise ValueError('jf_counts_labels_numpy: two [H,W] label maps of one size, got {} and {}'.format(pred.shape, gt.shape))
    if not 1 <= n_objects <= MAX_OBJECTS:
        raise ValueError('jf_counts_labels_numpy: n_objects {} outside [1, {}]'.format(n_objects, MAX_OBJECTS))
    return np.stack([davis_measures.jf_counts_numpy(pred == k, gt == k, radius) for k in range(1, n_objects + 1)])


def davis_palette() -> np.ndarray:
    """uint8 [256,3]: the PASCAL-VOC colour map the DAVIS 2017 annotation files carry, by the bit-interleaving rule: bit j of
    the index (j = 0, 1, 2 -> R, G, B; then the next three bits, and so on) lands at bit 7, 6, ... of its channel.  Entries
    0..3: (0,0,0), (128,0,0), (0,128,0), (128,128,0)."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        c = i
        for shift in range(7, -1, -1):
            for ch in range(3):
                pal[i, ch] |= ((c >> ch) & 1) << shift
            c >>= 3
    return pal


def object_score(counts: np.ndarray, keep: np.ndarray, object_id: int) -> dict:
    """One object's entry of the score dict: counts int64 [n_frames, 6], ``keep`` bool [n_frames] (the scored frames)."""
    j, f = davis_measures.jf_from_counts(counts) if len(counts) else (np.zeros(0), np.zeros(0))
    return {'object_id': int(object_id),
            'counts': [[int(v) for v in row] if k else None for row, k in zip(counts, keep)],
            'J': [float(v) if k else None for v, k in zip(j, keep)],
            'F': [float(v) if k else None for v, k in zip(f, keep)],
            'J_stats': davis_measures.sequence_statistics(j[keep]),
            'F_stats': davis_measures.sequence_statistics(f[keep])}


def mean_statistics(stats: Sequence[dict]) -> dict:
    """Every statistic (mean, recall, decay) averaged over the objects."""
    return {name: float(np.mean([s[name] for s in stats])) for name in ('mean', 'recall', 'decay')}
