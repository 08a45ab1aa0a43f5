"""Shapes and bands shared by tests/test_frame_resample_cpu.py and tests/test_gpu_frame_resample.py (not a test module).  The
frames and logits come from the generators of tests/frame_overlay_cases.py."""
import numpy as np

from frame_overlay_cases import ALPHAS, BAND, BAND_SHARE, COLORS, SOFT_ALPHAS, frames, logits  # noqa: F401

# (N, Hf, Wf, Hn, Wn): frames of [Hf,Wf], the net at [Hn,Wn]
CASES = [
    (1, 5, 7, 2, 3),        # tiny; scalar paths only
    (1, 16, 16, 8, 8),      # integer ratio; aligned
    (2, 33, 47, 16, 20),    # ragged fractional; two frames
    (1, 61, 107, 27, 48),   # ragged fractional
    (3, 48, 86, 48, 43),    # height unchanged
    (1, 33, 47, 33, 46),    # ratio just above 1; every window straddles two pixels
    (1, 64, 128, 32, 64),   # all groups full
    (1, 45, 80, 5, 9),      # ratio 9 and 8.9; windows wider than a tile
    (1, 40, 64, 1, 1),      # one output pixel; unbounded window
    (1, 96, 172, 48, 86),   # 2x; the small VGG's size
]
IDS = ["%dx%dx%d_to_%dx%d" % c for c in CASES]


def integer_ratio(case) -> bool:
    _, hf, wf, hn, wn = case
    return hf % hn == 0 and wf % wn == 0


def soft_band_scaled(img, lg, mirror, overlay, color, alpha):
    """bool [Hf,Wf]: ``frame_overlay_cases.soft_band`` with logits of the net's size - the pixels of one frame where an ulp
    of exp() may decide the soft byte."""
    from util import frame_overlay as F
    from util import frame_resample as R
    hf, wf = img.shape[:2]
    p = R.prediction_scaled(lg, hf, wf, False)
    if overlay:
        c = F.COLOR_CHANNEL[color]
        v = F.mirrored(img, mirror)[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
        return (np.abs(v - np.rint(v)) <= BAND) & (v < 255.0 + BAND)
    v = 255 * p + 0.5
    return np.abs(v - np.rint(v)) <= BAND
