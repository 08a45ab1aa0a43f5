"""Shapes, windows and bands shared by tests/test_frame_roi_cpu.py and tests/test_gpu_frame_roi.py (not a test module).  The
frames and logits come from the generators of tests/frame_overlay_cases.py."""
import numpy as np

from frame_overlay_cases import ALPHAS, BAND, BAND_SHARE, COLORS, SOFT_ALPHAS, frames, logits  # noqa: F401

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# ((N, Hf, Wf, Hn, Wn), windows [N][4] = (y0, x0, Hw, Ww)): the smallest shapes at which each mechanism can break
CASES = [
    ((1, 5, 7, 2, 3), [(1, 2, 3, 4)]),                             # scalar paths only
    ((1, 5, 7, 2, 3), [(0, 0, 5, 7)]),
    ((2, 33, 47, 16, 20), [(3, 5, 21, 31), (3, 5, 15, 31)]),       # a window a frame: valid and ragged; Hw < Hn = whole frame
    ((2, 33, 47, 16, 20), [(INT32_MIN, 0, 20, 30), (9, 14, 17, 23)]),
    ((1, 61, 107, 27, 48), [(0, 0, 30, 50)]),                      # flush to each of the four corners
    ((1, 61, 107, 27, 48), [(0, 57, 30, 50)]),
    ((1, 61, 107, 27, 48), [(31, 0, 30, 50)]),
    ((1, 61, 107, 27, 48), [(31, 57, 30, 50)]),
    ((1, 64, 128, 32, 64), [(32, 64, 32, 64)]),                    # the net's own size: 1:1, every weight trivial
    ((1, 33, 47, 33, 46), [(0, 0, 33, 47)]),                       # a ratio just above 1
    ((1, 6, 2100, 3, 5), [(0, 0, 6, 2100)]),                       # wider than one staged chunk of 1024 source pixels ...
    ((1, 6, 2100, 3, 5), [(0, 37, 6, 2050)]),                      # ... from a non-zero origin
    ((1, 40, 64, 1, 1), [(0, 0, 40, 64)]),                         # one output pixel
    ((1, 40, 64, 1, 1), [(7, 9, 30, 41)]),
    ((1, 19, 45, 7, 22), [(2, 1, 15, 40)]),                        # Wn no multiple of 4
]
IDS = ["%dx%dx%d_to_%dx%d_w%d" % (c + (k,)) for k, (c, _) in enumerate(CASES)]

# windows that are not valid for frames of 33 x 47 and a net of 16 x 20: each is read as (0, 0, 33, 47)
INVALID_33_47_16_20 = [
    (-1, 0, 20, 30), (0, -1, 20, 30),                  # a negative origin
    (0, 0, 15, 30), (0, 0, 20, 19), (0, 0, 0, 0),      # smaller than the net
    (14, 0, 20, 30), (0, 18, 20, 30),                  # y0 + Hw > Hf, x0 + Ww > Wf
    (0, 0, 34, 30), (0, 0, 20, 48),                    # larger than the frame
    (INT32_MIN, 0, 20, 30), (0, INT32_MIN, 20, 30), (0, 0, INT32_MIN, 30), (0, 0, 20, INT32_MIN),
    (INT32_MAX, 0, 20, 30), (0, INT32_MAX, 20, 30), (0, 0, INT32_MAX, 30), (0, 0, 20, INT32_MAX),
    (INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX), (INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN),
    (1, 1, INT32_MAX, INT32_MAX), (INT32_MAX, 1, 33, 47),
]


def windows_array(windows) -> np.ndarray:
    return np.ascontiguousarray(np.array(windows, dtype=np.int64).astype(np.int32))


def soft_band_window(img, lg, window, mirror, overlay, color, alpha):
    """bool [Hf,Wf]: ``frame_overlay_cases.soft_band`` with the logits painted into a window - the pixels of one frame where an
    ulp of exp() may decide the soft byte.  Outside the window the prediction is an exact 0.0 and nothing can differ."""
    from util import frame_overlay as F
    from util import frame_roi as W
    hf, wf = img.shape[:2]
    p = W.prediction_window(lg, window, hf, wf, False)
    _, inside = W.logits_up_window(lg, window, hf, wf)
    if overlay:
        c = F.COLOR_CHANNEL[color]
        v = F.mirrored(img, mirror)[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
        return inside & (np.abs(v - np.rint(v)) <= BAND) & (v < 255.0 + BAND)
    v = 255 * p + 0.5
    return inside & (np.abs(v - np.rint(v)) <= BAND)


# ------------------------------------------------------------------------------------------ next_window
def blob(hn, wn, rows, cols, value=1.0):
    """float32 [Hn,Wn]: negative everywhere but on rows x cols (inclusive ranges)."""
    x = np.full((hn, wn), -1.0, dtype=np.float32)
    x[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1] = value
    return x


# a drifting rectangle for the end-to-end tests: channel 2 (red) is 250 on the object and 10 elsewhere; the stand-in net
# thresholds that channel.  The object moves by (dy, dx) a frame
def drifting_frames(count, hf, wf, top=20, left=30, h=22, w=34, dy=1, dx=3, seed=0, distractor=None):
    """``distractor`` = (y, x, h, w): a second, smaller object that stands still."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        f = rng.integers(0, 60, (hf, wf, 3), dtype=np.uint8)
        y, x = top + dy * k, left + dx * k
        f[y:y + h, x:x + w, 2] = 250
        if distractor is not None:
            f[distractor[0]:distractor[0] + distractor[2], distractor[1]:distractor[1] + distractor[3], 2] = 250
        out.append(f)
    return out


RED_THRESHOLD = 150.0


def red_offset() -> float:
    """What the stand-in net subtracts from the (mean-subtracted) red channel: a float32 value, as a Python float."""
    from dataloaders.davis_2016 import MEANVAL
    return float(np.float32(np.float32(RED_THRESHOLD) - np.float32(MEANVAL[2])))


def threshold_net_fn(image):
    """float32 [1,3,Hn,Wn] (mean-subtracted BGR) -> float32 [Hn,Wn]: the red channel less ``red_offset()``, one float32
    subtraction - what the stand-in module of the GPU test computes."""
    return (image[0, 2] - np.float32(red_offset())).astype(np.float32)
