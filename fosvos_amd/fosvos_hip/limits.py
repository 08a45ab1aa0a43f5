"""The ranges the kernels take and the scalar checks of the Python face, each stated once.  ``ops``
keeps its public constant names as aliases of the ranges, ``options`` and ``stream`` check against them; the numpy definitions
under util/ keep their own copies (they are what the kernels are tested against and stand alone), and
tests/test_limits_cpu.py pins the two sides equal.

No torch, no numpy and no library load here: importable anywhere.
"""
from __future__ import annotations

from typing import Optional, Tuple

# following the object (util/frame_roi.py: MAX_LEVELS, MAX_PAD, MAX_PERMILLE / 1000)
ROI_MAX_LEVELS = 64
ROI_MAX_PAD = 4095
ROI_MAX_MARGIN = 4.0
# the distance gate and the pseudo-labels (util/online_adapt.MAX_DISTANCE)
GATE_MAX_DISTANCE = 4095
GATE_MAX_SIDE = 8192
# mask cleaning (util/mask_components.MAX_RADIUS); an area is a positive int32
CLEAN_MAX_RADIUS = 63
CLEAN_MAX_AREA = (1 << 31) - 1
FILL_RANGE = (-3.4028234663852886e38, 0.0)  # [lowest finite float32, 0)
# the guided filter (util/guided_upsample.py: MAX_RADIUS, EPS_RANGE, MAX_CLIP)
GUIDED_MAX_RADIUS = 8
GUIDED_EPS_RANGE = (1e-3, 1e9)
GUIDED_MAX_CLIP = 1e4
# a scaled call's frames (util/frame_resample.MAX_SIDE), the nets of a sequence (util/object_merge.MAX_OBJECTS; the joint CRF
# of util/label_crf.py has the same K and one label more)
MAX_FRAME_SIDE = 8192
MAX_OBJECTS = 16
# the boundary tolerance of the F measure, the JPEG encoder
JF_RADIUS = (1, 63)
JPEG_QUALITY = (1, 100)
JPEG_SUBSAMPLINGS = ('4:4:4', '4:2:0')
# rotating and zooming the training sample (dataloaders/custom_transforms.ScaleNRotate): degrees, and the zoom factor
ROTATE_MAX_ANGLE = 360.0
ROTATE_SCALE_RANGE = (1.0 / 16, 16.0)
# the test-time ensemble (util/test_ensemble.py: MAX_VIEWS, SCALE_RANGE); a view's sides are within MAX_FRAME_SIDE
ENSEMBLE_MAX_VIEWS = 8
ENSEMBLE_SCALE_RANGE = (0.25, 4.0)
# the CRF on the frame (util/mask_crf.py: MAX_ITERATIONS, MAX_RADIUS, THETA_*_RANGE, MAX_WEIGHT, MAX_CLIP)
CRF_MAX_ITERATIONS = 10
CRF_MAX_RADIUS = 5
CRF_THETA_POS_RANGE = (0.25, 1e3)
CRF_THETA_RGB_RANGE = (1.0, 1e3)
CRF_THETA_SMOOTH_RANGE = (0.25, 1e3)
CRF_MAX_WEIGHT = 100.0
CRF_MAX_CLIP = 1e4
# block matching (util/block_motion.py: BLOCKS, MAX_SEARCH, MAX_ZERO_BIAS)
MOTION_BLOCKS = (8, 16)
MOTION_MAX_SEARCH = 16
MOTION_MAX_ZERO_BIAS = 255
# moving the object against its background (dataloaders/lucid.py: MAX_DILATE, MAX_SMOOTH); angles and zooms as ROTATE_*, the
# object's shift in box sizes, contrast and tint as factors, brightness in grey levels
LUCID_MAX_DILATE = 31
LUCID_MAX_SMOOTH = 16
LUCID_MAX_SHIFT = 4.0
LUCID_GAIN_RANGE = (1.0 / 16, 16.0)
LUCID_MAX_BRIGHTNESS = 255.0


def real_number(v) -> bool:
    """A finite int or float that is not a bool."""
    return not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float("inf")


def check_int(who: str, name: str, v, lo: int, hi: Optional[int] = None, expect: Optional[str] = None,
              integral: bool = False) -> int:
    """``v`` as an int in ``lo..hi`` (``hi=None``: no upper bound), a bool refused; ``integral`` also takes any number equal
    to its ``int()`` (90.0, a numpy integer).  ``expect`` words the rule where the default does not say it."""
    if isinstance(v, bool) or (int(v) != v if integral else not isinstance(v, int)) or v < lo or (hi is not None and v > hi):
        if expect is None:
            expect = f"an integer >= {lo}" if hi is None else f"an integer in {lo}..{hi}"
        raise ValueError(f"{who}: {name} must be {expect}, got {v!r}")
    return int(v)


def check_real(who: str, name: str, v, lo: float, hi: Optional[float] = None, lo_open: bool = False, hi_open: bool = False,
               expect: Optional[str] = None) -> float:
    """``v`` as a float: a finite number in the range from ``lo`` to ``hi`` (``hi=None``: no upper bound), either end open
    or closed."""
    if not real_number(v) or not (v > lo if lo_open else v >= lo) or not (hi is None or (v < hi if hi_open else v <= hi)):
        if expect is None:
            expect = f"a finite number {'>' if lo_open else '>='} {lo:g}" if hi is None else \
                f"a finite number in {'(' if lo_open else '['}{lo:g}, {hi:g}{')' if hi_open else ']'}"
        raise ValueError(f"{who}: {name} must be {expect}, got {v!r}")
    return float(v)


def check_pair(who: str, name: str, v, of: str) -> Tuple[int, int]:
    """``v`` as a pair of positive ints; ``of`` names the two, e.g. '(Hn, Wn)'."""
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a pair {of}, got {v!r}") from None
    for x in (a, b):
        if isinstance(x, bool) or not isinstance(x, int) or x <= 0:
            raise ValueError(f"{who}: {name} must be a pair of positive ints, got {v!r}")
    return a, b


def check_member(who: str, name: str, v, allowed):
    """``v`` where it is one of ``allowed`` (a tuple, or the keys of a dict)."""
    if v not in allowed:
        raise ValueError(f"{who}: {name} must be one of {tuple(allowed)}, got {v!r}")
    return v
