"""fosvos_hip/limits.py: every scalar check against a table of accepted and refused values (with the full message), every
range against its twin in the numpy definitions under util/ and against the ``ops`` alias, and the options dataclasses
accepting and refusing exactly at those bounds."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from fosvos_hip import limits, options  # noqa: E402
from util import frame_resample, frame_roi, guided_upsample, mask_components, object_merge, online_adapt  # noqa: E402

NAN, INF = float("nan"), float("inf")


def refused(call, message):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == message


# ------------------------------------------------------------------------------------------------ the scalar checks
def test_check_int():
    for v in (0, 1, 63, 64):
        assert limits.check_int("op", "levels", v, 0, 64) == v
    assert limits.check_int("op", "steps", 10 ** 12, 0) == 10 ** 12
    for v, shown in ((-1, "-1"), (65, "65"), (True, "True"), (False, "False"), (1.0, "1.0"), (np.int64(3), repr(np.int64(3))),
                     (NAN, "nan"), (INF, "inf"), ("3", "'3'"), (None, "None")):
        refused(lambda: limits.check_int("op", "levels", v, 0, 64), f"op: levels must be an integer in 0..64, got {shown}")
    refused(lambda: limits.check_int("op", "steps", -1, 0), "op: steps must be an integer >= 0, got -1")
    refused(lambda: limits.check_int("op", "steps", True, 0), "op: steps must be an integer >= 0, got True")
    refused(lambda: limits.check_int("op", "budget", 0, 1, expect="a positive number of bytes"),
            "op: budget must be a positive number of bytes, got 0")


def test_check_int_integral():
    """``integral``: what ``ops.jpeg_encode`` always took as a quality - any number equal to its int()."""
    for v in (1, 100, 90.0, np.int64(90), np.float32(2.0)):
        got = limits.check_int("op", "quality", v, 1, 100, integral=True)
        assert type(got) is int and got == v
    for v, shown in ((0, "0"), (101, "101"), (True, "True"), (90.5, "90.5"), (np.int64(0), repr(np.int64(0)))):
        refused(lambda: limits.check_int("op", "quality", v, 1, 100, integral=True),
                f"op: quality must be an integer in 1..100, got {shown}")
    with pytest.raises(ValueError):      # int() itself refuses these two, in its own words
        limits.check_int("op", "quality", NAN, 1, 100, integral=True)
    with pytest.raises(OverflowError):
        limits.check_int("op", "quality", INF, 1, 100, integral=True)


def test_check_real_closed_and_open():
    closed = lambda v: limits.check_real("op", "eps", v, 1e-3, 1e9)  # noqa: E731
    for v in (1e-3, 1, 400.0, 1e9, np.float64(2.5)):
        got = closed(v)
        assert type(got) is float and got == v
    below, above = float(np.nextafter(1e-3, 0)), float(np.nextafter(1e9, INF))
    for v, shown in ((below, repr(below)), (above, repr(above)), (True, "True"), (NAN, "nan"), (INF, "inf"), (-INF, "-inf"),
                     (np.int64(5), repr(np.int64(5))), ("1", "'1'"), (None, "None")):
        refused(lambda: closed(v), f"op: eps must be a finite number in [0.001, 1e+09], got {shown}")
    half = lambda v: limits.check_real("op", "clip", v, 0.0, 1e4, lo_open=True)  # noqa: E731
    assert half(5e-324) == 5e-324 and half(1e4) == 1e4 and half(6) == 6.0
    for v, shown in ((0.0, "0.0"), (0, "0"), (float(np.nextafter(1e4, INF)), "10000.000000000002"), (NAN, "nan")):
        refused(lambda: half(v), f"op: clip must be a finite number in (0, 10000], got {shown}")
    both = lambda v: limits.check_real("op", "p", v, 0.5, 1.0, lo_open=True, hi_open=True, expect="a probability in (0.5, 1)")  # noqa: E731
    assert both(0.97) == 0.97 and both(float(np.nextafter(1.0, 0))) < 1
    for v, shown in ((0.5, "0.5"), (1.0, "1.0"), (1, "1"), (False, "False")):
        refused(lambda: both(v), f"op: p must be a probability in (0.5, 1), got {shown}")
    fill = lambda v: limits.check_real("op", "fill", v, *limits.FILL_RANGE, hi_open=True, expect="finite and negative")  # noqa: E731
    assert fill(-100.0) == -100.0 and fill(limits.FILL_RANGE[0]) == limits.FILL_RANGE[0] and fill(-5e-324) < 0
    for v, shown in ((0.0, "0.0"), (-0.0, "-0.0"), (-3.5e38, "-3.5e+38"), (-INF, "-inf"), (NAN, "nan"), (True, "True")):
        refused(lambda: fill(v), f"op: fill must be finite and negative, got {shown}")


def test_check_real_unbounded():
    at_least = lambda v: limits.check_real("op", "alpha", v, 0.0)  # noqa: E731
    assert at_least(0) == 0.0 and at_least(0.0) == 0.0 and at_least(1e300) == 1e300
    for v, shown in ((-5e-324, "-5e-324"), (INF, "inf"), (NAN, "nan"), (True, "True")):
        refused(lambda: at_least(v), f"op: alpha must be a finite number >= 0, got {shown}")
    above = lambda v: limits.check_real("op", "rate", v, 0.0, lo_open=True)  # noqa: E731
    assert above(5e-324) == 5e-324 and above(3) == 3.0
    for v, shown in ((0, "0"), (0.0, "0.0"), (-1e-8, "-1e-08"), (INF, "inf")):
        refused(lambda: above(v), f"op: rate must be a finite number > 0, got {shown}")


def test_check_pair():
    assert limits.check_pair("op", "net_size", (6, 10), "(Hn, Wn)") == (6, 10)
    assert limits.check_pair("op", "net_size", [1, 1], "(Hn, Wn)") == (1, 1)
    for v in (7, None, (1, 2, 3), (1,), "abc"):
        refused(lambda: limits.check_pair("op", "net_size", v, "(Hn, Wn)"), f"op: net_size must be a pair (Hn, Wn), got {v!r}")
    for v in ((0, 4), (4, -1), (True, 4), (4.0, 4), (np.int64(4), 4), (NAN, 4), ("ab")):
        refused(lambda: limits.check_pair("op", "frame_size", v, "(Hf, Wf)"),
                f"op: frame_size must be a pair of positive ints, got {v!r}")


def test_check_member():
    assert limits.check_member("op", "huffman", "fitted", {'fixed': 0, 'fitted': 1}) == "fitted"
    assert limits.check_member("op", "subsampling", "4:2:0", limits.JPEG_SUBSAMPLINGS) == "4:2:0"
    refused(lambda: limits.check_member("op", "huffman", "best", {'fixed': 0, 'fitted': 1}),
            "op: huffman must be one of ('fixed', 'fitted'), got 'best'")
    refused(lambda: limits.check_member("op", "subsampling", 420, limits.JPEG_SUBSAMPLINGS),
            "op: subsampling must be one of ('4:4:4', '4:2:0'), got 420")
    refused(lambda: limits.check_member("op", "color", None, {'b': 0, 'g': 1, 'r': 2}), "op: color must be one of ('b', 'g', 'r'), got None")


def test_real_number():
    for v in (0, -3, 2.5, np.float64(1.0), 10 ** 400):
        assert limits.real_number(v)
    for v in (True, False, NAN, INF, -INF, None, "1", np.int64(1), np.float32(1.0), 1j):
        assert not limits.real_number(v)


# ------------------------------------------------------------------------------------------------ the ranges, pinned
def test_ranges_equal_the_numpy_definitions():
    assert limits.ROI_MAX_LEVELS == frame_roi.MAX_LEVELS
    assert limits.ROI_MAX_PAD == frame_roi.MAX_PAD
    assert round(1000 * limits.ROI_MAX_MARGIN) == frame_roi.MAX_PERMILLE
    assert limits.GATE_MAX_DISTANCE == online_adapt.MAX_DISTANCE
    assert limits.GUIDED_MAX_RADIUS == guided_upsample.MAX_RADIUS
    assert limits.GUIDED_EPS_RANGE == guided_upsample.EPS_RANGE
    assert limits.GUIDED_MAX_CLIP == guided_upsample.MAX_CLIP
    assert limits.MAX_FRAME_SIDE == frame_resample.MAX_SIDE
    assert limits.CLEAN_MAX_RADIUS == mask_components.MAX_RADIUS
    assert limits.MAX_OBJECTS == object_merge.MAX_OBJECTS
    from util import jpeg_layout
    assert limits.JPEG_SUBSAMPLINGS == jpeg_layout.SUBSAMPLINGS
    assert limits.FILL_RANGE == (float(np.finfo(np.float32).min), 0.0)
    assert limits.CLEAN_MAX_AREA == np.iinfo(np.int32).max


def test_ranges_equal_the_ops_aliases():
    from fosvos_hip import ops
    for name in ("ROI_MAX_LEVELS", "ROI_MAX_PAD", "ROI_MAX_MARGIN", "GATE_MAX_DISTANCE", "GATE_MAX_SIDE", "GUIDED_MAX_RADIUS",
                 "GUIDED_EPS_RANGE", "GUIDED_MAX_CLIP", "MAX_FRAME_SIDE", "MAX_OBJECTS", "JPEG_SUBSAMPLINGS"):
        assert getattr(ops, name) is getattr(limits, name), name


def test_limits_imports_neither_torch_nor_numpy():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from fosvos_hip import limits, options; "
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules" % os.path.join(ROOT, "fosvos_amd"))
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


# ------------------------------------------------------------------------------------------------ the options, at the bounds
def accepted_and_refused(cls, field, good, bad, expect):
    for v in good:
        assert getattr(cls(**{field: v}), field) == v
    for v in bad:
        refused(lambda: cls(**{field: v}), f"{cls.__name__}: {field} must be {expect}, got {v!r}")


def test_roi_options_bounds():
    accepted_and_refused(options.RoiOptions, "levels", (1, limits.ROI_MAX_LEVELS), (0, limits.ROI_MAX_LEVELS + 1, True, 8.0),
                         "an integer in 1..64")
    accepted_and_refused(options.RoiOptions, "min_pad", (0, limits.ROI_MAX_PAD), (-1, limits.ROI_MAX_PAD + 1, False, 16.0),
                         "an integer in 0..4095")
    accepted_and_refused(options.RoiOptions, "margin", (0, 0.0, limits.ROI_MAX_MARGIN, 4),
                         (-1e-9, float(np.nextafter(4.0, 5)), True, INF, "0.25"), "a finite number in [0, 4]")
    refused(lambda: options.RoiOptions(margin=NAN), "RoiOptions: margin must be a finite number in [0, 4], got nan")
    assert options.RoiOptions(margin=limits.ROI_MAX_MARGIN).margin_permille == frame_roi.MAX_PERMILLE


def test_refine_options_bounds():
    lo, hi = limits.GUIDED_EPS_RANGE
    accepted_and_refused(options.RefineOptions, "radius", (1, limits.GUIDED_MAX_RADIUS), (0, limits.GUIDED_MAX_RADIUS + 1, True, 4.0),
                         "an integer in 1..8")
    accepted_and_refused(options.RefineOptions, "eps", (lo, hi, 1), (float(np.nextafter(lo, 0)), float(np.nextafter(hi, INF)), True, INF),
                         "a finite number in [0.001, 1e+09]")
    accepted_and_refused(options.RefineOptions, "clip", (5e-324, limits.GUIDED_MAX_CLIP), (0.0, float(np.nextafter(1e4, INF)), False, INF),
                         "a finite number in (0, 10000]")


def test_clean_options_bounds():
    accepted_and_refused(options.CleanOptions, "min_area", (0, limits.CLEAN_MAX_AREA), (-1, limits.CLEAN_MAX_AREA + 1, True, 4.0),
                         "an integer in 0..2147483647")
    accepted_and_refused(options.CleanOptions, "temporal_radius", (None, 0, limits.CLEAN_MAX_RADIUS),
                         (-1, limits.CLEAN_MAX_RADIUS + 1, True, 3.0), "None or an integer in 0..63")
    accepted_and_refused(options.CleanOptions, "fill", (-100.0, -1, limits.FILL_RANGE[0], -5e-324), (0.0, 1.0, -INF, True, -3.5e38),
                         "finite and negative")


def test_adapt_options_bounds():
    accepted_and_refused(options.AdaptOptions, "steps", (0, 1, 1000), (-1, True, 1.0), "an integer >= 0")
    for field in ("neg_distance", "erode"):
        accepted_and_refused(options.AdaptOptions, field, (0, limits.GATE_MAX_DISTANCE), (-1, limits.GATE_MAX_DISTANCE + 1, True, 15.0),
                             "an integer in 0..4095")
    accepted_and_refused(options.AdaptOptions, "pos_prob", (float(np.nextafter(0.5, 1)), float(np.nextafter(1.0, 0))),
                         (0.5, 1.0, 1, True, INF), "a probability in (0.5, 1)")
    accepted_and_refused(options.AdaptOptions, "frame_weight", (5e-324, 1, 1e300), (0, 0.0, -1.0, INF, True), "a finite number > 0")
    accepted_and_refused(options.AdaptOptions, "first_weight", (0, 0.0, 1e300), (-5e-324, INF, False), "a finite number >= 0")
    accepted_and_refused(options.AdaptOptions, "learning_rate", (5e-324, 1e-8), (0.0, -1e-8, INF, True), "a finite number > 0")
