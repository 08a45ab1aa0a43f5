"""Moving the object against its background (dataloaders/lucid.py) without a GPU: the painted-out background, the bilinear
alpha, the composition and its two exact ends, the eleven draws, LucidOptions, the flags and the one-shot loader on a CPU
device.  Every comparison is exact equality of bits (or of integers)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import custom_transforms as T  # noqa: E402
from dataloaders import lucid as L  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016, MEANVAL  # noqa: E402
from fosvos_hip import limits  # noqa: E402
from fosvos_hip.options import LucidOptions, RotateOptions  # noqa: E402
from test_resident_set_cpu import _epochs, write_davis_tree  # noqa: E402

IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
FAR = np.array([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0]])
SHEAR = np.array([[1.0, 0.3, -4.5], [-0.2, 1.1, 3.25]])  # taps fall outside on all four sides (the rotate test's)
ONE, ZERO = np.ones(3, np.float32), np.zeros(3, np.float32)
N_EPOCHS = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def luts(lab):
    """(img_lut [256,3], gt_lut [256]) as the resident loaders build them."""
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = np.ascontiguousarray(ds.convert_raw(ramp, None)[0].reshape(256, 3))
    return img_lut, np.arange(256, dtype=np.float32) / np.float32(max(float(lab.max()), 1e-8))


def sample(h, w, peak=255, kind="blob"):
    """(frame, filled background, mask): random bytes under an object of ``peak``: an ellipse off the centre with a second
    label value in it ("blob"), nothing ("empty"), everything ("full") or a rectangle that touches two borders ("corner")."""
    rng = np.random.RandomState(h * 1000 + w)
    frame = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[:h, :w]
    mask = np.zeros((h, w), np.uint8)
    if kind == "blob":
        inside = ((y - 0.45 * h) / (0.3 * h)) ** 2 + ((x - 0.55 * w) / (0.25 * w)) ** 2 <= 1.0
        mask[inside] = peak
        mask[inside & (x % 3 == 0)] = max(peak // 2, 1)
        mask[int(0.45 * h), int(0.55 * w)] = peak
    elif kind == "full":
        mask[:] = peak
    elif kind == "corner":
        mask[: h // 2, w - w // 3:] = peak
    else:
        assert kind == "empty"
    return frame, L.fill_background(frame, mask, 2, 1), mask


def drawn_pairs(h, w, mask, flip, n=3, seed=11):
    """``n`` (M_bg, M_fg, gain, bias) drawn as the loader draws them, for the (flipped) mask."""
    import random
    dream = LucidOptions().dream()
    rng = random.Random(seed + h * w)
    box = L.mask_box(mask[:, ::-1] if flip else mask)
    return [dream.matrices(dream.draw(rng), box, (h, w)) for _ in range(n)]


# ------------------------------------------------------------------------------------------ fill_background
def hand_case():
    v = (10 * np.arange(5)[:, None] + np.arange(6)[None, :]).astype(np.uint8)
    frame = np.stack([v, 2 * v, np.full_like(v, 100)], axis=2)
    mask = np.zeros((5, 6), np.uint8)
    mask[0:2, 2:4] = 255  # a whole cell of level 1
    mask[4, 5] = 1        # the lone child of a corner cell
    return frame, mask


def test_fill_hand_worked_pyramid():
    frame, mask = hand_case()
    levels = L.push_pyramid(frame, mask == 0)
    assert [n.shape for _, n in levels] == [(5, 6), (3, 3), (2, 2), (1, 1)]
    s = [lv[0][..., 0].tolist() for lv in levels]
    n = [lv[1].tolist() for lv in levels]
    assert s[1] == [[22, 0, 38], [102, 110, 118], [81, 85, 44]] and n[1] == [[4, 0, 4], [4, 4, 4], [2, 2, 1]]
    assert s[2] == [[234, 156], [166, 44]] and n[2] == [[12, 8], [4, 1]]
    assert s[3] == [[600]] and n[3] == [[25]]
    assert np.array_equal(levels[1][0][..., 1], 2 * levels[1][0][..., 0]) and levels[3][0][0, 0, 2] == 2500
    fills = L.pull_pyramid(levels)
    f = [lv[..., 0].tolist() for lv in fills]
    assert f[3] == [[24]]                       # 600 / 25
    assert f[2] == [[20, 20], [42, 44]]         # 19.5, 19.5 and 41.5 round up
    assert f[1] == [[6, 20, 10], [26, 28, 30], [41, 43, 44]]  # the empty cell takes its parent's 20
    want = frame[..., 0].astype(np.int64)
    want[0:2, 2:4], want[4, 5] = 20, 44
    assert f[0] == want.tolist()
    got = L.fill_background(frame, mask, 0, 0)
    assert got.dtype == np.uint8 and np.array_equal(got[..., 0], want)
    assert (got[0:2, 2:4, 1] == 39).all() and got[4, 5, 1] == 88 and (got[..., 2] == 100).all()  # 468 / 12 = 39 exactly
    # one smoothing pass: the corner pixel's 3 x 3 with the border replicated is 34 35 35 / 44 44 44 / 44 44 44
    smooth = L.fill_background(frame, mask, 0, 1)
    assert smooth[4, 5, 0] == (368 + 4) // 9 == 41
    # the 2 x 2 hole, all at 20: (0, 2) sees rows 0, 0, 1 and columns 1..3: 1 20 20 / 1 20 20 / 11 20 20
    assert smooth[0, 2, 0] == (1 + 1 + 11 + 6 * 20 + 4) // 9 == 15
    assert np.array_equal(smooth[mask == 0], frame[mask == 0])


def test_fill_properties():
    frame, _, mask = sample(37, 53)
    for dilate, smooth in ((0, 0), (3, 2), (8, 16)):
        got = L.fill_background(frame, mask, dilate, smooth)
        valid = ~L.dilated_hole(mask, dilate)
        assert valid.any() and not valid.all()
        assert got.shape == frame.shape and got.dtype == np.uint8
        assert np.array_equal(got[valid], frame[valid])                      # valid pixels are untouched
        assert valid.sum() < (mask == 0).sum() or dilate == 0
        # what holds of a second pass: the frame's bytes inside the hole are never read, so with the same mask and options the
        # fill of ANY frame that agrees on the valid pixels is the same array - the output itself included: fully idempotent
        assert np.array_equal(L.fill_background(got, mask, dilate, smooth), got)
        scribbled = frame.copy()
        scribbled[~valid] = 255 - scribbled[~valid]
        assert np.array_equal(L.fill_background(scribbled, mask, dilate, smooth), got)
    # ... and with a smaller margin it is not: the ring between the two holes is now valid and keeps the earlier fill's values
    wide = L.fill_background(frame, mask, 3, 2)
    assert not np.array_equal(L.fill_background(wide, mask, 0, 2), L.fill_background(frame, mask, 0, 2))
    # the dilation is the clipped square
    one = np.zeros((9, 11), np.uint8)
    one[0, 10] = 7
    want = np.zeros((9, 11), bool)
    want[0:3, 8:11] = True
    assert np.array_equal(L.dilated_hole(one, 2), want) and np.array_equal(L.dilated_hole(one, 0), one != 0)
    assert L.dilated_hole(one, 31).all()
    # one colour fills with that colour
    flat = np.empty((37, 53, 3), np.uint8)
    flat[:] = (9, 200, 77)
    assert np.array_equal(L.fill_background(flat, mask, 4, 3), flat)
    # an empty mask and a full mask (and a hole that grows over everything) return the frame
    for m in (np.zeros_like(mask), np.full_like(mask, 3)):
        got = L.fill_background(frame, m, 5, 2)
        assert np.array_equal(got, frame) and got is not frame
    assert np.array_equal(L.fill_background(frame[:9, :11], one, 31, 2), frame[:9, :11])
    for bad in (dict(dilate=-1), dict(dilate=32), dict(smooth=17), dict(smooth=1.0), dict(dilate=True)):
        with pytest.raises(ValueError, match="fill_background"):
            L.fill_background(frame, mask, **{"dilate": 1, "smooth": 1, **bad})
    with pytest.raises(ValueError, match="fill_background"):
        L.fill_background(frame, mask[:, :-1], 1, 1)
    with pytest.raises(ValueError, match="fill_background"):
        L.fill_background(frame.astype(np.float32), mask, 1, 1)


# ------------------------------------------------------------------------------------------ warp_affine_bilinear
def test_bilinear_identity_and_ramp():
    rng = np.random.RandomState(3)
    arr = rng.randn(19, 23).astype(np.float32)
    assert np.array_equal(bits(L.warp_affine_bilinear(arr, IDENTITY)), bits(arr + np.float32(0.0)))
    # a ramp of small integers over quarter-pixel shifts: every product and sum is exact, so is the interpolation
    y, x = np.mgrid[:19, :23]
    ramp = (3 * x + 5 * y).astype(np.float32)
    m = np.array([[1.0, 0.0, 0.25], [0.0, 1.0, 0.5]])
    got = L.warp_affine_bilinear(ramp, m)
    want = (3 * (x - 0.25) + 5 * (y - 0.5)).astype(np.float32)
    assert np.array_equal(bits(got[1:, 1:]), bits(want[1:, 1:]))       # the four taps lie inside the frame
    assert (got[0, 1:] == ramp[0, 1:] * np.float32(0.5) - np.float32(0.375)).all()  # the row above is outside: val = 0
    # n counts the taps inside the frame and on the object
    obj = np.zeros((19, 23), bool)
    obj[4:9, 6:12] = True
    alpha, n = L.warp_affine_bilinear(obj.astype(np.float32), m, object=obj)
    assert n.max() == 4 and n.min() == 0 and (n[5:9, 7:12] == 4).all() and n[4, 6] == 1 and n[4, 8] == 2
    assert np.array_equal(bits(alpha), bits(L.warp_affine_bilinear(obj.astype(np.float32), m)))
    assert alpha[4, 6] == np.float32(0.5) * np.float32(0.75) and not alpha[n == 0].any()
    with pytest.raises(ValueError, match="warp_affine_bilinear"):
        L.warp_affine_bilinear(arr.astype(np.float64), IDENTITY)


# ------------------------------------------------------------------------------------------ compose
def test_compose_identity_far_and_the_two_ends():
    h, w = 33, 47
    frame, background, mask = sample(h, w)
    img_lut, gt_lut = luts(mask)
    chans = np.arange(3)[None, None, :]
    for flip in (False, True):
        cols = np.arange(w)[::-1] if flip else np.arange(w)
        # identity / identity at gain 1 and bias 0: the frame (in value: -0.0 * 1 + 0 is +0.0) wherever the background is the
        # frame, i.e. with dilate 0 everywhere, and the gt
        for bg in (frame, L.fill_background(frame, mask, 0, 2)):
            image, gt = L.compose(frame, bg, mask, img_lut, gt_lut, flip, IDENTITY, IDENTITY, ONE, ZERO)
            assert image.dtype == np.float32 and image.shape == (h, w, 3) and gt.shape == (h, w)
            assert np.array_equal(image, img_lut[frame[:, cols], chans]) and np.array_equal(bits(gt), bits(gt_lut[mask[:, cols]]))
        # the object far outside (or absent): the warped background alone, and no gt
        for m_bg in (IDENTITY, SHEAR):
            want = T.warp_affine(img_lut[background[:, cols], chans], m_bg) * ONE + ZERO
            for m_fg in (FAR, None):
                image, gt = L.compose(frame, background, mask, img_lut, gt_lut, flip, m_bg, m_fg, ONE, ZERO)
                assert np.array_equal(bits(image), bits(want)) and not gt.any()
        # a moved object: alpha's two ends are exact, interior pixels are the warped frame bit for bit, the rest blends
        m_bg, m_fg, gain, bias = drawn_pairs(h, w, mask, flip, n=1)[0]
        fmask = mask[:, cols]
        alpha, n = L.warp_affine_bilinear((fmask != 0).astype(np.float32), m_fg, object=fmask != 0)
        pinned = L.object_alpha(fmask, m_fg)
        assert (pinned[n == 4] == 1).all() and (pinned[n == 0] == 0).all() and (n == 4).sum() > 50 and (n == 0).sum() > 50
        between = (n > 0) & (n < 4)
        assert between.any() and np.array_equal(bits(pinned[between]), bits(alpha[between]))
        B = T.warp_affine(img_lut[background[:, cols], chans], m_bg)
        Fg = T.warp_affine(img_lut[frame[:, cols], chans], m_fg)
        image, gt = L.compose(frame, background, mask, img_lut, gt_lut, flip, m_bg, m_fg, gain, bias)
        assert np.array_equal(bits(image[pinned == 1]), bits(Fg[pinned == 1] * gain + bias))
        assert np.array_equal(bits(image[pinned == 0]), bits(B[pinned == 0] * gain + bias))
        mid = (pinned > 0) & (pinned < 1)
        a = pinned[mid][:, None]
        assert mid.any() and np.array_equal(bits(image[mid]), bits((B[mid] + a * (Fg[mid] - B[mid])) * gain + bias))
        assert np.array_equal(bits(gt), bits(T.warp_affine(gt_lut[fmask], m_fg)))
        # at gain 1 and bias 0 the interior is the warped frame itself (in value)
        plain, _ = L.compose(frame, background, mask, img_lut, gt_lut, flip, m_bg, m_fg, ONE, ZERO)
        assert np.array_equal(plain[n == 4], Fg[n == 4])
    with pytest.raises(ValueError, match="compose"):
        L.compose(frame, background[:-1], mask, img_lut, gt_lut, False, IDENTITY, IDENTITY, ONE, ZERO)
    with pytest.raises(ValueError, match="compose"):
        L.compose(frame, background, mask, img_lut, gt_lut, False, IDENTITY, IDENTITY, ONE[:2], ZERO)


def test_the_sum_of_the_four_weights_is_not_always_one():
    """Why n == 4 is pinned to exactly 1: in fp32 the four products need not add up to 1."""
    full = np.ones((40, 40), np.float32)
    m = T.rotation_matrix((20, 20), 12.34, 0.9)
    alpha, n = L.warp_affine_bilinear(full, m, object=full != 0)
    assert (alpha[n == 4] != 1).any() and (L.object_alpha(full.astype(np.uint8), m)[n == 4] == 1).all()


# ------------------------------------------------------------------------------------------ the draws
def test_draw_takes_eleven_randoms_in_order():
    class Rng:
        def __init__(self):
            self.calls = 0

        def random(self):
            self.calls += 1
            return self.calls / 16.0

        def randint(self, a, b):
            raise AssertionError("draw takes random() only")

    opts = LucidOptions()
    r = Rng()
    d = opts.dream().draw(r)
    assert r.calls == 11 and d._fields == L.DRAWS == (
        "bg_rot", "bg_zoom", "fg_rot", "fg_zoom", "fg_shift_x", "fg_shift_y", "contrast", "tint_b", "tint_g", "tint_r",
        "brightness")
    ranges = [opts.bg_rots, opts.bg_scales, opts.fg_rots, opts.fg_scales, opts.fg_shift, opts.fg_shift, opts.contrast, opts.tint,
              opts.tint, opts.tint, opts.brightness]
    assert list(d) == [lo + (hi - lo) * ((k + 1) / 16.0) for k, (lo, hi) in enumerate(ranges)]
    # what the draws mean
    m_bg, m_fg, gain, bias = opts.dream().matrices(d, (10, 4, 29, 13), (24, 40))
    assert np.array_equal(m_bg, T.rotation_matrix((20.0, 12.0), d.bg_rot, d.bg_zoom))
    want = T.rotation_matrix((19.5, 8.5), d.fg_rot, d.fg_zoom)
    want[0, 2] += d.fg_shift_x * 20
    want[1, 2] += d.fg_shift_y * 10
    assert np.array_equal(m_fg, want)
    assert gain.dtype == bias.dtype == np.float32
    assert gain.tolist() == [np.float32(d.contrast * t) for t in (d.tint_b, d.tint_g, d.tint_r)]
    assert bias.tolist() == [np.float32(d.brightness)] * 3
    assert opts.dream().matrices(d, None, (24, 40))[1] is None
    # the box and its mirror image
    mask = np.zeros((24, 40), np.uint8)
    mask[4:14, 10:30] = 9
    assert L.mask_box(mask) == (10, 4, 29, 13) and L.mask_box(mask * 0) is None
    assert L.mirrored_box(L.mask_box(mask), 40) == L.mask_box(mask[:, ::-1]) == (10, 4, 29, 13)
    mask[20, 35] = 1
    assert L.mirrored_box(L.mask_box(mask), 40) == L.mask_box(mask[:, ::-1]) == (4, 4, 29, 20)
    assert L.mirrored_box(None, 40) is None


# ------------------------------------------------------------------------------------------ LucidOptions
def test_lucid_options_validation():
    d = LucidOptions()
    assert (d.bg_rots, d.bg_scales, d.fg_rots, d.fg_scales) == ((-10.0, 10.0), (1.0, 1.2), (-15.0, 15.0), (0.85, 1.15))
    assert (d.fg_shift, d.contrast, d.tint, d.brightness, d.dilate, d.smooth) == \
        ((-0.15, 0.15), (0.85, 1.15), (0.95, 1.05), (-15.0, 15.0), 5, 2)
    with pytest.raises(Exception):
        d.dilate = 3  # frozen
    assert (limits.LUCID_MAX_DILATE, limits.LUCID_MAX_SMOOTH) == (L.MAX_DILATE, L.MAX_SMOOTH) == (31, 16)
    good = [dict(bg_rots=(-360, 360)), dict(bg_scales=(1 / 16, 16)), dict(fg_scales=[1, 1]), dict(fg_shift=(-4, 4)),
            dict(contrast=(1 / 16, 16)), dict(tint=(1.0, 1.0)), dict(brightness=(-255, 255)), dict(dilate=0, smooth=0),
            dict(dilate=31, smooth=16)]
    for kw in good:
        o = LucidOptions(**kw)
        assert isinstance(o.dream(), L.LucidDream) and all(type(getattr(o, k)) in (tuple, int) for k in kw)
    assert LucidOptions(fg_scales=[1, 1]) == LucidOptions(fg_scales=(1, 1))
    assert LucidOptions().as_dict()["fg_shift"] == [-0.15, 0.15]
    ranges = ("bg_rots", "bg_scales", "fg_rots", "fg_scales", "fg_shift", "contrast", "tint", "brightness")
    bad = [{name: (2, 1)} for name in ranges] + [{name: (1,)} for name in ranges] + [{name: 1.0} for name in ranges] + \
        [{name: (float("nan"), 1)} for name in ranges] + [{name: (1, float("inf"))} for name in ranges] + \
        [{name: (1, True)} for name in ranges] + \
        [dict(bg_rots=(-361, 0)), dict(fg_rots=(0, 360.5)), dict(bg_scales=(0.05, 1)), dict(fg_scales=(1, 16.5)),
         dict(fg_shift=(-4.5, 0)), dict(contrast=(0, 1)), dict(tint=(1, 17)), dict(brightness=(-256, 0)), dict(bg_rots=None),
         dict(fg_shift=(0, "1")), dict(bg_rots=(1, 2, 3)), dict(dilate=-1), dict(dilate=32), dict(dilate=1.0), dict(dilate=True),
         dict(smooth=-1), dict(smooth=17), dict(smooth=None)]
    for kw in bad:
        with pytest.raises(ValueError, match="^LucidOptions: "):
            LucidOptions(**kw)
    with pytest.raises(ValueError) as e:
        LucidOptions(fg_scales=(0.01, 1))
    assert str(e.value) == "LucidOptions: fg_scales must be a finite number in [0.0625, 16], got 0.01"
    with pytest.raises(ValueError) as e:
        LucidOptions(dilate=40)
    assert str(e.value) == "LucidOptions: dilate must be an integer in 0..31, got 40"


# ------------------------------------------------------------------------------------------ the flags
RANGE_FLAGS = {"--lucid-bg-rotate": "bg_rots", "--lucid-bg-zoom": "bg_scales", "--lucid-fg-rotate": "fg_rots",
               "--lucid-fg-zoom": "fg_scales", "--lucid-fg-shift": "fg_shift", "--lucid-contrast": "contrast",
               "--lucid-tint": "tint", "--lucid-brightness": "brightness"}


def test_flags_parse():
    from util import args_helper
    assert args_helper.parse_args(is_online=True, argv=[]).lucid is None
    assert args_helper.parse_args(is_online=False, argv=[]).lucid is None
    assert args_helper.parse_args(is_online=True, argv=["--augment-lucid"]).lucid == LucidOptions()
    for flag, field in RANGE_FLAGS.items():
        got = args_helper.parse_args(is_online=True, argv=["--augment-lucid", flag, "1", "1.5"]).lucid
        assert got == LucidOptions(**{field: (1.0, 1.5)}), flag
    got = args_helper.parse_args(is_online=True, argv=["--augment-lucid", "--lucid-dilate", "0", "--lucid-smooth", "16",
                                                       "--lucid-fg-shift", "-0.5", "0.25"]).lucid
    assert got == LucidOptions(dilate=0, smooth=16, fg_shift=(-0.5, 0.25))
    for extra in (["--multi-object"], ["--adapt-steps", "1"], ["--score"], ["--fast-test"], ["--fast-test", "--score", "--png-fitted"],
                  ["--fast-test", "--clean-largest"], ["--device-decode"]):
        assert args_helper.parse_args(is_online=True, argv=["--augment-lucid"] + extra).lucid == LucidOptions()
        assert args_helper.parse_args(is_online=True, argv=["--augment-lucid"] + extra).rotate is None


def test_flag_refusals_give_the_reason(capsys):
    from util import args_helper
    cases = [([flag, "1", "1.5"], flag + " set(s) an option of the lucid augmentation: it needs --augment-lucid")
             for flag in RANGE_FLAGS]
    cases += [
        (["--lucid-dilate", "3"], "--lucid-dilate set(s) an option of the lucid augmentation: it needs --augment-lucid"),
        (["--lucid-smooth", "3", "--lucid-tint", "1", "1"], "--lucid-tint / --lucid-smooth set(s)"),
        (["--augment-lucid", "--augment-rotate"], "both stand in place of the rescale"),
        (["--augment-lucid", "--synthetic"], "the loader of --synthetic augments nothing"),
        (["--augment-lucid", "--data-parallel"], "not wired to the sharded loaders of --data-parallel"),
        (["--augment-lucid", "--lucid-fg-zoom", "0.01", "1"], "--lucid-*: fg_scales must be a finite number"),
        (["--augment-lucid", "--lucid-bg-rotate", "10", "-10"], "--lucid-*: bg_rots must be (lo, hi) with lo <= hi"),
        (["--augment-lucid", "--lucid-dilate", "32"], "--lucid-*: dilate must be an integer in 0..31"),
        (["--augment-lucid", "--lucid-smooth", "-1"], "--lucid-*: smooth must be an integer in 0..16"),
        (["--augment-lucid", "--lucid-contrast", "1"], "expected 2 arguments"),
        (["--augment-lucid", "--lucid-dilate", "1.5"], "invalid int value")]
    for argv, reason in cases:
        with pytest.raises(SystemExit):
            args_helper.parse_args(is_online=True, argv=argv)
        assert reason in capsys.readouterr().err, argv
    # the offline command line has no one-shot sample
    for argv in (["--augment-lucid"], ["--augment-lucid", "--resident-train-set"]):
        with pytest.raises(SystemExit):
            args_helper.parse_args(is_online=False, argv=argv)
        assert "the offline training set would need a filled background per training frame" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        args_helper.parse_args(is_online=False, argv=["--lucid-dilate", "3"])
    assert "it needs --augment-lucid" in capsys.readouterr().err


def test_online_main_passes_the_option(monkeypatch, tmp_path):
    import train_online
    seen = []

    def fake_loader(*args, **kwargs):
        seen.append(("sequence", args[2], kwargs))
        raise KeyboardInterrupt

    class FakeOneShot:
        def __init__(self, dataset, **kwargs):
            seen.append(("object", dataset, kwargs))
            raise KeyboardInterrupt

    monkeypatch.setattr(train_online.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_online, "rotate", None)
    monkeypatch.setattr(train_online, "lucid", None)
    monkeypatch.setattr(train_online, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_online, "save_dir_results", tmp_path / "results")
    monkeypatch.setattr(train_online.io_helper, "get_data_loader_train", fake_loader)
    monkeypatch.setattr(train_online.io_helper, "write_settings", lambda *a, **k: None)
    monkeypatch.setattr(train_online.provider_mapping[("online", "vgg16")], "load_network_train", lambda self: None)
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["--augment-lucid", "--lucid-dilate", "7", "-s", "bear", "--no-testing"])
    assert seen[-1] == ("sequence", "bear", {"synthetic": None, "lucid": LucidOptions(dilate=7)})
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["-s", "bear", "--no-testing"])
    assert seen[-1] == ("sequence", "bear", {"synthetic": None}) and train_online.lucid is None  # absent: the call is what it was
    import dataloaders.davis_2017 as D17
    import dataloaders.resident as R
    monkeypatch.setattr(D17, "n_objects", lambda root, seq: 2)
    monkeypatch.setattr(D17, "DAVIS2017", lambda **kw: ("dataset", kw["seq_name"], kw["object_id"]))
    monkeypatch.setattr(R, "ResidentOneShotLoader", FakeOneShot)
    monkeypatch.setattr(train_online, "_get_summary_writer", lambda *a, **k: None)
    with pytest.raises(KeyboardInterrupt):
        train_online.main(["--augment-lucid", "--multi-object", "-s", "bear", "--no-testing"])
    assert seen[-1] == ("object", ("dataset", "bear", 1), {"lucid": LucidOptions()})


# ------------------------------------------------------------------------------------------ the loader on a CPU device
SEQS = {"bear": (2, 24, 40), "camel": (2, 24, 40)}


@pytest.fixture(scope="module")
def davis_root(tmp_path_factory):
    return write_davis_tree(tmp_path_factory.mktemp("davis_lucid"), seqs=SEQS, train=["bear"])


def lucid_epochs(loader, seed, n_epochs=N_EPOCHS):
    torch.manual_seed(seed)
    return _epochs(loader, n_epochs)


def test_cpu_loader(davis_root):
    import train_online
    from dataloaders.resident import ResidentOneShotLoader, ResidentTrainSetLoader
    from util import io_helper
    ds = DAVIS2016(mode="train", db_root_dir=str(davis_root), seq_name="bear")
    opts = LucidOptions()
    loader = ResidentOneShotLoader(ds, device=torch.device("cpu"), lucid=opts)
    assert len(loader) == 1 and loader.lucid is opts and loader.rotate is None
    assert loader.scales == [1] and list(loader.variants) == [(False, 0)]
    a, b = lucid_epochs(loader, 5), lucid_epochs(ResidentOneShotLoader(ds, device=torch.device("cpu"), lucid=opts), 5)
    assert torch.equal(a[1], b[1])  # the default generator is left in the same state
    for xa, xb in zip(a[0], b[0]):
        assert len(xa) == len(xb) == 1 and xa[0]["seq_name"] == ["bear"] and xa[0]["fname"] == xb[0]["fname"]
        assert tuple(xa[0]["image"].shape) == (1, 3, 24, 40) and tuple(xa[0]["gt"].shape) == (1, 1, 24, 40)
        for key in ("image", "gt"):
            assert xa[0][key].dtype == torch.float32 and torch.equal(xa[0][key].view(torch.int32), xb[0][key].view(torch.int32))
    assert len({m[0]["image"].numpy().tobytes() for m in a[0]}) == N_EPOCHS  # every epoch another composition
    assert not torch.equal(lucid_epochs(loader, 6)[0][0][0]["image"], a[0][0][0]["image"])
    # the draws are recorded, and they are what the loader composed from
    assert len(loader.draws) == 2 * N_EPOCHS
    flip, draws = loader.draws[0]
    assert isinstance(flip, bool) and isinstance(draws, L.Draws) and len(draws) == 11
    for (lo, hi), v in zip(opts.dream().ranges, draws):
        assert lo <= v <= hi
    again = loader.composed(flip, draws)
    assert torch.equal(again["image"], a[0][0][0]["image"]) and torch.equal(again["gt"], a[0][0][0]["gt"])
    img, lab = ds.read_raw(0)
    img, lab = np.asarray(img, np.uint8), np.asarray(lab, np.uint8)
    img_lut, gt_lut = luts(lab)
    box = L.mask_box(lab[:, ::-1] if flip else lab)
    want = L.compose(img, L.fill_background(img, lab, opts.dilate, opts.smooth), lab, img_lut, gt_lut, flip,
                     *opts.dream().matrices(draws, box, (24, 40)))
    assert np.array_equal(bits(again["image"][0].permute(1, 2, 0).numpy()), bits(want[0]))
    assert np.array_equal(bits(again["gt"][0, 0].numpy()), bits(want[1])) and want[1].any()
    # the replay: base seed, the flip's random(), the eleven draws, then the sampler's seed
    import random
    torch.manual_seed(5)
    rng = random.Random(int(torch.empty((), dtype=torch.int64).random_().item()))
    assert (rng.random() < 0.5, opts.dream().draw(rng)) == loader.draws[0]
    # the unaugmented frame is what online adaptation trains on
    first = train_online._first_sample(loader)
    plain = train_online._first_sample(ResidentOneShotLoader(ds, device=torch.device("cpu")))
    assert torch.equal(first["image"], plain["image"]) and torch.equal(first["gt"], plain["gt"])
    # the factory, and what is refused
    made = io_helper.get_data_loader_train(str(davis_root), 1, "bear", lucid=opts)
    assert isinstance(made, ResidentOneShotLoader) and made.lucid is opts
    for kw, reason in ((dict(seq_name="bear", rotate=RotateOptions()), "pass one of them"),
                       (dict(seq_name="bear", synthetic=(24, 40)), "synthetic loader augments nothing"),
                       (dict(), "filled background per training frame"),
                       (dict(resident_set=True), "filled background per training frame"),
                       (dict(seq_name="bear", resident=False), "the host DataLoader has none to fill from"),
                       (dict(seq_name="bear", shard=(0, 2)), "the host DataLoader has none to fill from")):
        with pytest.raises(ValueError, match=reason):
            io_helper.get_data_loader_train(str(davis_root), 1, lucid=opts, **kw)
    with pytest.raises(ValueError, match="pass one of them"):
        ResidentOneShotLoader(ds, device=torch.device("cpu"), rotate=RotateOptions(), lucid=opts)
    with pytest.raises(ValueError, match="one-shot sample only"):
        ResidentTrainSetLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root)), device="cpu", lucid=opts)
    # without the option the factory makes what it made
    plain = io_helper.get_data_loader_train(str(davis_root), 1, "bear")
    assert isinstance(plain, ResidentOneShotLoader) and plain.lucid is None and len(plain.variants) == 6


# ------------------------------------------------------------------------------------------ the prototype
def test_prototype_the_object_moves_and_leaves_no_trace():
    """97 x 161: a bright ellipse (bytes >= 200) on a dark texture (bytes <= 120), shifted right by a third of its box with
    everything else at rest.  gt is the ellipse 17 pixels further right.  The measure for the old location: over the vacated
    pixels (on the object before, alpha == 0 now) the image is bit for bit the table value of the FILLED background, whose
    bytes there are all <= 120 - not one value of the object's range is left."""
    h, w = 97, 161
    rng = np.random.RandomState(1)
    y, x = np.mgrid[:h, :w]
    obj = ((y - 48) / 20.0) ** 2 + ((x - 60) / 25.0) ** 2 <= 1.0
    frame = rng.randint(0, 121, size=(h, w, 3)).astype(np.uint8)
    frame[obj] = rng.randint(200, 256, size=(int(obj.sum()), 3)).astype(np.uint8)
    mask = np.where(obj, 255, 0).astype(np.uint8)
    box = L.mask_box(mask)
    assert box == (35, 28, 85, 68)
    opts = LucidOptions()
    background = L.fill_background(frame, mask, opts.dilate, opts.smooth)
    assert background.max() <= 120 and np.array_equal(background[~L.dilated_hole(mask, 5)], frame[~L.dilated_hole(mask, 5)])
    draws = L.Draws(0.0, 1.0, 0.0, 1.0, 1.0 / 3, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0)
    m_bg, m_fg, gain, bias = opts.dream().matrices(draws, box, (h, w))
    assert np.array_equal(m_bg, IDENTITY) and np.array_equal(m_fg, [[1.0, 0.0, 17.0], [0.0, 1.0, 0.0]])
    img_lut, gt_lut = luts(mask)
    image, gt = L.compose(frame, background, mask, img_lut, gt_lut, False, m_bg, m_fg, gain, bias)
    moved = np.zeros_like(obj)
    moved[:, 17:] = obj[:, :-17]
    assert np.array_equal(gt, moved.astype(np.float32))
    chans = np.arange(3)[None, None, :]
    assert np.array_equal(image[moved], img_lut[frame, chans][obj])      # the object's own pixels, 17 further right
    vacated = obj & ~moved
    assert vacated.sum() > 500
    assert np.array_equal(image[vacated], img_lut[background, chans][vacated])
    assert (image[vacated] <= img_lut[120][None, :]).all() and (image[moved] >= img_lut[200][None, :]).all()
