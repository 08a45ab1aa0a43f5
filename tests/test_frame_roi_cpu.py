"""Following the object as util/frame_roi.py states it: windows against the whole-frame and the unscaled definitions, the
sanitising rule, the ladder, next_window and its edge cases, the tracking loop, RoiOptions and the options of run_webcam.
No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_resample_cases as RC  # noqa: E402
import frame_roi_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402
from util import frame_roi as W  # noqa: E402


# ------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize("case", RC.CASES, ids=RC.IDS)
def test_whole_frame_window_is_the_scaled_definition(case):
    n, hf, wf, hn, wn = case
    f, x = C.frames(n, hf, wf), C.logits(n, hn, wn)
    whole = (0, 0, hf, wf)
    for k in range(n):
        for mirror in (False, True):
            assert W.prepare_frame_window(f[k], whole, hn, wn, mirror).tobytes() == \
                R.prepare_frame_scaled(f[k], hn, wn, mirror).tobytes()
            for boolean in (True, False):
                for color, alpha in (("r", 1.0), ("g", 0.5), ("b", 2.0)):
                    assert np.array_equal(W.overlay_window(f[k], x[k, 0], whole, mirror, boolean, color, alpha),
                                          R.overlay_scaled(f[k], x[k, 0], mirror, boolean, color, alpha))
        for boolean in (True, False):
            assert np.array_equal(W.mask_bytes_window(x[k, 0], whole, hf, wf, boolean), R.mask_bytes_scaled(x[k, 0], hf, wf, boolean))
            assert np.array_equal(W.apply_window(f[k], x[k, 0], whole, overlay_on=False, boolean_mask=boolean),
                                  R.apply_scaled(f[k], x[k, 0], overlay_on=False, boolean_mask=boolean))
        v, inside = W.logits_up_window(x[k, 0], whole, hf, wf)
        assert inside.all() and v.tobytes() == R.logits_up(x[k, 0], hf, wf).tobytes()


@pytest.mark.parametrize("hf,wf,hn,wn,y0,x0", [(33, 47, 16, 20, 3, 5), (33, 47, 16, 20, 17, 27), (64, 128, 32, 64, 32, 64),
                                               (9, 11, 9, 11, 0, 0)])
def test_net_sized_window_is_the_unscaled_definition_of_the_crop(hf, wf, hn, wn, y0, x0):
    f, x = C.frames(1, hf, wf)[0], C.logits(1, hn, wn)[0, 0]
    window = (y0, x0, hn, wn)
    for mirror in (False, True):
        seen = F.mirrored(f, mirror)
        crop = np.ascontiguousarray(seen[y0:y0 + hn, x0:x0 + wn])
        assert W.prepare_frame_window(f, window, hn, wn, mirror).tobytes() == F.prepare_frame(crop).tobytes()
        for boolean in (True, False):
            got = W.overlay_window(f, x, window, mirror, boolean, "g", 0.5)
            want = np.array(seen, copy=True)
            want[y0:y0 + hn, x0:x0 + wn] = F.overlay(crop, x, False, boolean, "g", 0.5)
            assert np.array_equal(got, want)  # the crop's overlay inside, the frame untouched elsewhere
            mask = W.mask_bytes_window(x, window, hf, wf, boolean)
            want = np.zeros((hf, wf), dtype=np.uint8)
            want[y0:y0 + hn, x0:x0 + wn] = F.mask_bytes(x, boolean)
            assert np.array_equal(mask, want)


def test_every_invalid_window_is_the_whole_frame():
    hf, wf, hn, wn = 33, 47, 16, 20
    f, x = C.frames(1, hf, wf)[0], C.logits(1, hn, wn, zeros=False)[0, 0]
    whole = (0, 0, hf, wf)
    prep = W.prepare_frame_window(f, whole, hn, wn, True).tobytes()
    over = W.overlay_window(f, x, whole, True, False, "r", 0.5)
    assert W.sanitize((3, 5, 21, 31), hf, wf, hn, wn) == (3, 5, 21, 31)
    assert W.sanitize((17, 27, 16, 20), hf, wf, hn, wn) == (17, 27, 16, 20) and W.sanitize(whole, hf, wf, hn, wn) == whole
    for bad in C.INVALID_33_47_16_20:
        as_i32 = C.windows_array([bad])[0]
        assert W.sanitize(as_i32, hf, wf, hn, wn) == whole, bad
        assert W.prepare_frame_window(f, as_i32, hn, wn, True).tobytes() == prep, bad
        assert np.array_equal(W.overlay_window(f, x, as_i32, True, False, "r", 0.5), over), bad
        assert W.next_window(x, as_i32, hf, wf) == W.next_window(x, whole, hf, wf), bad
    for not_a_window in ((1, 2, 3), (1.0, 2.0, 3.0, 4.0), (0, 0, 2 ** 31, 5)):
        with pytest.raises(ValueError):
            W.sanitize(not_a_window, hf, wf, hn, wn)


# ------------------------------------------------------------------------------------------ the ladder, next_window
@pytest.mark.parametrize("hf,wf,hn,wn", [(1080, 1920, 480, 854), (33, 47, 16, 20), (96, 172, 48, 86), (40, 64, 1, 1), (9, 9, 9, 9)])
def test_ladder_is_monotone_from_the_net_to_the_frame(hf, wf, hn, wn):
    for levels in (1, 2, 4, 8, 64):
        sizes = W.ladder(hf, wf, hn, wn, levels)
        assert len(sizes) == levels + 1 and sizes[0] == (hn, wn) and sizes[-1] == (hf, wf)
        for (h0, w0), (h1, w1) in zip(sizes, sizes[1:]):
            assert h0 <= h1 and w0 <= w1
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            W.ladder(hf, wf, hn, wn, bad)


def padded_box(x, window, hf, wf, permille, min_pad):
    """Steps 1 to 5 of next_window, written out again: the padded box cut to the frame, or None."""
    hn, wn = x.shape
    y0, x0, hw, ww = window
    obj = x >= 0
    if not obj.any():
        return None
    ii, jj = np.nonzero(obj)
    by0, by1 = y0 + int(ii.min()) * hw // hn, y0 + -(-(int(ii.max()) + 1) * hw // hn)
    bx0, bx1 = x0 + int(jj.min()) * ww // wn, x0 + -(-(int(jj.max()) + 1) * ww // wn)
    pad = min_pad + -(-permille * max(by1 - by0, bx1 - bx0) // 1000)
    return max(by0 - pad, 0), min(by1 + pad, hf), max(bx0 - pad, 0), min(bx1 + pad, wf), by1 - by0 + 2 * pad, bx1 - bx0 + 2 * pad


def test_next_window_is_a_valid_ladder_window_that_holds_the_padded_box():
    rng = np.random.default_rng(5)
    hf, wf, hn, wn = 96, 172, 24, 43
    n_checked = 0
    for trial in range(300):
        levels = int(rng.choice([1, 3, 8, 64]))
        permille, min_pad = int(rng.choice([0, 250, 1000, 4000])), int(rng.choice([0, 4, 16]))
        sizes = W.ladder(hf, wf, hn, wn, levels)
        hw, ww = sizes[int(rng.integers(0, levels + 1))]
        window = (int(rng.integers(0, hf - hw + 1)), int(rng.integers(0, wf - ww + 1)), hw, ww)
        i0, j0 = int(rng.integers(0, hn)), int(rng.integers(0, wn))
        x = C.blob(hn, wn, (i0, int(rng.integers(i0, hn))), (j0, int(rng.integers(j0, wn))))
        got = W.next_window(x, window, hf, wf, levels, permille, min_pad)
        assert W.sanitize(got, hf, wf, hn, wn) == got and got[2:] in sizes, (trial, got)
        top, bottom, left, right, need_h, need_w = padded_box(x, window, hf, wf, permille, min_pad)
        # the smallest level that is large enough
        k = sizes.index(got[2:])
        assert got[2] >= min(need_h, hf) and got[3] >= min(need_w, wf)
        assert k == 0 or not (sizes[k - 1][0] >= min(need_h, hf) and sizes[k - 1][1] >= min(need_w, wf))
        # it holds the padded box, cut to the frame
        assert got[0] <= top and got[0] + got[2] >= bottom and got[1] <= left and got[1] + got[3] >= right, (trial, got)
        n_checked += 1
    assert n_checked == 300


def test_next_window_edge_cases():
    hf, wf, hn, wn = 96, 172, 24, 43
    whole = (0, 0, hf, wf)
    some = (10, 20, 48, 86)
    empty = np.full((hn, wn), -1.0, dtype=np.float32)
    assert W.next_window(empty, some, hf, wf) == whole                        # a lost object is looked for everywhere
    assert W.next_window(np.full((hn, wn), np.nan, dtype=np.float32), some, hf, wf) == whole
    x = empty.copy()
    x[5, 7] = -0.0                                                            # -0.0 is object
    got = W.next_window(x, some, hf, wf, 8, 0, 0)
    assert got != whole and got[0] <= 10 + 5 * 48 // 24 and got[1] <= 20 + 7 * 86 // 43
    x[5, 7] = np.nan                                                          # a NaN is not
    assert W.next_window(x, some, hf, wf) == whole
    # one pixel in a corner of the map, seen through the whole frame: the smallest level, clamped to that corner
    for i, j in ((0, 0), (0, wn - 1), (hn - 1, 0), (hn - 1, wn - 1)):
        x = empty.copy()
        x[i, j] = 1.0
        # the pixel covers 4 x 4 frame pixels; pad 4 + 1: 14 x 14 needed, level 0 is 24 x 43
        got = W.next_window(x, whole, hf, wf, 8, 250, 4)
        assert got[2:] == (hn, wn)
        assert got[0] == (hf - hn if i else 0) and got[1] == (wf - wn if j else 0), ((i, j), got)
    # a static object: the second step changes nothing
    x = C.blob(hn, wn, (8, 13), (15, 25))
    first = W.next_window(x, whole, hf, wf, 8, 250, 4)
    img = np.zeros((hf, wf), dtype=np.float32) - 1
    img[32:56, 60:104] = 1.0                                                  # the same object, as the frame holds it

    def seen_through(window):
        y0, x0, hw, ww = window
        s = R.box_weights(hw, hn).astype(np.float64) @ img[y0:y0 + hw, x0:x0 + ww].astype(np.float64) @ \
            R.box_weights(ww, wn).astype(np.float64).T
        return np.where(s / (hw * ww) > -1.0, 1.0, -1.0).astype(np.float32)   # any object pixel under the net pixel

    assert first == W.next_window(seen_through(whole), whole, hf, wf, 8, 250, 4)
    second = W.next_window(seen_through(first), first, hf, wf, 8, 250, 4)
    assert second == W.next_window(seen_through(second), second, hf, wf, 8, 250, 4)  # a fixed point after one step
    for bad in (dict(levels=0), dict(levels=65), dict(margin_permille=-1), dict(margin_permille=4001), dict(min_pad=-1),
                dict(min_pad=4096), dict(min_pad=1.5)):
        with pytest.raises(ValueError):
            W.next_window(x, whole, hf, wf, **bad)


def test_window_of_mask_is_next_window_of_the_annotation():
    hf, wf, hn, wn = 96, 172, 48, 86
    mask = np.zeros((hf, wf), dtype=np.uint8)
    mask[30:50, 100:140] = 255
    got = W.window_of_mask(mask, hn, wn, 4, 250, 4)
    pad = 4 + (250 * 40 + 999) // 1000
    sizes = W.ladder(hf, wf, hn, wn, 4)
    want_size = next(s for s in sizes if s[0] >= 20 + 2 * pad and s[1] >= 40 + 2 * pad)
    assert got[2:] == want_size and got[0] <= 30 - pad and got[1] <= 100 - pad
    assert got[0] + got[2] >= 50 + pad and got[1] + got[3] >= 140 + pad
    assert W.window_of_mask(mask != 0, hn, wn, 4, 250, 4) == got
    assert W.window_of_mask(np.zeros((hf, wf), dtype=bool), hn, wn) == (0, 0, hf, wf)
    with pytest.raises(ValueError):
        W.window_of_mask(mask.astype(np.float32), hn, wn)


# ------------------------------------------------------------------------------------------ the loop
def disc_frames(count, hf, wf, radius, cy, cx, dy, dx):
    yy, xx = np.mgrid[0:hf, 0:wf]
    rng = np.random.default_rng(1)
    out, centres = [], []
    for k in range(count):
        f = rng.integers(0, 60, (hf, wf, 3), dtype=np.uint8)
        y, x = cy + dy * k, cx + dx * k
        f[..., 2][(yy - y) ** 2 + (xx - x) ** 2 <= radius ** 2] = 250
        out.append(f)
        centres.append((y, x))
    return out, centres


@pytest.mark.parametrize("mirror", [False, True])
def test_track_keeps_a_drifting_disc_inside_every_window(mirror):
    hf, wf, hn, wn, radius, min_pad = 120, 200, 30, 50, 12, 6
    frames, centres = disc_frames(14, hf, wf, radius, 30, 40, 3, 5)  # moves by less than min_pad a frame
    seen_logits = []

    def net_fn(image):
        seen_logits.append(C.threshold_net_fn(image))
        return seen_logits[-1]

    outs, used, last = W.track(frames, net_fn, hn, wn, mirror=mirror, levels=6, margin_permille=0, min_pad=min_pad)
    assert len(outs) == len(used) == 14 and used[0] == (0, 0, hf, wf)
    assert len({w[2:] for w in used[1:]}) >= 1 and used[1][2:] != (hf, wf)  # it did zoom in
    for k, (f, window) in enumerate(zip(frames, used)):
        assert W.sanitize(window, hf, wf, hn, wn) == window
        y, x = centres[k]
        if mirror:
            x = wf - 1 - x
        assert window[0] <= y - radius and y + radius < window[0] + window[2], (k, window)
        assert window[1] <= x - radius and x + radius < window[1] + window[3], (k, window)
        assert np.array_equal(outs[k], W.apply_window(f, seen_logits[k], window, mirror))
        assert (seen_logits[k] >= 0).any()
    assert last == W.next_window(seen_logits[-1], used[-1], hf, wf, 6, 0, min_pad)
    # the same from an annotation of the first frame: the first window is window_of_mask's
    mask = F.mirrored(frames[0], mirror)[..., 2] > 200
    start = W.window_of_mask(mask, hn, wn, 6, 0, min_pad)
    _, used2, _ = W.track(frames, C.threshold_net_fn, hn, wn, mirror=mirror, levels=6, margin_permille=0, min_pad=min_pad,
                          window=start)
    assert used2[0] == start and start[2:] != (hf, wf)


# ------------------------------------------------------------------------------------------ options
def test_roi_options_validate():
    from fosvos_hip.options import RoiOptions
    r = RoiOptions()
    assert (r.levels, r.margin, r.min_pad, r.margin_permille) == (8, 0.25, 16, 250)
    assert RoiOptions(levels=1, margin=0, min_pad=0).margin_permille == 0 and RoiOptions(levels=64, margin=4, min_pad=4095)
    assert RoiOptions(margin=0.0004).margin_permille == 0 and RoiOptions(margin=0.0006).margin_permille == 1
    assert r.as_dict() == {'levels': 8, 'margin': 0.25, 'min_pad': 16}
    for bad in (dict(levels=0), dict(levels=65), dict(levels=2.0), dict(levels=True), dict(margin=-0.1), dict(margin=4.1),
                dict(margin=float("nan")), dict(margin=float("inf")), dict(margin="1"), dict(margin=True), dict(min_pad=-1),
                dict(min_pad=4096), dict(min_pad=1.0), dict(min_pad=False)):
        with pytest.raises(ValueError):
            RoiOptions(**bad)


BASE = ["--synthetic", "1", "--height", "24", "--width", "40"]
SIZE = ["--net-height", "12", "--net-width", "20"]


@pytest.mark.parametrize("extra,reason", [
    (["--roi"], "--net-height"),
    (["--roi", "--net-height", "12"], "both or neither"),
    (["--roi"] + SIZE + ["--no-network"], "--no-network"),
    (["--roi"] + SIZE + ["--models", "a.pth", "b.pth"], "--models"),
    (["--roi"] + SIZE + ["--clean-temporal", "2"], "--clean-temporal"),
    (SIZE + ["--roi-levels", "4"], "--roi-levels is an option of --roi"),
    (SIZE + ["--roi-margin", "0.5"], "--roi-margin is an option of --roi"),
    (SIZE + ["--roi-min-pad", "4"], "--roi-min-pad is an option of --roi"),
    (SIZE + ["--roi-seed", "a.png"], "--roi-seed is an option of --roi"),
    (["--roi"] + SIZE + ["--roi-levels", "0"], "--roi-levels"),
    (["--roi"] + SIZE + ["--roi-levels", "65"], "--roi-levels"),
    (["--roi"] + SIZE + ["--roi-margin", "4.5"], "--roi-margin"),
    (["--roi"] + SIZE + ["--roi-margin", "nan"], "--roi-margin"),
    (["--roi"] + SIZE + ["--roi-min-pad", "-1"], "--roi-min-pad"),
    (["--roi"] + SIZE + ["--roi-min-pad", "4096"], "--roi-min-pad"),
    (["--roi"] + SIZE + ["--roi-levels", "many"], "invalid int"),
])
def test_run_webcam_refuses_roi_combinations_with_a_reason(capsys, extra, reason):
    import run_webcam
    with pytest.raises(SystemExit):  # argparse level: refused before anything is read, loaded or launched
        run_webcam.main(BASE + extra)
    assert reason in capsys.readouterr().err


def test_run_webcam_roi_options_combine():
    import run_webcam
    from fosvos_hip.options import RoiOptions
    parser = run_webcam.build_parser()

    def parsed(extra):
        args = parser.parse_args(BASE + extra)
        return args, run_webcam.roi_of(parser, args, run_webcam.net_size_of(parser, args)), run_webcam.clean_of(parser, args)

    args, roi, clean = parsed([])
    assert roi is None and clean is None and args.roi is False and args.roi_seed is None
    _, roi, _ = parsed(["--roi"] + SIZE)
    assert roi == RoiOptions()
    args, roi, clean = parsed(["--roi"] + SIZE + ["--roi-levels", "4", "--roi-margin", "0.5", "--roi-min-pad", "3", "--roi-seed", "m.png",
                                                  "--clean-largest", "--clean-min-area", "9", "--no-mirror", "--depth", "3",
                                                  "--output-format", "jpeg", "--output", "x.avi", "--jpeg-subsampling", "420",
                                                  "--device-decode", "--no-overlay"])
    assert roi == RoiOptions(levels=4, margin=0.5, min_pad=3) and args.roi_seed == "m.png"
    assert clean.largest and clean.min_area == 9 and clean.temporal_radius is None
