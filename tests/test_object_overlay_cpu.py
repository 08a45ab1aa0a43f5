"""The several-objects overlay as numpy states it (util/object_overlay.py), without a GPU: against a per-pixel restatement in
plain Python, against the modules it is built from, its edge cases, and the coverage the GPU tests rely on - asserted here on
the reference alone, so that a GPU test cannot pass vacuously.  Also ``run_webcam --models``' rejections."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import object_overlay_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402
from util import object_merge as M  # noqa: E402
from util import object_overlay as OO  # noqa: E402


# ------------------------------------------------------------------------------------------ the restatement
def pixel_label(values):
    """The rule on one pixel, in plain Python floats."""
    best, label = None, 0
    for k, v in enumerate(values):
        v = float(v)
        if math.isnan(v) or not v >= 0.0:
            continue
        if best is None or v > best:
            best, label = v, k + 1
    return label


def tap(x, n_src, n_dst):
    num = (2 * x + 1) * n_src - n_dst
    i0, r = num // (2 * n_dst), num % (2 * n_dst)
    if num < 0:
        i0, r = 0, 0
    if i0 >= n_src - 1:
        i0, r = n_src - 1, 0
    return i0, min(i0 + 1, n_src - 1), float(2 * n_dst - r), float(r)


def pixel_value_up(a, y, x, hf, wf):
    hn, wn = a.shape
    y0, y1, wy0, wy1 = tap(y, hn, hf)
    x0, x1, wx0, wx1 = tap(x, wn, wf)
    top = float(a[y0, x0]) * wx0 + float(a[y0, x1]) * wx1
    bot = float(a[y1, x0]) * wx0 + float(a[y1, x1]) * wx1
    return top * wy0 + bot * wy1


def python_labels(maps, hf=None, wf=None):
    h, w = (hf, wf) if hf is not None else maps[0].shape
    out = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            out[y, x] = pixel_label([m[y, x] if hf is None else pixel_value_up(m, y, x, hf, wf) for m in maps])
    return out


def python_overlay(img, lab, mirror, palette, alpha):
    h, w, _ = img.shape
    out = np.zeros((h, w, 3), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            src = img[y, w - 1 - x] if mirror else img[y, x]
            for c in range(3):
                b = float(src[c])
                if lab[y, x] == 0:
                    out[y, x, c] = src[c]
                else:
                    col = float(palette[lab[y, x]][2 - c])
                    out[y, x, c] = int(math.trunc(b + float(alpha) * (col - b) + 0.5))
    return out


# ------------------------------------------------------------------------------------------ labels and overlay
def test_labels_without_sizes_is_merge_labels():
    for (n, h, w) in C.SHAPES:
        for k in C.KS:
            maps = C.logits(k, n, h, w)
            want = M.merge_labels(np.stack([m[:, 0] for m in maps]))
            for f in range(n):
                assert np.array_equal(OO.labels(C.frame_maps(maps, f)), want[f]), (n, h, w, k, f)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.SHAPE_IDS)
def test_unscaled_equals_the_python_restatement(shape):
    n, h, w = shape
    img = C.frames(n, h, w)
    pals = C.palettes()
    for ki, k in enumerate(C.KS):
        maps = C.logits(k, n, h, w)
        for f in range(n):
            fm = C.frame_maps(maps, f)
            lab = python_labels(fm)
            assert np.array_equal(OO.labels(fm), lab), (shape, k, f)
            for mi, mirror in enumerate((False, True)):
                for pi, (name, pal) in enumerate(pals.items()):
                    alpha = C.ALPHAS[(ki + mi + pi + f) % len(C.ALPHAS)]
                    want = python_overlay(img[f], lab, mirror, M.davis_palette() if pal is None else pal, alpha)
                    got = OO.overlay(img[f], fm, mirror, pal, alpha)
                    assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, k, f, mirror, name, alpha)
                    assert np.array_equal(OO.apply(img[f], fm, mirror, True, pal, alpha), want)
            assert np.array_equal(OO.apply(img[f], fm, True, False, None, 0.5), lab)


@pytest.mark.parametrize("size", C.SCALED, ids=C.SCALED_IDS)
def test_scaled_equals_the_python_restatement(size):
    hf, wf, hn, wn = size
    img = C.frames(C.SCALED_N, hf, wf)
    pal = C.random_palette()
    for ki, k in enumerate(C.KS):
        maps = C.logits_scaled(k, C.SCALED_N, hn, wn)
        for f in range(C.SCALED_N):
            fm = C.frame_maps(maps, f)
            lab = python_labels(fm, hf, wf)
            assert np.array_equal(OO.labels(fm, hf, wf), lab), (size, k, f)
            alpha = C.ALPHAS[(ki + f) % len(C.ALPHAS)]
            for mirror in (False, True):
                want = python_overlay(img[f], lab, mirror, pal, alpha)
                assert np.array_equal(OO.overlay(img[f], fm, mirror, pal, alpha, hf, wf), want), (size, k, f, mirror)
            assert np.array_equal(OO.apply(img[f], fm, False, False, pal, alpha, hf, wf), lab)


def test_one_object_is_the_single_object_mask():
    for (n, h, w) in C.SHAPES:
        maps = C.logits(1, n, h, w)
        for f in range(n):
            assert np.array_equal(OO.labels([maps[0][f, 0]]), F.mask_bytes(maps[0][f, 0], True) // 255)
    for (hf, wf, hn, wn) in C.SCALED:
        maps = C.logits_scaled(1, C.SCALED_N, hn, wn)
        for f in range(C.SCALED_N):
            assert np.array_equal(OO.labels([maps[0][f, 0]], hf, wf), R.mask_bytes_scaled(maps[0][f, 0], hf, wf, True) // 255)


def test_alpha_zero_is_the_frame_and_alpha_one_the_colour():
    pal = C.random_palette()
    for (n, h, w) in C.SHAPES:
        img, maps = C.frames(n, h, w), C.logits(3, n, h, w)
        for f in range(n):
            fm = C.frame_maps(maps, f)
            lab = OO.labels(fm)
            for mirror in (False, True):
                src = img[f][:, ::-1] if mirror else img[f]
                assert np.array_equal(OO.overlay(img[f], fm, mirror, pal, 0.0), src)
                full = OO.overlay(img[f], fm, mirror, pal, 1.0)
                assert np.array_equal(full[lab > 0], pal[lab[lab > 0]][:, ::-1])  # RGB -> BGR
                assert np.array_equal(full[lab == 0], src[lab == 0])


def test_swapping_two_maps_that_never_tie_renames_the_labels():
    rng = np.random.default_rng(5)
    a = (rng.integers(-16, 17, (9, 13)) * 0.25).astype(np.float32)
    b = (a + rng.choice([-0.125, 0.125], a.shape)).astype(np.float32)  # never equal to a, exact in float32
    c = (rng.integers(-16, 17, (9, 13)) * 0.25).astype(np.float32)
    one, two = OO.labels([a, b, c]), OO.labels([b, a, c])
    assert set(np.unique(one).tolist()) == {0, 1, 2, 3}
    rename = np.array([0, 2, 1, 3], dtype=np.uint8)
    assert np.array_equal(two, rename[one])
    b = (a + np.float32(0.125)).astype(np.float32)  # a constant offset stays one under interpolation
    assert np.array_equal(OO.labels([b, a, c], 20, 31), rename[OO.labels([a, b, c], 20, 31)])


def test_bad_arguments_raise():
    img = C.frames(1, 5, 7)[0]
    maps = C.frame_maps(C.logits(2, 1, 5, 7), 0)
    for alpha in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            OO.overlay(img, maps, alpha=alpha)
        with pytest.raises(ValueError):
            OO.apply(img, maps, overlay_on=False, alpha=alpha)
    for bad in (lambda: OO.labels([]), lambda: OO.labels([maps[0]] * 17), lambda: OO.labels([maps[0].astype(np.float64)]),
                lambda: OO.labels([maps[0], maps[1][:4]]), lambda: OO.labels([maps[0][np.newaxis]]),
                lambda: OO.labels(maps, 5), lambda: OO.labels(maps, 4, 7),               # smaller than the maps
                lambda: OO.overlay(img, maps, palette=np.zeros((255, 3), np.uint8)),
                lambda: OO.overlay(img, maps, palette=np.zeros((256, 3), np.int32)),
                lambda: OO.overlay(img.astype(np.int32), maps), lambda: OO.overlay(img[:4], maps),
                lambda: OO.overlay(img, maps, hf=10, wf=14),                             # not the frame's size
                lambda: OO.apply(img[:4], maps, overlay_on=False)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ what the GPU tests rely on
def test_cases_cover_every_label_ties_and_exact_zeros():
    for k in C.KS:
        seen, tie = set(), False
        for (n, h, w) in C.SHAPES:
            maps = C.logits(k, n, h, w)
            x = np.stack([m[:, 0] for m in maps])
            lab = M.merge_labels(x)
            if n * h * w >= k + 1:
                seen |= set(np.unique(lab).tolist())
            valid = x >= 0
            top = np.where(valid, x, -np.inf).max(axis=0)
            tie |= bool((((x == top) & valid).sum(axis=0) >= 2).any())
        assert seen == set(range(k + 1)), (k, seen)
        assert tie or k == 1, k
        seen, tie, zero = set(), False, False
        for (hf, wf, hn, wn) in C.SCALED:
            maps = C.logits_scaled(k, C.SCALED_N, hn, wn)
            for f in range(C.SCALED_N):
                v = np.stack([R.logits_up(m[f, 0], hf, wf) for m in maps])
                assert np.isfinite(v).all()
                seen |= set(np.unique(OO.labels(C.frame_maps(maps, f), hf, wf)).tolist())
                top = np.where(v >= 0, v, -np.inf).max(axis=0)
                tie |= bool((((v == top) & (v >= 0)).sum(axis=0) >= 2).any())
                zero |= bool((v == 0).any())
        assert seen == set(range(k + 1)), (k, seen)
        assert (tie or k == 1) and zero, (k, tie, zero)


def test_random_palette_differs_from_its_reverse():
    pal = C.random_palette()
    assert pal.dtype == np.uint8 and pal.shape == (256, 3) and (pal != pal[:, ::-1])[:, [0, 2]].all()
    assert M.davis_palette()[1].tolist() == [128, 0, 0]  # red first: RGB


# ------------------------------------------------------------------------------------------ run_webcam --models
def test_run_webcam_models_rejections(capsys):
    import run_webcam
    p = run_webcam.build_parser()
    args = p.parse_args(["--models", "a.pth", "b.pth", "c.pth", "--palette-alpha", "0.25", "--variant", "vgg"])
    assert args.models == ["a.pth", "b.pth", "c.pth"] and args.palette_alpha == 0.25 and args.model is None
    assert p.parse_args([]).models is None and p.parse_args([]).palette_alpha == 0.5
    for argv, word in ((["--models", "a.pth", "--model", "b.pth"], "--model"),
                       (["--models", "a.pth", "--no-network"], "--no-network"),
                       (["--models", "a.pth", "-nn"], "--no-network"),
                       (["--models", "a.pth", "--overlay-color", "g"], "--overlay-color"),
                       (["--models", "a.pth", "-oc", "r"], "--overlay-color"),
                       (["--models", "a.pth", "--overlay-alpha=1.0"], "--overlay-alpha"),
                       (["--models", "a.pth", "--no-boolean-mask"], "--no-boolean-mask"),
                       (["--models", "a.pth", "-nbm"], "--no-boolean-mask"),
                       (["--models", "a.pth", "--palette-alpha", "1.5"], "--palette-alpha"),
                       (["--models"] + ["a.pth"] * 17, "16"),
                       (["--models"], "--models")):
        with pytest.raises(SystemExit) as info:
            run_webcam.main(argv + ["--synthetic", "1"])
        assert info.value.code == 2
        assert word in capsys.readouterr().err, (argv, word)
