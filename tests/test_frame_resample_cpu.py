"""The resampling of streaming inference as util/frame_resample.py states it: the area average against exact fractions and
PIL, the upsample against torch's float64 bilinear, and the options of run_webcam.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_resample_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402


def test_area_sums_are_the_exact_area_average():
    hf, wf, hn, wn = 7, 9, 3, 4
    img = np.random.default_rng(0).integers(0, 256, (hf, wf, 3), dtype=np.uint8)
    s = R.area_sums(img, hn, wn)
    assert s.dtype == np.int64 and s.shape == (hn, wn, 3)
    for i in range(hn):
        for j in range(wn):
            for c in range(3):
                total = Fraction(0)
                for y in range(hf):
                    oy = max(Fraction(0), min(Fraction(y + 1), Fraction((i + 1) * hf, hn)) - max(Fraction(y), Fraction(i * hf, hn)))
                    for x in range(wf):
                        ox = max(Fraction(0),
                                 min(Fraction(x + 1), Fraction((j + 1) * wf, wn)) - max(Fraction(x), Fraction(j * wf, wn)))
                        total += oy * ox * int(img[y, x, c])
                mean = total / (Fraction(hf, hn) * Fraction(wf, wn))  # the area sum over the pixel's area
                assert mean == Fraction(int(s[i, j, c]), hf * wf), (i, j, c)


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_weight_rows_sum_to_the_source_and_mirror_commutes(case):
    n, hf, wf, hn, wn = case
    for n_src, n_dst in ((hf, hn), (wf, wn)):
        w = R.box_weights(n_src, n_dst)
        assert w.shape == (n_dst, n_src) and (w.sum(axis=1) == n_src).all() and (w.sum(axis=0) == n_dst).all()
        assert np.array_equal(w, w[::-1, ::-1])  # symmetric
    f = C.frames(n, hf, wf)
    for k in range(n):
        s = R.area_sums(f[k], hn, wn)
        assert 0 <= s.min() and s.max() <= 255 * hf * wf
        plain, flipped = R.prepare_frame_scaled(f[k], hn, wn, False), R.prepare_frame_scaled(f[k], hn, wn, True)
        assert plain.dtype == np.float32 and plain.shape == (1, 3, hn, wn) and flipped.flags.c_contiguous
        assert flipped.tobytes() == np.ascontiguousarray(plain[..., ::-1]).tobytes()
    if (hn, wn) == (hf, wf):
        assert plain.tobytes() == F.prepare_frame(f[-1]).tobytes()


def test_equal_sizes_are_the_unscaled_definitions():
    f, x = C.frames(1, 33, 47)[0], C.logits(1, 33, 47)[0, 0]
    assert R.prepare_frame_scaled(f, 33, 47, True).tobytes() == F.prepare_frame(f, True).tobytes()
    v = R.logits_up(x, 33, 47)
    assert v.dtype == np.float64 and np.array_equal(v / (4.0 * 33 * 47), x.astype(np.float64))  # the identity
    for boolean in (True, False):
        assert np.array_equal(R.overlay_scaled(f, x, True, boolean, "g", 0.5), F.overlay(f, x, True, boolean, "g", 0.5))
        assert np.array_equal(R.apply_scaled(f, x, False, False, boolean), F.mask_bytes(x, boolean))


@pytest.mark.parametrize("case", [c for c in C.CASES if C.integer_ratio(c)], ids=lambda c: "%dx%dx%d_to_%dx%d" % c)
def test_rounded_mean_is_within_one_level_of_pil_reduce(case):
    n, hf, wf, hn, wn = case
    f = C.frames(n, hf, wf)
    for k in range(n):
        mine = np.rint(R.area_sums(f[k], hn, wn) / (hf * wf)).astype(np.int32)
        pil = np.asarray(Image.fromarray(f[k]).reduce((wf // wn, hf // hn))).astype(np.int32)
        assert pil.shape == mine.shape
        print(case, "levels apart from PIL.Image.reduce: max", int(np.abs(mine - pil).max()), "differing", int((mine != pil).sum()))
        assert np.abs(mine - pil).max() <= 1


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_upsample_is_torchs_float64_bilinear(case):
    n, hf, wf, hn, wn = case
    x = C.logits(n, hn, wn)
    for k in range(n):
        mine = R.logits_up(x[k, 0], hf, wf) / (4.0 * hf * wf)
        ref = torch.nn.functional.interpolate(torch.from_numpy(x[k:k + 1].astype(np.float64)), size=(hf, wf), mode="bilinear",
                                              align_corners=False)[0, 0].numpy()
        err = float(np.abs(mine - ref).max())
        print(case, "max |mine - torch| = %.3g" % err)
        assert err <= 1e-9 * float(np.abs(x[k]).max())
    i0, i1, w0, w1 = R.taps(wn, wf)
    assert (w0 + w1 == 2 * wf).all() and i0.min() >= 0 and i1.max() <= wn - 1 and ((i1 - i0) <= 1).all()


def test_scaled_overlay_known_answers_and_checks():
    img = np.full((2, 4, 3), 100, dtype=np.uint8)
    lg = np.array([[-1.0, 3.0]], dtype=np.float32)   # [1,2] -> [2,4]: columns at -1, -1 + 1/4 * 4 = 0 ... 3
    v = R.logits_up(lg, 2, 4)
    assert (v[0] == v[1]).all() and v[0].tolist() == [-32.0, 0.0, 64.0, 96.0]   # 4 Hf Wf = 32 times -1, 0, 2, 3
    assert R.mask_bytes_scaled(lg, 2, 4).tolist() == [[0, 255, 255, 255]] * 2   # zero counts as object
    out = R.overlay_scaled(img, lg, False, True, "r", 0.5)
    assert out[:, :, 2].tolist() == [[100, 227, 227, 227]] * 2 and (out[:, :, :2] == 100).all()
    assert R.apply_scaled(img, lg, overlay_on=False, boolean_mask=False)[0].tolist() == [
        int(255 / (1 + np.exp(-t)) + 0.5) for t in (-1.0, 0.0, 2.0, 3.0)]
    for bad in (lambda: R.area_sums(img, 3, 4), lambda: R.area_sums(img, 2, 5), lambda: R.area_sums(img, 0, 4),
                lambda: R.logits_up(lg, 2, 1), lambda: R.logits_up(lg.astype(np.float64), 2, 4),
                lambda: R.overlay_scaled(img, lg, color="x"), lambda: R.apply_scaled(img, lg, overlay_on=False, alpha=-1.0),
                lambda: R.prepare_frame_scaled(img.astype(np.float32), 1, 2)):
        with pytest.raises(ValueError):
            bad()


def test_run_webcam_takes_the_net_size_options():
    import run_webcam
    p = run_webcam.build_parser()
    a = p.parse_args([])
    assert a.net_height is None and a.net_width is None and run_webcam.net_size_of(p, a) is None
    a = p.parse_args(["--net-height", "480", "--net-width", "854"])
    assert run_webcam.net_size_of(p, a) == (480, 854)
    for argv in (["--net-height", "480"], ["--net-width", "854"], ["--net-height", "0", "--net-width", "854"]):
        with pytest.raises(SystemExit):
            run_webcam.net_size_of(p, p.parse_args(argv))
    with pytest.raises(SystemExit):
        run_webcam.main(["--synthetic", "1", "--net-width", "854"])  # refused before anything is opened
