"""The numpy definition of the edge-aware upsampling (util/guided_upsample.py), without a GPU: the box sums against a per-pixel
double loop, the coefficients against the textbook guided filter, the denominator's sign, non-finite logits, the constant
frame, the mirror, the edge-snap case, RefineOptions, the options of run_webcam and the segmenters' refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import guided_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402
from util import guided_upsample as G  # noqa: E402


# ------------------------------------------------------------------------------------------ the box sum
@pytest.mark.parametrize("r", [1, 3, 8])
def test_box_sum_and_count_are_the_per_pixel_loops(r):
    h, w = 6, 7
    v = np.random.default_rng(r).standard_normal((h, w)) * 1e3
    n = G.window_count(h, w, r)
    s = G.box_sum(v, r)
    for y in range(h):
        for x in range(w):
            ya, yb, xa, xb = max(0, y - r), min(h - 1, y + r), max(0, x - r), min(w - 1, x + r)
            assert n[y, x] == (yb - ya + 1) * (xb - xa + 1)
            total = 0.0
            for xx in range(xa, xb + 1):   # columns last: the sum over columns of the sums over rows, both ascending
                col = 0.0
                for yy in range(ya, yb + 1):
                    col = col + v[yy, xx]
                total = total + col
            assert s[y, x] == total, (y, x)   # bit for bit: the order is the definition
    assert n.dtype == np.float64 and s.dtype == np.float64
    with pytest.raises(ValueError):
        G.box_sum(v.astype(np.float32), r)


def test_box_sum_starts_from_plus_zero():
    v = np.full((3, 3), -0.0)
    assert not np.signbit(G.box_sum(v, 1)).any()   # 0.0 + -0.0 = +0.0


# ------------------------------------------------------------------------------------------ the filter
def textbook(image, logits, r, eps, clip):
    """He et al.'s guided filter in its mean form, means by cumsum."""
    g = image.astype(np.float64).sum(axis=0)
    p = np.clip(np.nan_to_num(logits.astype(np.float64), nan=-clip, posinf=clip, neginf=-clip), -clip, clip)
    h, w = g.shape

    def mean(v):
        c = np.zeros((h + 1, w + 1))
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        y, x = np.arange(h), np.arange(w)
        ya, yb, xa, xb = np.maximum(0, y - r), np.minimum(h - 1, y + r) + 1, np.maximum(0, x - r), np.minimum(w - 1, x + r) + 1
        s = c[yb][:, xb] - c[ya][:, xb] - c[yb][:, xa] + c[ya][:, xa]
        return s / ((yb - ya)[:, None] * (xb - xa)[None, :])

    mg, mp = mean(g), mean(p)
    a = (mean(g * p) - mg * mp) / (mean(g * g) - mg * mg + eps)
    b = mp - a * mg
    return np.stack([mean(a), mean(b)])


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_coefficients_are_the_textbook_guided_filter(case):
    n, hf, wf, hn, wn, r = case
    f, im, x, coeff = C.reference(case, "random", 400.0)
    for k in range(n):
        want = textbook(im[k], x[k, 0], r, 400.0, C.CLIP)
        scale = np.abs(want).max(axis=(1, 2), keepdims=True)
        assert (np.abs(coeff[k] - want) <= 1e-9 * scale).all(), (case, float(np.abs(coeff[k] - want).max()))
    assert coeff.dtype == np.float64 and coeff.shape == (n, 2, hn, wn)


@pytest.mark.parametrize("kind", C.KINDS)
def test_denominator_is_positive_at_the_smallest_eps(kind):
    for case in C.CASES:
        n, hf, wf, hn, wn, r = case
        f, x = C.frames(n, hf, wf, kind), C.logits(n, hn, wn)
        im = C.images(f, hn, wn)
        for k in range(n):
            a, b, den = G.fit(im[k], x[k, 0], r, 1e-3, C.CLIP)
            assert (den > 0).all() and np.isfinite(a).all() and np.isfinite(b).all(), (case, kind, float(den.min()))
    # full-size frames of the two degenerate kinds: a constant guide and a 0 / 255 step
    f = C.frames(1, 48, 86, kind)
    _, _, den = G.fit(C.images(f, 48, 86)[0], C.logits(1, 48, 86)[0, 0], 8, 1e-3, C.CLIP)
    print(kind, "smallest den", float(den.min()))
    assert (den > 0).all()


def test_non_finite_logits_give_finite_coefficients_and_nan_is_minus_clip():
    n, hf, wf, hn, wn, r = case = C.CASES[1]
    f, im, x, coeff = C.reference(case, "random", 1e-3)
    assert not np.isfinite(x).all() and np.isnan(x).any() and np.isfinite(coeff).all()
    y = x.copy()
    y[np.isnan(x)] = -C.CLIP
    y[x == np.inf] = C.CLIP
    y[x == -np.inf] = -C.CLIP
    y[x == np.float32(1e30)] = 7.0        # anything above the clip is the clip
    y[x == np.float32(-1e30)] = -1e3      # ... and below it
    y[x == -100.0] = -6.5
    assert (x == np.float32(1e30)).any() and (x == -100.0).any()
    for k in range(n):
        assert G.coefficients(im[k], y[k, 0], r, 1e-3, C.CLIP).tobytes() == coeff[k].tobytes()
    g, p = G.guide_and_target(im[0], x[0, 0], C.CLIP)
    assert (p[np.isnan(x[0, 0])] == -C.CLIP).all() and np.abs(p).max() == C.CLIP


def test_a_constant_frame_gives_the_twice_smoothed_target():
    n, hf, wf, hn, wn, r = case = C.CASES[1]
    f, im, x, coeff = C.reference(case, "constant", 400.0)
    assert (np.abs(coeff[:, 0]) < 1e-9).all()
    for k in range(n):
        _, p = G.guide_and_target(im[k], x[k, 0], C.CLIP)
        cnt = G.window_count(hn, wn, r)
        twice = G.box_sum(G.box_sum(p, r) / cnt, r) / cnt
        v = G.refined_up(coeff[k], f[k]) / (4.0 * hf * wf)
        assert np.abs(v - G.map_up(twice, hf, wf) / (4.0 * hf * wf)).max() < 1e-6


@pytest.mark.parametrize("case", C.CASES[:4], ids=C.IDS[:4])
def test_mirror_is_the_flipped_frame(case):
    n, hf, wf, hn, wn, r = case
    f, x = C.frames(n, hf, wf), C.logits(n, hn, wn)
    for k in range(n):
        flipped = np.ascontiguousarray(f[k][:, ::-1])
        im_m, im_f = C.images(f[k:k + 1], hn, wn, True), C.images(flipped[None], hn, wn, False)
        assert im_m.tobytes() == im_f.tobytes()
        for overlay_on in (True, False):
            for boolean in (True, False):
                a = G.apply_guided(f[k], im_m, x[k, 0], True, overlay_on, boolean, "g", 0.5, r, 400.0, C.CLIP)
                b = G.apply_guided(flipped, im_f, x[k, 0], False, overlay_on, boolean, "g", 0.5, r, 400.0, C.CLIP)
                assert a.tobytes() == b.tobytes() and a.shape == ((hf, wf, 3) if overlay_on else (hf, wf))


def test_equal_sizes_use_identity_taps():
    n, hf, wf, hn, wn, r = case = C.CASES[3]
    f, im, x, coeff = C.reference(case, "random", 400.0)
    v = G.refined_up(coeff[0], f[0])
    up = lambda m: (m * (2.0 * wf)) * (2.0 * hf)   # the weights of a tap that hits its pixel: (2 Wf, 0) and (2 Hf, 0)
    assert np.array_equal(v, up(coeff[0, 0]) * G.frame_guide(f[0]) + up(coeff[0, 1]))


def test_the_filter_snaps_a_shifted_mask_to_the_frames_edge():
    frame, truth, lg = C.ellipse_case()
    hf, wf = truth.shape
    bilinear = R.logits_up(lg, hf, wf) >= 0
    image = R.prepare_frame_scaled(frame, lg.shape[0], lg.shape[1])[0]
    guided = G.refined_up(G.coefficients(image, lg, 4, 400.0, 6.0), frame) >= 0
    iou_b, iou_g = C.iou(bilinear, truth), C.iou(guided, truth)
    print("IoU bilinear %.4f guided %.4f" % (iou_b, iou_g))
    assert iou_g >= iou_b + 0.05
    assert np.array_equal(G.mask_bytes_guided(frame, G.coefficients(image, lg, 4, 400.0, 6.0)) == 255, guided)


def test_parameters_are_checked():
    im, x = np.zeros((3, 4, 5), dtype=np.float32), np.zeros((4, 5), dtype=np.float32)
    for bad in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(eps=1e-4), dict(eps=1e10),
                dict(eps=float("nan")), dict(eps="1"), dict(clip=0.0), dict(clip=-1.0), dict(clip=1e5), dict(clip=float("inf"))):
        with pytest.raises(ValueError):
            G.coefficients(im, x, **bad)
    for bad in ((im.astype(np.float64), x), (im[:2], x), (im, x[:3]), (im, x.astype(np.float64))):
        with pytest.raises(ValueError):
            G.coefficients(*bad)
    with pytest.raises(ValueError):
        G.refined_up(np.zeros((2, 4, 5), dtype=np.float32), np.zeros((8, 10, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        G.refined_up(np.zeros((2, 9, 5)), np.zeros((8, 10, 3), dtype=np.uint8))   # a map larger than the frame


# ------------------------------------------------------------------------------------------ options
def test_refine_options_validate():
    import dataclasses
    from fosvos_hip.options import RefineOptions
    o = RefineOptions()
    assert (o.radius, o.eps, o.clip) == (4, 400.0, 6.0) and o.as_dict() == {'radius': 4, 'eps': 400.0, 'clip': 6.0}
    assert RefineOptions(radius=1, eps=1e-3, clip=1e4) and RefineOptions(radius=8, eps=1e9, clip=1e-9) and RefineOptions(eps=1)
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.radius = 2
    for bad in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(eps=9e-4), dict(eps=1.1e9),
                dict(eps=float("nan")), dict(eps=float("inf")), dict(eps="1"), dict(eps=True), dict(clip=0), dict(clip=-6.0),
                dict(clip=1.1e4), dict(clip=float("nan")), dict(clip=False)):
        with pytest.raises(ValueError):
            RefineOptions(**bad)
    assert "unmeasured" in RefineOptions.__doc__ and "environ" in RefineOptions.__doc__


BASE = ["--synthetic", "1", "--height", "24", "--width", "40"]
SIZE = ["--net-height", "12", "--net-width", "20"]


@pytest.mark.parametrize("extra,reason", [
    (["--refine-radius", "3"], "--refine-radius is an option of --refine"),
    (["--refine-eps", "10"], "--refine-eps is an option of --refine"),
    (["--refine-clip", "4"], "--refine-clip is an option of --refine"),
    (["--refine", "--no-network"], "--no-network runs no net"),
    (["--refine", "--roi"] + SIZE, "--refine with --roi is not built"),
    (["--refine", "--models", "a.pth", "b.pth"], "--models) is not built"),
    (["--refine", "--refine-radius", "0"], "--refine-radius"),
    (["--refine", "--refine-radius", "9"], "--refine-radius"),
    (["--refine", "--refine-eps", "1e-4"], "--refine-eps"),
    (["--refine", "--refine-eps", "nan"], "--refine-eps"),
    (["--refine", "--refine-clip", "0"], "--refine-clip"),
    (["--refine", "--refine-clip", "inf"], "--refine-clip"),
    (["--refine", "--refine-radius", "wide"], "invalid int"),
])
def test_run_webcam_refuses_refine_combinations_with_a_reason(capsys, extra, reason):
    import run_webcam
    with pytest.raises(SystemExit):  # argparse level: refused before anything is read, loaded or launched
        run_webcam.main(BASE + extra)
    assert reason in capsys.readouterr().err


def test_run_webcam_refine_options_combine():
    import run_webcam
    from fosvos_hip.options import RefineOptions
    parser = run_webcam.build_parser()

    def parsed(extra):
        args = parser.parse_args(BASE + extra)
        return args, run_webcam.refine_of(parser, args)

    args, refine = parsed([])
    assert refine is None and args.refine is False
    assert parsed(["--refine"])[1] == RefineOptions() and parsed(["--refine"] + SIZE)[1] == RefineOptions()
    _, refine = parsed(["--refine", "--refine-radius", "2", "--refine-eps", "50", "--refine-clip", "3.5", "--clean-largest",
                        "--no-overlay", "--no-mirror", "--output-format", "jpeg", "--output", "x"])
    assert refine == RefineOptions(radius=2, eps=50.0, clip=3.5)


def test_segmenters_refuse_what_refine_does_not_go_with_before_the_device():
    from fosvos_hip.options import RefineOptions, RoiOptions
    from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
    net = object()   # never looked at: every refusal comes first
    with pytest.raises(ValueError, match="roi is not built"):
        FrameSegmenter(net, 24, 40, net_size=(12, 20), roi=RoiOptions(), refine=RefineOptions())
    with pytest.raises(ValueError, match="RefineOptions"):
        FrameSegmenter(net, 24, 40, refine=dict(radius=4))
    with pytest.raises(ValueError, match="not built"):
        ObjectSegmenter([net], 24, 40, refine=RefineOptions())
    assert FrameSegmenter.refine is None
