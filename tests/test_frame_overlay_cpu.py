"""The per-frame arithmetic of streaming inference as util/frame_overlay.py states it (known answers worked out by hand), the
seeded inputs the GPU test compares the kernels on, and the options of run_webcam.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_overlay_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402

# 2 x 3 frame, BGR; bytes 0, 200 and 255 in every channel
IMG = np.array([[[0, 200, 255], [255, 0, 200], [200, 255, 0]],
                [[200, 200, 200], [0, 0, 0], [255, 255, 255]]], dtype=np.uint8)
LOGITS = np.array([[-1.0, -0.0, 0.0], [3.0, -1.0, 3.0]], dtype=np.float32)
MASK = np.array([[0, 1, 1], [1, 0, 1]])  # logit >= 0: both zeros are object


def test_prepare_frame_known_answers():
    from dataloaders.davis_2016 import MEANVAL
    assert F.MEANVAL is MEANVAL  # the one constant
    x = F.prepare_frame(IMG)
    assert x.dtype == np.float32 and x.shape == (1, 3, 2, 3) and x.flags.c_contiguous
    m = [np.float32(v) for v in MEANVAL]
    assert x[0, 0].tolist() == [[np.float32(0) - m[0], np.float32(255) - m[0], np.float32(200) - m[0]],
                                [np.float32(200) - m[0], np.float32(0) - m[0], np.float32(255) - m[0]]]
    assert x[0, 2, 0].tolist() == [np.float32(255) - m[2], np.float32(200) - m[2], np.float32(0) - m[2]]
    assert x[0, 1, 0, 0] == np.float32(200) - np.float32(116.66877)
    xm = F.prepare_frame(IMG, mirror=True)
    assert np.array_equal(xm, x[:, :, :, ::-1]) and xm.flags.c_contiguous
    assert xm[0, 0, 0].tolist() == [np.float32(200) - m[0], np.float32(255) - m[0], np.float32(0) - m[0]]


def test_prediction_known_answers():
    assert F.prediction(LOGITS, True).tolist() == MASK.astype(np.float64).tolist()
    p = F.prediction(LOGITS, False)
    assert p.dtype == np.float64
    assert p[0, 1] == 0.5 and p[0, 2] == 0.5
    assert abs(p[0, 0] - 0.2689414213699951) < 1e-15 and abs(p[1, 0] - 0.9525741268224334) < 1e-15


@pytest.mark.parametrize("color", C.COLORS)
def test_boolean_overlay_known_answers(color):
    c = {"b": 0, "g": 1, "r": 2}[color]
    # alpha -> what is added where the mask is set, then the clamp
    for alpha, add in ((0.0, 0.0), (0.5, 127.5), (1.0, 255.0), (2.0, 510.0)):
        for mirror in (False, True):
            img = IMG[:, ::-1] if mirror else IMG
            want = img.copy()
            for y in range(2):
                for x in range(3):
                    want[y, x, c] = int(min(int(img[y, x, c]) + add * MASK[y, x], 255.0))  # int(): towards zero
            got = F.overlay(IMG, LOGITS, mirror, True, color, alpha)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (color, alpha, mirror)
    # spelled out: red, alpha 0.5, not mirrored
    got = F.overlay(IMG, LOGITS, False, True, "r", 0.5)[:, :, 2]
    assert got.tolist() == [[255, 255, 127], [255, 0, 255]]     # 255 | 200 + 127.5 -> 255 | 0 + 127.5 -> 127 ; 327 -> 255 | 0 | 255
    got = F.overlay(IMG, LOGITS, True, True, "b", 0.5)[:, :, 0]
    assert got.tolist() == [[200, 255, 127], [255, 0, 255]]     # mirrored blue 200 255 0 / 255 0 200, mask 0 1 1 / 1 0 1
    # alpha * 255 >= 255: the byte, or 255
    for alpha in (1.0, 2.0, 1e300):
        got = F.overlay(IMG, LOGITS, False, True, "g", alpha)
        assert np.array_equal(got[:, :, 1], np.where(MASK == 1, 255, IMG[:, :, 1]))
        assert np.array_equal(got[:, :, [0, 2]], IMG[:, :, [0, 2]])


def test_soft_overlay_and_mask_known_answers():
    p = [[0.2689414213699951, 0.5, 0.5], [0.9525741268224334, 0.2689414213699951, 0.9525741268224334]]
    got = F.overlay(IMG, LOGITS, False, False, "r", 1.0)
    # 255 + 68.58 -> 255 | 200 + 127.5 -> 255 | 0 + 127.5 -> 127 ; 200 + 242.9 -> 255 | 0 + 68.58 -> 68 | 255
    assert got[:, :, 2].tolist() == [[255, 255, 127], [255, 68, 255]]
    assert np.array_equal(got[:, :, :2], IMG[:, :, :2])
    got = F.overlay(IMG, LOGITS, False, False, "b", 0.5)
    # 0 + 34.29 -> 34 | 255 | 200 + 63.75 -> 255 ; 200 + 121.45 -> 255 | 0 + 34.29 -> 34 | 255
    assert got[:, :, 0].tolist() == [[34, 255, 255], [255, 34, 255]]
    assert F.overlay(IMG, LOGITS, False, False, "g", 0.0).tolist() == IMG.tolist()
    assert F.mask_bytes(LOGITS, True).tolist() == [[0, 255, 255], [255, 0, 255]]
    # 255 p + 0.5: 69.08 | 128.0 | 128.0 ; 243.4 | 69.08 | 243.4
    assert F.mask_bytes(LOGITS, False).tolist() == [[69, 128, 128], [243, 69, 243]]
    assert [[int(255 * v + 0.5) for v in row] for row in p] == F.mask_bytes(LOGITS, False).tolist()
    assert F.apply(IMG, LOGITS, True, False, False).tolist() == F.mask_bytes(LOGITS, False).tolist()  # a mask has no mirror
    assert F.apply(IMG, LOGITS, True, True, True, "g", 0.5).tolist() == F.overlay(IMG, LOGITS, True, True, "g", 0.5).tolist()


def test_bad_arguments_raise():
    for alpha in (-0.1, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            F.overlay(IMG, LOGITS, alpha=alpha)
        with pytest.raises(ValueError):
            F.apply(IMG, LOGITS, overlay_on=False, alpha=alpha)
    for color in ("x", "R", 2, None):
        with pytest.raises(ValueError):
            F.overlay(IMG, LOGITS, color=color)
    with pytest.raises(ValueError):
        F.overlay(IMG, LOGITS[:, :2])                 # logits of another shape
    with pytest.raises(ValueError):
        F.overlay(IMG, LOGITS.astype(np.float64))
    with pytest.raises(ValueError):
        F.overlay(IMG[:, :, :2], LOGITS)              # not three channels
    with pytest.raises(ValueError):
        F.prepare_frame(IMG.astype(np.float32))
    with pytest.raises(ValueError):
        F.prepare_frame(IMG[0])
    with pytest.raises(ValueError):
        F.mask_bytes(LOGITS[np.newaxis])


def test_seeded_inputs_of_the_gpu_test():
    """What tests/test_gpu_frame_overlay.py relies on: the logit generator leaves a gap around zero (so the reference's
    float32 ``sigmoid >= 0.5`` and ``logit >= 0`` agree everywhere), plants both zeros, and the pixels the soft comparison
    has to exclude are at most 1e-4 of all."""
    n_band = n_all = 0
    for n, h, w in C.SHAPES:
        x = C.logits(n, h, w)
        assert x.dtype == np.float32 and not ((np.abs(x) < 1e-6) & (x != 0)).any()
        assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
        assert (x > 0).any() and (x < 0).any()
        f = C.frames(n, h, w)
        assert (f == 0).any() and (f == 255).any()
        soft = C.logits(n, h, w, zeros=False)
        assert not (soft == 0).any() and not ((np.abs(soft) < 1e-6)).any()
        for k in range(n):
            for mirror in (False, True):
                for alpha in C.SOFT_ALPHAS:
                    for color in C.COLORS:
                        n_band += int(C.soft_band(f[k], soft[k, 0], mirror, True, color, alpha).sum())
                        n_all += h * w
            n_band += int(C.soft_band(f[k], soft[k, 0], False, False, "r", 1.0).sum())
            n_all += h * w
    assert n_band <= C.BAND_SHARE * n_all, (n_band, n_all)


def test_run_webcam_options_match_the_reference():
    import run_webcam
    a = run_webcam.build_parser().parse_args([])
    # src/run_webcam.py:19-29
    assert (a.variant, a.version, a.webcam, a.mirror, a.use_network, a.use_cuda, a.overlay, a.boolean_mask, a.overlay_color,
            a.overlay_alpha) == ("resnet", None, 0, True, True, True, True, True, "r", 1.0)
    assert (a.model, a.source, a.synthetic, a.output, a.depth) == (None, None, None, None, 2)
    a = run_webcam.build_parser().parse_args(["--variant", "prune", "--version", "3", "--webcam", "1", "--no-mirror",
                                              "--no-network", "--no-overlay", "--no-boolean-mask", "--overlay-color", "g",
                                              "--overlay-alpha", "0.25"])
    assert (a.variant, a.version, a.webcam, a.mirror, a.use_network, a.overlay, a.boolean_mask, a.overlay_color,
            a.overlay_alpha) == ("prune", 3, 1, False, False, False, False, "g", 0.25)
    b = run_webcam.build_parser().parse_args(["-var", "prune", "-ver", "3", "-wc", "1", "-nm", "-nn", "-no", "-nbm", "-oc", "g",
                                              "-oa", "0.25"])
    assert vars(a) == vars(b)
    c = run_webcam.build_parser().parse_args(["--no-mirror", "--mirror", "-nn", "--use-network", "-no", "-o", "-nbm", "-bm"])
    assert c.mirror and c.use_network and c.overlay and c.boolean_mask
    for bad in (["--variant", "alexnet"], ["--overlay-color", "x"], ["--overlay-alpha", "much"], ["--version", "x"]):
        with pytest.raises(SystemExit):
            run_webcam.build_parser().parse_args(bad)
    # the reference's file names
    assert run_webcam.model_file_name("vgg", None) == "vgg16.pth"
    assert [run_webcam.model_file_name("resnet", v) for v in (None, 18, 34, 50)] == ["resnet18.pth", "resnet18.pth",
                                                                                    "resnet34.pth", "resnet18.pth"]
    assert run_webcam.model_file_name("prune", 7) == "prune_64_1_7.pth"


def test_run_webcam_mimic_and_missing_cv2_raise():
    import run_webcam
    with pytest.raises(Exception, match="Not yet implemented"):
        run_webcam.get_network("mimic", None)
    with pytest.raises(Exception, match="Not yet implemented"):
        run_webcam.main(["--variant", "mimic", "--synthetic", "1"])
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="--source"):
            run_webcam.main(["--webcam", "0", "--no-network"])
        with pytest.raises(RuntimeError, match="--source"):
            run_webcam.open_webcam(0)
    with pytest.raises(RuntimeError, match="no CPU"):
        run_webcam.main(["--no-cuda", "--synthetic", "1"])


def test_run_webcam_passes_frames_through_without_a_network(tmp_path):
    """--no-network: only the mirror is applied (src/run_webcam.py:71-75); files come out in order, BGR written as RGB."""
    import run_webcam
    from PIL import Image
    rates = run_webcam.main(["--no-network", "--synthetic", "3", "--height", "10", "--width", "14", "--output", str(tmp_path)])
    assert len(rates) == 3 and sorted(os.listdir(tmp_path)) == ["%05d.png" % k for k in range(3)]
    for k in range(3):
        frame = run_webcam.synthetic_frame(10, 14, k)
        assert frame.dtype == np.uint8 and frame.shape == (10, 14, 3)
        got = np.asarray(Image.open(str(tmp_path / ("%05d.png" % k))))
        assert np.array_equal(got, frame[:, ::-1, ::-1])
    # the frames are read back from files the same way
    src = tmp_path / "src"
    src.mkdir()
    for k in (1, 0):
        Image.fromarray(run_webcam.synthetic_frame(10, 14, k)[:, :, ::-1].copy()).save(str(src / ("f%d.png" % k)))
    out = tmp_path / "out"
    run_webcam.main(["--no-network", "--no-mirror", "--source", str(src), "--output", str(out)])
    for k in range(2):
        got = np.asarray(Image.open(str(out / ("%05d.png" % k))))
        assert np.array_equal(got, run_webcam.synthetic_frame(10, 14, k)[:, :, ::-1])
