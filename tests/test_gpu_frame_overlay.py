"""Streaming inference on a real MI355X: ``ops.frame_prep`` and ``ops.overlay`` (csrc/stream.hip) against the numpy statement
of the arithmetic (util/frame_overlay.py) - bit for bit for the prep and the boolean modes, everywhere but within 1e-9 of a
rounding boundary for the soft ones - and against the reference's float32 form restated here; ``FrameSegmenter`` and
``run_webcam.main`` end to end."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frame_overlay_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = ["%dx%dx%d" % s for s in C.SHAPES]


def offset_view(t, elems=1):
    """The same values in a tensor whose base pointer lies `elems` elements (1 byte for uint8, 4 for fp32) behind an
    allocation's start."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    view = buf[elems:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elems * t.element_size()
    return view


def garbage(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=dtype, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def reference_f32(img, logits, mirror, boolean_mask, color, alpha):
    """src/run_webcam.py:81-133 in this file's own words: the sigmoid in float32, the mask where it is >= 0.5, the blend in
    float64, values above 255 set to 255, cast to bytes."""
    if mirror:
        img = img[:, ::-1]
    p = 1 / (1 + np.exp(-logits))
    assert p.dtype == np.float32
    if boolean_mask:
        p = np.where(p >= 0.5, np.float32(1), np.float32(0))
    plane = np.zeros(img.shape, dtype=float)
    plane[..., {"r": 2, "g": 1, "b": 0}[color]] = 255
    out = img + alpha * plane * p[..., np.newaxis]
    out[out > 255] = 255
    return out.astype("uint8")


# ------------------------------------------------------------------------------------------ frame_prep
@pytest.mark.parametrize("shape", C.SHAPES, ids=IDS)
def test_frame_prep_is_prepare_frame(shape):
    from fosvos_hip import ops
    n, h, w = shape
    f = C.frames(n, h, w)
    fd = torch.from_numpy(f).to(DEV)
    for mirror in (False, True):
        want = np.concatenate([F.prepare_frame(f[k], mirror) for k in range(n)])
        out = garbage((n, 3, h, w), torch.float32)
        assert ops.frame_prep(fd, mirror, out=out) is out
        got = out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (shape, mirror, int((got != want).sum()))
        again = ops.frame_prep(fd, mirror)
        assert torch.equal(again, out)
        # base pointers off every boundary: the frames by one byte, the image by one float
        out2 = offset_view(garbage((n, 3, h, w), torch.float32))
        ops.frame_prep(offset_view(fd), mirror, out=out2)
        assert out2.cpu().numpy().tobytes() == want.tobytes(), (shape, mirror, "offset")


# ------------------------------------------------------------------------------------------ overlay, boolean
@pytest.mark.parametrize("shape", C.SHAPES, ids=IDS)
def test_boolean_overlay_is_exact(shape):
    from fosvos_hip import ops
    n, h, w = shape
    f, x = C.frames(n, h, w), C.logits(n, h, w)
    fd, xd = torch.from_numpy(f).to(DEV), torch.from_numpy(x).to(DEV)
    fo, xo = offset_view(fd), offset_view(xd)
    for mirror in (False, True):
        src = f[:, :, ::-1] if mirror else f
        for color in C.COLORS:
            c = F.COLOR_CHANNEL[color]
            for alpha in C.ALPHAS:
                want = np.stack([F.overlay(f[k], x[k, 0], mirror, True, color, alpha) for k in range(n)])
                out = garbage((n, h, w, 3), torch.uint8)
                assert ops.overlay(fd, xd, mirror, True, color, alpha, out=out) is out
                got = out.cpu().numpy()
                assert np.array_equal(got, want), (shape, mirror, color, alpha, int((got != want).sum()))
                others = [k for k in range(3) if k != c]
                assert np.array_equal(got[..., others], src[..., others])  # untouched channels: the (mirrored) input
                # the reference's float32 form agrees everywhere (the generator leaves a gap around zero)
                ref = np.stack([reference_f32(f[k], x[k, 0], mirror, True, color, alpha) for k in range(n)])
                assert np.array_equal(got, ref), (shape, mirror, color, alpha)
        out = offset_view(garbage((n, h, w, 3), torch.uint8))
        ops.overlay(fo, xo, mirror, True, "g", 0.5, out=out)
        want = np.stack([F.overlay(f[k], x[k, 0], mirror, True, "g", 0.5) for k in range(n)])
        assert np.array_equal(out.cpu().numpy(), want), (shape, mirror, "offset")
    # the mask bytes (nothing to mirror: the logits are in output order)
    want = np.stack([F.mask_bytes(x[k, 0], True) for k in range(n)])
    for mirror in (False, True):
        out = garbage((n, h, w), torch.uint8)
        assert ops.overlay(fd, xd, mirror, True, overlay=False, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want), (shape, mirror)
    out = offset_view(garbage((n, h, w), torch.uint8))
    ops.overlay(fo, xo, True, True, overlay=False, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert set(np.unique(want).tolist()) == {0, 255}
    assert np.array_equal(want == 255, x[:, 0] >= 0) and (want[(x[:, 0] == 0)] == 255).all()  # both zeros are object


# ------------------------------------------------------------------------------------------ overlay, soft
@pytest.mark.parametrize("shape", C.SHAPES, ids=IDS)
def test_soft_overlay_outside_the_rounding_band(shape):
    from fosvos_hip import ops
    n, h, w = shape
    f, x = C.frames(n, h, w), C.logits(n, h, w, zeros=False)
    fd, xd = torch.from_numpy(f).to(DEV), torch.from_numpy(x).to(DEV)
    n_band = n_all = 0

    def compare(got, want, band, ref, what):
        nonlocal n_band, n_all
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print(what, "band pixels", int(band.sum()), "differing", int((diff != 0).sum()))
        assert not (diff != 0)[~band].any(), (what, int((diff != 0)[~band].sum()))
        assert diff.max() <= 1, what
        assert np.abs(got.astype(np.int32) - ref.astype(np.int32)).max() <= 1, what  # the float32 form: within one level
        n_band += int(band.sum())
        n_all += band.size

    for mirror in (False, True):
        for color in C.COLORS:
            c = F.COLOR_CHANNEL[color]
            for alpha in C.SOFT_ALPHAS:
                want = np.stack([F.overlay(f[k], x[k, 0], mirror, False, color, alpha) for k in range(n)])
                band = np.stack([C.soft_band(f[k], x[k, 0], mirror, True, color, alpha) for k in range(n)])
                ref = np.stack([reference_f32(f[k], x[k, 0], mirror, False, color, alpha) for k in range(n)])
                out = garbage((n, h, w, 3), torch.uint8)
                got = ops.overlay(fd, xd, mirror, False, color, alpha, out=out).cpu().numpy()
                others = [k for k in range(3) if k != c]
                assert np.array_equal(got[..., others], want[..., others])
                compare(got[..., c], want[..., c], band, ref[..., c], (shape, mirror, color, alpha))
        # alpha 0 adds an exact zero: no exclusion
        got = ops.overlay(fd, xd, mirror, False, "r", 0.0).cpu().numpy()
        assert np.array_equal(got, f[:, :, ::-1] if mirror else f)
    want = np.stack([F.mask_bytes(x[k, 0], False) for k in range(n)])
    band = np.stack([C.soft_band(f[k], x[k, 0], False, False, "r", 1.0) for k in range(n)])
    p32 = 1 / (1 + np.exp(-x[:, 0]))
    ref = (255 * p32.astype(np.float64) + 0.5).astype(np.uint8)
    out = offset_view(garbage((n, h, w), torch.uint8))
    got = ops.overlay(offset_view(fd), offset_view(xd), True, False, overlay=False, out=out).cpu().numpy()
    compare(got, want, band, ref, (shape, "mask"))
    assert n_band <= C.BAND_SHARE * n_all, (n_band, n_all)


# ------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    n, h, w = 2, 33, 47
    f = torch.from_numpy(C.frames(n, h, w)).to(DEV)
    x = torch.from_numpy(C.logits(n, h, w)).to(DEV)
    out = torch.full((n, h, w, 3), 7, dtype=torch.uint8, device=DEV)
    img = torch.full((n, 3, h, w), 7.0, device=DEV)
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    mean = ops._mean_bgr()
    with LaunchProfile(0) as prof:
        for bad in (lambda: ops.frame_prep(f.float()), lambda: ops.frame_prep(f[:, :, :, :2]), lambda: ops.frame_prep(f[0]),
                    lambda: ops.frame_prep(f, out=img[:, :2]), lambda: ops.frame_prep(f, out=img.double()),
                    lambda: ops.frame_prep(f[:0]),                                     # N = 0
                    lambda: ops.overlay(f.int(), x), lambda: ops.overlay(f, x.double()), lambda: ops.overlay(f, x.half()),
                    lambda: ops.overlay(f, x[:, :, :, :46]), lambda: ops.overlay(f, x[:1]), lambda: ops.overlay(f, x[:, 0]),
                    lambda: ops.overlay(f, x, alpha=-0.5), lambda: ops.overlay(f, x, alpha=float("nan")),
                    lambda: ops.overlay(f, x, alpha=float("inf")), lambda: ops.overlay(f, x, color="x"),
                    lambda: ops.overlay(f, x, out=out[:, :, :, :2]), lambda: ops.overlay(f, x, overlay=False, out=out),
                    lambda: ops.overlay(f[:0], x[:0])):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.frame_prep(f.cpu()), lambda: ops.frame_prep(f, out=img.cpu()),
                    lambda: ops.overlay(f.cpu(), x), lambda: ops.overlay(f, x.cpu()), lambda: ops.overlay(f, x, out=out.cpu())):
            with pytest.raises(RuntimeError):
                bad()

        # straight through the C ABI: the library's error codes, never a fault
        def ov(fr=f.data_ptr(), lg=x.data_ptr(), n_=n, h_=h, w_=w, mode=0, ch=2, alpha=1.0, o=out.data_ptr()):
            return L.fosvos_overlay(fr, lg, n_, h_, w_, 1, mode, ch, alpha, o, 0, st)

        assert ov(ch=3) == -2 and b"channel" in L.fosvos_last_error()
        assert ov(ch=-1) == -2 and ov(mode=4) == -2 and ov(mode=-1) == -2
        assert ov(alpha=-1.0) == -2 and ov(alpha=float("nan")) == -2 and ov(alpha=float("inf")) == -2
        assert ov(fr=None) == -2 and ov(lg=None) == -2 and ov(o=None) == -2
        assert ov(n_=0) == -1 and ov(h_=0) == -1 and ov(w_=-3) == -1
        assert ov(lg=x.data_ptr() + 2) == -2  # logits off their own alignment
        assert L.fosvos_frame_prep(None, n, h, w, 0, mean, img.data_ptr(), 0, st) == -2
        assert L.fosvos_frame_prep(f.data_ptr(), n, h, w, 0, None, img.data_ptr(), 0, st) == -2
        assert L.fosvos_frame_prep(f.data_ptr(), n, h, w, 0, mean, None, 0, st) == -2
        assert L.fosvos_frame_prep(f.data_ptr(), 0, h, w, 0, mean, img.data_ptr(), 0, st) == -1
        assert L.fosvos_frame_prep(f.data_ptr(), n, h, 0, 1, mean, img.data_ptr(), 0, st) == -1
    assert "k_frame_prep" not in prof.records and "k_overlay" not in prof.records, prof.records
    torch.cuda.synchronize()
    assert (out == 7).all() and (img == 7.0).all()  # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        ops.frame_prep(f, True, out=img)
        ops.overlay(f, x, True, out=out)
        assert ov(fr=None, mode=2, o=out.data_ptr()) == 0  # the mask modes do not read the frames
    assert prof.records["k_frame_prep"]["launches"] == 1 and prof.records["k_overlay"]["launches"] == 2


def test_ops_run_on_the_callers_stream_and_repeat():
    from fosvos_hip import ops
    n, h, w = 3, 48, 86
    f = torch.from_numpy(C.frames(n, h, w)).to(DEV)
    x = torch.from_numpy(C.logits(n, h, w, zeros=False)).to(DEV)
    first = [ops.frame_prep(f, True), ops.overlay(f, x, True, False, "b", 0.5), ops.overlay(f, x, True, False, overlay=False)]
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        second = [ops.frame_prep(f, True), ops.overlay(f, x, True, False, "b", 0.5),
                  ops.overlay(f, x, True, False, overlay=False)]
    side.synchronize()
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------ FrameSegmenter
_NETS = {}


def small_net(kind):
    """Seeded nets, built once: the small-weight VGG of the oracle, a thin ResNet-18."""
    if kind not in _NETS:
        if kind == "vgg":
            from networks.osvos_vgg import OSVOS_VGG
            net = OSVOS_VGG(pretrained=0)
            net.load_state_dict(O.make_state_dict(2))
            size = (48, 86)
        else:
            from networks.osvos_resnet import OSVOS_RESNET
            torch.manual_seed(7)
            net = OSVOS_RESNET(pretrained=False, version=18, scale_down_exponent=3)
            size = (64, 96)
        _NETS[kind] = (net.to(DEV).eval(), size)
    return _NETS[kind]


def camera_frames(count, h, w, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def expected(net, frame, mirror=True, overlay=True, boolean_mask=True, color="r", alpha=1.0):
    with torch.no_grad():
        logits = net.forward(torch.from_numpy(F.prepare_frame(frame, mirror)).to(DEV))[-1]
    return F.apply(frame, logits[0, 0].cpu().numpy(), mirror, overlay, boolean_mask, color, alpha), logits[0, 0].cpu().numpy()


@pytest.mark.parametrize("kind", ["vgg", "resnet"])
def test_segmenter_apply_is_the_definition(kind):
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_net(kind)
    frames = camera_frames(2, h, w)
    assert net.compute_side_outputs is True
    with FrameSegmenter(net, h, w) as seg:  # defaults: mirror, boolean overlay, red, alpha 1
        for frame in frames:
            want, logits = expected(net, frame)
            got = seg.apply(frame)
            assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got, want)
            print(kind, "object share of the mask: %.3f" % float((logits >= 0).mean()))
        assert net.compute_side_outputs is True  # restored
    with FrameSegmenter(net, h, w, depth=1, mirror=False, overlay=True, boolean_mask=True, color="g", alpha=0.5) as seg:
        want, _ = expected(net, frames[0], False, True, True, "g", 0.5)
        assert np.array_equal(seg.apply(frames[0]), want)
    with FrameSegmenter(net, h, w, overlay=False) as seg:
        want, _ = expected(net, frames[1], True, False)
        got = seg.apply(frames[1])
        assert got.shape == (h, w) and np.array_equal(got, want)
    with FrameSegmenter(net, h, w, mirror=False, boolean_mask=False, color="b", alpha=0.5) as seg:
        want, logits = expected(net, frames[1], False, True, False, "b", 0.5)
        got = seg.apply(frames[1])
        band = C.soft_band(frames[1], logits, False, True, "b", 0.5)
        assert np.array_equal(got[..., 1:], want[..., 1:]) and np.array_equal(got[..., 0][~band], want[..., 0][~band])
    net.compute_side_outputs = False
    try:
        with FrameSegmenter(net, h, w) as seg:
            seg.apply(frames[0])
        assert net.compute_side_outputs is False
    finally:
        net.compute_side_outputs = True


def test_segmenter_keeps_order_and_reuses_slots_cleanly():
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_net("vgg")
    frames = camera_frames(7, h, w, seed=11)
    with FrameSegmenter(net, h, w, depth=1) as seg:
        singles = [seg.apply(f) for f in frames]
    assert len({s.tobytes() for s in singles}) == 7  # seven different outputs: a swapped pair would show
    for depth in (1, 2, 3):
        with FrameSegmenter(net, h, w, depth=depth) as seg:
            first = list(seg.segment(iter(frames)))
            second = list(seg.segment(frames))
            assert len(first) == len(second) == 7
            for k in range(7):
                assert np.array_equal(first[k], singles[k]) and np.array_equal(second[k], singles[k]), (depth, k)
            # the arrays are the caller's own
            keep = first[1].copy()
            first[0][...] = 0
            third = list(seg.segment(frames[:3]))
            third[2][...] = 0
            assert np.array_equal(first[1], keep) and np.array_equal(third[1], singles[1])
            # submit / result by hand, more frames than slots before the first result
            for f in frames[:depth + 2]:
                seg.submit(f)
            assert seg.pending == depth + 2
            for k in range(depth + 2):
                assert np.array_equal(seg.result(), singles[k]), (depth, k)
            with pytest.raises(RuntimeError):
                seg.result()


def test_segmenter_refuses_bad_frames_before_queueing():
    from fosvos_hip import LaunchProfile
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_net("vgg")
    good = camera_frames(1, h, w, seed=5)[0]
    with FrameSegmenter(net, h, w, depth=2) as seg:
        want = seg.apply(good)
        with LaunchProfile(0) as prof:
            for bad in (good[:, :-1], good[:-1], good[:, :, :2], good.astype(np.float32), good.astype(np.int8), good.tolist(),
                        torch.from_numpy(good)):
                with pytest.raises(ValueError):
                    seg.submit(bad)
            assert seg.pending == 0
        assert not prof.records, prof.records  # nothing was queued
        assert np.array_equal(seg.apply(good), want)
        # a failing net leaves the segmenter usable
        forward = net.forward
        net.forward = lambda x: (_ for _ in ()).throw(KeyError("no such layer"))
        try:
            with pytest.raises(KeyError):
                seg.submit(good)
        finally:
            del net.forward
        assert net.forward == forward and seg.pending == 0 and net.compute_side_outputs is True
        assert np.array_equal(seg.apply(good), want)
        seg.submit(good)
        with pytest.raises(RuntimeError):
            seg.apply(good)  # a frame is in flight
        assert np.array_equal(seg.result(), want)
    with pytest.raises(RuntimeError):
        seg.submit(good)  # closed
    for bad in (dict(color="x"), dict(alpha=-1.0), dict(alpha=float("nan")), dict(depth=0)):
        with pytest.raises(ValueError):
            FrameSegmenter(net, h, w, **bad)
    from networks.osvos_vgg import OSVOS_VGG
    with pytest.raises(RuntimeError, match="GPU"):
        FrameSegmenter(OSVOS_VGG(pretrained=0), h, w)


# ------------------------------------------------------------------------------------------ run_webcam
def test_run_webcam_main(tmp_path):
    import run_webcam
    net, (h, w) = small_net("vgg")
    ckpt = tmp_path / "vgg.pth"
    torch.save(O.make_state_dict(2), str(ckpt))
    common = ["--variant", "vgg", "--model", str(ckpt), "--synthetic", "4", "--height", str(h), "--width", str(w)]
    frames = [run_webcam.synthetic_frame(h, w, k) for k in range(4)]
    names = ["%05d.png" % k for k in range(4)]

    rates = run_webcam.main(common + ["--output", str(tmp_path / "overlay")])
    assert len(rates) == 4 and sorted(os.listdir(tmp_path / "overlay")) == names
    for k, name in enumerate(names):
        want, _ = expected(net, frames[k])  # the defaults: mirrored, boolean mask, red, alpha 1
        got = np.asarray(Image.open(str(tmp_path / "overlay" / name)))
        assert got.shape == (h, w, 3) and np.array_equal(got, want[:, :, ::-1])  # written as RGB

    run_webcam.main(common + ["--no-overlay", "--no-mirror", "--output", str(tmp_path / "mask")])
    assert sorted(os.listdir(tmp_path / "mask")) == names
    for k, name in enumerate(names):
        want, _ = expected(net, frames[k], False, False)
        im = Image.open(str(tmp_path / "mask" / name))
        assert im.mode == "L" and np.array_equal(np.asarray(im), want)

    run_webcam.main(common + ["--no-network", "--output", str(tmp_path / "plain")])
    for k, name in enumerate(names):
        got = np.asarray(Image.open(str(tmp_path / "plain" / name)))
        assert np.array_equal(got, frames[k][:, ::-1, ::-1])  # the mirrored input
