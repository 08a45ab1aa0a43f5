"""Streaming inference with the net at a size of its own, on a real MI355X: ``ops.frame_prep(net_size=)`` and
``ops.overlay(net_size=)`` (csrc/stream.hip: k_frame_prep_scaled, k_overlay_scaled) against the numpy statement of the
arithmetic (util/frame_resample.py) - bit for bit for the prep and the boolean modes, everywhere but within 1e-9 of a rounding
boundary for the soft ones; ``FrameSegmenter(net_size=)`` and ``run_webcam.main --net-height --net-width`` end to end."""
import io
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

import frame_resample_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def offset_view(t, elems=1):
    """The same values in a tensor whose base pointer lies `elems` elements behind an allocation's start."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    view = buf[elems:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elems * t.element_size()
    return view


def garbage(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=dtype, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------ frame_prep
@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_scaled_frame_prep_is_prepare_frame_scaled(case):
    from fosvos_hip import ops
    n, hf, wf, hn, wn = case
    f = C.frames(n, hf, wf)
    fd = torch.from_numpy(f).to(DEV)
    for mirror in (False, True):
        want = np.concatenate([R.prepare_frame_scaled(f[k], hn, wn, mirror) for k in range(n)])
        out = garbage((n, 3, hn, wn), torch.float32)
        assert ops.frame_prep(fd, mirror, out=out, net_size=(hn, wn)) is out
        got = out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (case, mirror, int((got != want).sum()))
        again = ops.frame_prep(fd, mirror, net_size=(hn, wn))
        assert again.shape == (n, 3, hn, wn) and torch.equal(again, out)
        # base pointers off every boundary: the frames by one byte, the image by one float
        out2 = offset_view(garbage((n, 3, hn, wn), torch.float32))
        ops.frame_prep(offset_view(fd), mirror, out=out2, net_size=(hn, wn))
        assert out2.cpu().numpy().tobytes() == want.tobytes(), (case, mirror, "offset")


def test_scaled_frame_prep_sums_past_32_bits():
    """255 Hf Wf passes 2^32 from 4097 x 4097 on: a bright frame of 4200 x 4100 down to 1 x 2 (the whole frame is the window of
    two pixels) and, mirrored, to 3 x 5.  The expected sums are taken here with float64 matrix products of the weights - exact,
    every partial sum is an integer below 2^53 - not with the definition's code."""
    from fosvos_hip import ops
    hf, wf = 4200, 4100
    f = np.random.default_rng(42).integers(250, 256, (1, hf, wf, 3), dtype=np.uint8)
    fd = torch.from_numpy(f).to(DEV)
    planes = [f[0, :, :, c].astype(np.float64) for c in range(3)]
    mean = np.array(F.MEANVAL, dtype=np.float32)
    for (hn, wn), mirror in (((1, 2), False), ((3, 5), True)):
        wy, wx = R.box_weights(hf, hn).astype(np.float64), R.box_weights(wf, wn).astype(np.float64)
        s = np.stack([wy @ p @ wx.T for p in planes])  # [3,Hn,Wn]
        assert s.min() > 2 ** 32 and s.max() < 2 ** 53
        want = (s / np.float64(hf * wf)).astype(np.float32) - mean[:, None, None]
        if mirror:
            want = np.ascontiguousarray(want[:, :, ::-1])
        got = ops.frame_prep(fd, mirror, net_size=(hn, wn)).cpu().numpy()
        assert got.shape == (1, 3, hn, wn) and got[0].tobytes() == want.tobytes(), ((hn, wn), got, want)


# ------------------------------------------------------------------------------------------ overlay, boolean
@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_scaled_boolean_overlay_is_exact(case):
    from fosvos_hip import ops
    n, hf, wf, hn, wn = case
    size = (hn, wn)
    f, x = C.frames(n, hf, wf), C.logits(n, hn, wn)
    fd, xd = torch.from_numpy(f).to(DEV), torch.from_numpy(x).to(DEV)
    fo, xo = offset_view(fd), offset_view(xd)
    for mirror in (False, True):
        src = f[:, :, ::-1] if mirror else f
        for color in C.COLORS:
            c = F.COLOR_CHANNEL[color]
            for alpha in C.ALPHAS:
                want = np.stack([R.overlay_scaled(f[k], x[k, 0], mirror, True, color, alpha) for k in range(n)])
                out = garbage((n, hf, wf, 3), torch.uint8)
                assert ops.overlay(fd, xd, mirror, True, color, alpha, out=out, net_size=size) is out
                got = out.cpu().numpy()
                assert np.array_equal(got, want), (case, mirror, color, alpha, int((got != want).sum()))
                others = [k for k in range(3) if k != c]
                assert np.array_equal(got[..., others], src[..., others])  # untouched channels: the (mirrored) input
        out = offset_view(garbage((n, hf, wf, 3), torch.uint8))
        ops.overlay(fo, xo, mirror, True, "g", 0.5, out=out, net_size=size)
        want = np.stack([R.overlay_scaled(f[k], x[k, 0], mirror, True, "g", 0.5) for k in range(n)])
        assert np.array_equal(out.cpu().numpy(), want), (case, mirror, "offset")
    # the mask bytes, at the frames' size (nothing to mirror: the logits are in output order)
    want = np.stack([R.mask_bytes_scaled(x[k, 0], hf, wf, True) for k in range(n)])
    for mirror in (False, True):
        out = garbage((n, hf, wf), torch.uint8)
        assert ops.overlay(fd, xd, mirror, True, overlay=False, out=out, net_size=size) is out
        assert np.array_equal(out.cpu().numpy(), want), (case, mirror)
    out = offset_view(garbage((n, hf, wf), torch.uint8))
    ops.overlay(fo, xo, True, True, overlay=False, out=out, net_size=size)
    assert np.array_equal(out.cpu().numpy(), want)
    v = np.stack([R.logits_up(x[k, 0], hf, wf) for k in range(n)])
    assert set(np.unique(want).tolist()) <= {0, 255} and np.array_equal(want == 255, v >= 0)
    assert (want[v == 0] == 255).all()  # both zeros are object


# ------------------------------------------------------------------------------------------ overlay, soft
def test_scaled_soft_overlay_outside_the_rounding_band():
    """Every case in one test: the band's share is taken over all of them."""
    from fosvos_hip import ops
    n_band = n_all = 0

    def compare(got, want, band, what):
        nonlocal n_band, n_all
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print(what, "band pixels", int(band.sum()), "differing", int((diff != 0).sum()))
        assert not (diff != 0)[~band].any(), (what, int((diff != 0)[~band].sum()))
        assert diff.max() <= 1, what
        n_band += int(band.sum())
        n_all += band.size

    for case in C.CASES:
        n, hf, wf, hn, wn = case
        size = (hn, wn)
        f, x = C.frames(n, hf, wf), C.logits(n, hn, wn, zeros=False)
        fd, xd = torch.from_numpy(f).to(DEV), torch.from_numpy(x).to(DEV)
        for mirror in (False, True):
            for color in C.COLORS:
                c = F.COLOR_CHANNEL[color]
                for alpha in C.SOFT_ALPHAS:
                    want = np.stack([R.overlay_scaled(f[k], x[k, 0], mirror, False, color, alpha) for k in range(n)])
                    band = np.stack([C.soft_band_scaled(f[k], x[k, 0], mirror, True, color, alpha) for k in range(n)])
                    out = garbage((n, hf, wf, 3), torch.uint8)
                    got = ops.overlay(fd, xd, mirror, False, color, alpha, out=out, net_size=size).cpu().numpy()
                    others = [k for k in range(3) if k != c]
                    assert np.array_equal(got[..., others], want[..., others])
                    compare(got[..., c], want[..., c], band, (case, mirror, color, alpha))
            # alpha 0 adds an exact zero: no exclusion
            got = ops.overlay(fd, xd, mirror, False, "r", 0.0, net_size=size).cpu().numpy()
            assert np.array_equal(got, f[:, :, ::-1] if mirror else f)
        want = np.stack([R.mask_bytes_scaled(x[k, 0], hf, wf, False) for k in range(n)])
        band = np.stack([C.soft_band_scaled(f[k], x[k, 0], False, False, "r", 1.0) for k in range(n)])
        out = offset_view(garbage((n, hf, wf), torch.uint8))
        got = ops.overlay(offset_view(fd), offset_view(xd), True, False, overlay=False, out=out, net_size=size).cpu().numpy()
        compare(got, want, band, (case, "mask"))
    print("band pixels", n_band, "of", n_all)
    assert n_band <= C.BAND_SHARE * n_all, (n_band, n_all)


# ------------------------------------------------------------------------------------------ arguments
def test_scaled_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    n, hf, wf, hn, wn = 2, 33, 47, 16, 20
    size = (hn, wn)
    f = torch.from_numpy(C.frames(n, hf, wf)).to(DEV)
    x = torch.from_numpy(C.logits(n, hn, wn)).to(DEV)
    xf = torch.from_numpy(C.logits(n, hf, wf)).to(DEV)
    out = torch.full((n, hf, wf, 3), 7, dtype=torch.uint8, device=DEV)
    img = torch.full((n, 3, hn, wn), 7.0, device=DEV)
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    mean = ops._mean_bgr()
    with LaunchProfile(0) as prof:
        for bad in (lambda: ops.frame_prep(f, net_size=(hf + 1, wn)), lambda: ops.frame_prep(f, net_size=(hn, wf + 1)),
                    lambda: ops.frame_prep(f, net_size=(0, wn)), lambda: ops.frame_prep(f, net_size=(hn, -1)),
                    lambda: ops.frame_prep(f, net_size=(hn,)), lambda: ops.frame_prep(f, net_size=16),
                    lambda: ops.frame_prep(f, net_size=(16.0, 20)), lambda: ops.frame_prep(f, net_size=(True, 20)),
                    lambda: ops.frame_prep(f, out=img[:, :, :, :19], net_size=size),       # a wrong out shape
                    lambda: ops.frame_prep(f, out=torch.empty((n, 3, hf, wf), device=DEV), net_size=size),
                    lambda: ops.frame_prep(f, out=img.double(), net_size=size),
                    lambda: ops.frame_prep(f[:0], net_size=size),                          # N = 0
                    lambda: ops.overlay(f, x, net_size=(hf + 1, wn)), lambda: ops.overlay(f, x, net_size=(hn, wf + 1)),
                    lambda: ops.overlay(f, xf, net_size=size),                             # logits not of net_size
                    lambda: ops.overlay(f, x[:, :, :, :19], net_size=size), lambda: ops.overlay(f, x[:1], net_size=size),
                    lambda: ops.overlay(f, x),                                             # scaling is never inferred
                    lambda: ops.overlay(f, x, net_size=(hf, wf)),
                    lambda: ops.overlay(f, x.double(), net_size=size),
                    lambda: ops.overlay(f, x, alpha=-0.5, net_size=size), lambda: ops.overlay(f, x, color="x", net_size=size),
                    lambda: ops.overlay(f, x, out=out[:, :, :, :2], net_size=size),
                    lambda: ops.overlay(f, x, overlay=False, out=out, net_size=size),
                    lambda: ops.overlay(f, x, overlay=False, out=torch.empty((n, hn, wn), dtype=torch.uint8, device=DEV),
                                        net_size=size),                                    # the mask keeps the frames' size
                    lambda: ops.overlay(f[:0], x[:0], net_size=size)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.frame_prep(f.cpu(), net_size=size), lambda: ops.overlay(f, x.cpu(), net_size=size),
                    lambda: ops.overlay(f, x, out=out.cpu(), net_size=size)):
            with pytest.raises(RuntimeError):
                bad()

        # straight through the C ABI: the library's error codes, never a fault
        def ov(fr=f.data_ptr(), lg=x.data_ptr(), n_=n, hf_=hf, wf_=wf, hn_=hn, wn_=wn, mode=0, ch=2, alpha=1.0,
               o=out.data_ptr()):
            return L.fosvos_overlay_scaled(fr, lg, n_, hf_, wf_, hn_, wn_, 1, mode, ch, alpha, o, 0, st)

        def fp(fr=f.data_ptr(), n_=n, hf_=hf, wf_=wf, hn_=hn, wn_=wn, m=mean, im=img.data_ptr()):
            return L.fosvos_frame_prep_scaled(fr, n_, hf_, wf_, hn_, wn_, 0, m, im, 0, st)

        assert ov(ch=3) == -2 and b"channel" in L.fosvos_last_error()
        assert ov(ch=-1) == -2 and ov(mode=4) == -2 and ov(mode=-1) == -2
        assert ov(alpha=-1.0) == -2 and ov(alpha=float("nan")) == -2 and ov(alpha=float("inf")) == -2
        assert ov(fr=None) == -2 and ov(lg=None) == -2 and ov(o=None) == -2
        assert ov(n_=0) == -1 and ov(hf_=0) == -1 and ov(wf_=-3) == -1 and ov(hn_=0) == -1 and ov(wn_=0) == -1
        assert ov(hn_=hf + 1) == -1 and b"exceeds" in L.fosvos_last_error()
        assert ov(wn_=wf + 1) == -1 and ov(hf_=8193) == -1 and ov(wf_=8193) == -1
        assert ov(lg=x.data_ptr() + 2) == -2  # logits off their own alignment
        assert fp(fr=None) == -2 and fp(m=None) == -2 and fp(im=None) == -2
        assert fp(n_=0) == -1 and fp(hf_=0) == -1 and fp(wf_=0) == -1 and fp(hn_=0) == -1 and fp(wn_=-2) == -1
        assert fp(hn_=hf + 1) == -1 and fp(wn_=wf + 1) == -1 and fp(hf_=8193) == -1 and fp(wf_=8193) == -1
        assert fp(im=img.data_ptr() + 2) == -2  # the image off its own alignment
    assert not prof.records, prof.records
    torch.cuda.synchronize()
    assert (out == 7).all() and (img == 7.0).all()  # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        ops.frame_prep(f, True, out=img, net_size=size)
        ops.overlay(f, x, True, out=out, net_size=size)
        assert ov(fr=None, mode=2, o=out.data_ptr()) == 0  # the mask modes do not read the frames
        full = torch.empty((n, 3, hf, wf), device=DEV)
        assert fp(hn_=hf, wn_=wf, im=full.data_ptr()) == 0  # equal sizes are in range
    assert prof.records["k_frame_prep_scaled"]["launches"] == 2 and prof.records["k_overlay_scaled"]["launches"] == 2
    assert "k_frame_prep" not in prof.records and "k_overlay" not in prof.records


def test_scaled_entries_at_equal_sizes_are_the_unscaled_ones():
    """The C entries take Hn = Hf, Wn = Wf (the Python face never sends it): windows of one pixel, the identity upsample."""
    from fosvos_hip import lib, ops
    n, h, w = 2, 33, 47
    f = torch.from_numpy(C.frames(n, h, w)).to(DEV)
    x = torch.from_numpy(C.logits(n, h, w)).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    img = garbage((n, 3, h, w), torch.float32)
    assert lib().fosvos_frame_prep_scaled(f.data_ptr(), n, h, w, h, w, 1, ops._mean_bgr(), img.data_ptr(), 0, st) == 0
    assert torch.equal(img, ops.frame_prep(f, True))
    out = garbage((n, h, w, 3), torch.uint8)
    assert lib().fosvos_overlay_scaled(f.data_ptr(), x.data_ptr(), n, h, w, h, w, 1, 0, 1, 0.5, out.data_ptr(), 0, st) == 0
    assert torch.equal(out, ops.overlay(f, x, True, True, "g", 0.5))


# ------------------------------------------------------------------------------------------ FrameSegmenter
_NETS = {}


def small_net(kind):
    """Seeded nets, built once: the small-weight VGG of the oracle, a thin ResNet-18; with the size each runs at."""
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


def expected(net, size, frame, mirror=True, overlay=True, boolean_mask=True, color="r", alpha=1.0):
    with torch.no_grad():
        logits = net.forward(torch.from_numpy(R.prepare_frame_scaled(frame, size[0], size[1], mirror)).to(DEV))[-1]
    logits = logits[0, 0].cpu().numpy()
    assert logits.shape == tuple(size)
    return R.apply_scaled(frame, logits, mirror, overlay, boolean_mask, color, alpha), logits


@pytest.mark.parametrize("kind,hf,wf", [("vgg", 96, 172), ("vgg", 61, 107), ("resnet", 80, 141)])
def test_scaled_segmenter_apply_is_the_definition(kind, hf, wf):
    from fosvos_hip.stream import FrameSegmenter
    net, size = small_net(kind)
    frames = camera_frames(2, hf, wf)
    with FrameSegmenter(net, hf, wf, net_size=size) as seg:  # defaults: mirror, boolean overlay, red, alpha 1
        assert seg.net_size == size
        for frame in frames:
            want, logits = expected(net, size, frame)
            got = seg.apply(frame)
            assert got.dtype == np.uint8 and got.shape == (hf, wf, 3) and np.array_equal(got, want)
            print(kind, "object share of the mask: %.3f" % float((R.logits_up(logits, hf, wf) >= 0).mean()))
        assert net.compute_side_outputs is True  # restored
    with FrameSegmenter(net, hf, wf, depth=1, mirror=False, color="g", alpha=0.5, net_size=size) as seg:
        want, _ = expected(net, size, frames[0], False, True, True, "g", 0.5)
        assert np.array_equal(seg.apply(frames[0]), want)
    with FrameSegmenter(net, hf, wf, overlay=False, net_size=size) as seg:
        want, _ = expected(net, size, frames[1], True, False)
        got = seg.apply(frames[1])
        assert got.shape == (hf, wf) and np.array_equal(got, want)  # mask bytes at the frame's size
        # a frame that is on the device already
        assert np.array_equal(seg.apply(torch.from_numpy(frames[1]).to(DEV)), want)
    with FrameSegmenter(net, hf, wf, mirror=False, boolean_mask=False, color="b", alpha=0.5, net_size=size) as seg:
        want, logits = expected(net, size, frames[1], False, True, False, "b", 0.5)
        got = seg.apply(frames[1])
        band = C.soft_band_scaled(frames[1], logits, False, True, "b", 0.5)
        assert np.array_equal(got[..., 1:], want[..., 1:]) and np.array_equal(got[..., 0][~band], want[..., 0][~band])


def test_scaled_segmenter_keeps_order():
    from fosvos_hip.stream import FrameSegmenter
    net, size = small_net("vgg")
    hf, wf = 96, 172
    frames = camera_frames(7, hf, wf, seed=11)
    singles = [expected(net, size, f)[0] for f in frames]
    assert len({s.tobytes() for s in singles}) == 7  # seven different outputs: a swapped pair would show
    for depth in (1, 2, 3):
        with FrameSegmenter(net, hf, wf, depth=depth, net_size=size) as seg:
            first = list(seg.segment(iter(frames)))
            second = list(seg.segment(frames))
            assert len(first) == len(second) == 7
            for k in range(7):
                assert np.array_equal(first[k], singles[k]) and np.array_equal(second[k], singles[k]), (depth, k)


def test_scaled_segmenter_jpeg_files_have_the_frames_size():
    from fosvos_hip import ops
    from fosvos_hip.stream import FrameSegmenter
    net, size = small_net("vgg")
    hf, wf = 96, 172
    frames = camera_frames(3, hf, wf, seed=5)
    for kw, mode in ((dict(), "RGB"), (dict(overlay=False), "L")):
        defined = [expected(net, size, f, overlay=kw.get("overlay", True))[0] for f in frames]
        buf, lengths = ops.jpeg_encode(torch.from_numpy(np.ascontiguousarray(np.stack(defined))).to(DEV), 90)
        want = [buf[k, :int(lengths[k])].cpu().numpy().tobytes() for k in range(3)]
        with FrameSegmenter(net, hf, wf, depth=2, encode="jpeg", quality=90, net_size=size, **kw) as seg:
            assert seg.capacity == ops.jpeg_capacity(hf, wf, 3 if mode == "RGB" else 1, "4:4:4")  # sized by the frame
            got = list(seg.segment(frames))
        for k in range(3):
            assert isinstance(got[k], bytes)
            with Image.open(io.BytesIO(got[k])) as im, Image.open(io.BytesIO(want[k])) as ref:
                assert im.size == (wf, hf) and im.mode == mode
                assert np.array_equal(np.asarray(im), np.asarray(ref)), (kw, k)
            assert got[k] == want[k]


def test_segmenter_refuses_bad_net_sizes():
    from fosvos_hip.stream import FrameSegmenter
    net, _ = small_net("vgg")
    for bad in ((97, 86), (48, 173), (0, 86), (48, -1), (48,), 48, (48.0, 86), (True, 86), "ab"):
        with pytest.raises(ValueError):
            FrameSegmenter(net, 96, 172, net_size=bad)


def test_default_and_the_frames_own_size_are_the_unscaled_launches():
    from fosvos_hip import LaunchProfile
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_net("vgg")
    frames = camera_frames(3, h, w, seed=9)
    outs = []
    for kw in (dict(), dict(net_size=(h, w)), dict(net_size=None)):
        with FrameSegmenter(net, h, w, **kw) as seg:
            assert seg.net_size is None
            with LaunchProfile(0) as prof:
                outs.append([seg.apply(f) for f in frames])
            assert prof.records["k_frame_prep"]["launches"] == 3 and prof.records["k_overlay"]["launches"] == 3
            assert "k_frame_prep_scaled" not in prof.records and "k_overlay_scaled" not in prof.records
    for k in range(3):
        assert outs[0][k].tobytes() == outs[1][k].tobytes() == outs[2][k].tobytes()
    with FrameSegmenter(net, 2 * h, 2 * w, net_size=(h, w)) as seg:
        with LaunchProfile(0) as prof:
            seg.apply(camera_frames(1, 2 * h, 2 * w)[0])
    assert prof.records["k_frame_prep_scaled"]["launches"] == 1 and prof.records["k_overlay_scaled"]["launches"] == 1
    assert "k_frame_prep" not in prof.records and "k_overlay" not in prof.records


# ------------------------------------------------------------------------------------------ run_webcam
def test_run_webcam_main_with_a_net_size(tmp_path):
    import run_webcam
    net, size = small_net("vgg")
    hf, wf = 96, 172
    ckpt = tmp_path / "vgg.pth"
    torch.save(O.make_state_dict(2), str(ckpt))
    common = ["--variant", "vgg", "--model", str(ckpt), "--synthetic", "4", "--height", str(hf), "--width", str(wf),
              "--net-height", str(size[0]), "--net-width", str(size[1])]
    frames = [run_webcam.synthetic_frame(hf, wf, k) for k in range(4)]
    names = ["%05d.png" % k for k in range(4)]
    rates = run_webcam.main(common + ["--output", str(tmp_path / "overlay")])
    assert len(rates) == 4 and sorted(os.listdir(tmp_path / "overlay")) == names
    for k, name in enumerate(names):
        want, _ = expected(net, size, frames[k])  # the defaults: mirrored, boolean mask, red, alpha 1
        got = np.asarray(Image.open(str(tmp_path / "overlay" / name)))
        assert got.shape == (hf, wf, 3) and np.array_equal(got, want[:, :, ::-1])  # written as RGB
    run_webcam.main(common + ["--no-network", "--output", str(tmp_path / "plain")])  # the net's size is ignored
    for k, name in enumerate(names):
        got = np.asarray(Image.open(str(tmp_path / "plain" / name)))
        assert np.array_equal(got, frames[k][:, ::-1, ::-1])
