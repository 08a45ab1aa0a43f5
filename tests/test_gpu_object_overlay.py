"""Several objects in streaming inference, on a real MI355X: ``ops.overlay_objects`` (csrc/stream.hip: k_overlay_objects,
k_overlay_objects_scaled) against the numpy statement of the bytes (util/object_overlay.py), ``ObjectSegmenter`` and
``run_webcam.main --models`` end to end.  Every comparison is exact equality: there are no soft modes."""
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

import object_overlay_cases as C  # noqa: E402
from util import frame_overlay as F  # noqa: E402
from util import frame_resample as R  # noqa: E402
from util import jpeg_layout  # noqa: E402
from util import object_merge as M  # noqa: E402
from util import object_overlay as OO  # noqa: E402
from util import png_layout  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = 0xA5
GUARD = 16


def offset_view(t, elems=1):
    """The same values in a tensor whose base pointer lies `elems` elements behind an allocation's start."""
    buf = torch.empty(t.numel() + elems, dtype=t.dtype, device=t.device)
    view = buf[elems:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elems * t.element_size()
    return view


def guarded(shape, lead):
    """(buffer, view): a uint8 output of `shape` filled with garbage, `lead` bytes behind the start of a buffer of garbage
    that also runs GUARD bytes past it."""
    numel = int(np.prod(shape))
    buf = torch.full((lead + numel + GUARD,), GARBAGE, dtype=torch.uint8, device=DEV)
    return buf, buf[lead:lead + numel].view(shape)


def guards_intact(buf, view, lead):
    b = buf.cpu().numpy()
    return (b[:lead] == GARBAGE).all() and (b[lead + view.numel():] == GARBAGE).all()


def on_device(maps, offsets=False):
    """The K maps on the device; with `offsets` map k lies 1, 2 or 3 floats behind an allocation's start."""
    ts = [torch.from_numpy(m).to(DEV) for m in maps]
    return [offset_view(t, 1 + k % 3) for k, t in enumerate(ts)] if offsets else ts


def device_palette(pal):
    return None if pal is None else torch.from_numpy(pal).to(DEV)


# ------------------------------------------------------------------------------------------ unscaled
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.SHAPE_IDS)
def test_overlay_objects_is_the_definition(shape):
    from fosvos_hip import ops
    n, h, w = shape
    f = C.frames(n, h, w)
    fd = torch.from_numpy(f).to(DEV)
    step = 0
    for k in (1, 3, 16):
        maps = C.logits(k, n, h, w)
        for mirror in (False, True):
            for name, pal in C.palettes().items():
                alpha = C.ALPHAS[step % len(C.ALPHAS)]
                step += 1
                want = np.stack([OO.overlay(f[i], C.frame_maps(maps, i), mirror, pal, alpha) for i in range(n)])
                for offsets in (False, True):
                    lead = 5 if offsets else GUARD
                    buf, out = guarded((n, h, w, 3), lead)
                    got = ops.overlay_objects(offset_view(fd, 1) if offsets else fd, on_device(maps, offsets), mirror, True,
                                              device_palette(pal), alpha, out=out)
                    assert got is out
                    got = out.cpu().numpy()
                    assert np.array_equal(got, want), (shape, k, mirror, name, alpha, offsets, int((got != want).sum()))
                    assert guards_intact(buf, out, lead), (shape, k, mirror, name, offsets)
    again = ops.overlay_objects(fd, on_device(maps), True, palette=device_palette(pal), alpha=alpha)  # an out of its own
    assert again.shape == (n, h, w, 3) and np.array_equal(again.cpu().numpy(), want)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.SHAPE_IDS)
def test_label_map_unscaled_is_merge_objects(shape):
    from fosvos_hip import LaunchProfile, ops
    n, h, w = shape
    fd = torch.from_numpy(C.frames(n, h, w)).to(DEV)
    for k in (1, 3, 16):
        maps = C.logits(k, n, h, w)
        md = on_device(maps)
        want = ops.merge_objects(md).cpu().numpy()
        assert np.array_equal(want, np.stack([OO.labels(C.frame_maps(maps, i)) for i in range(n)]))
        with LaunchProfile(0) as prof:
            for mirror in (False, True):  # nothing to mirror: the logits are in output order
                buf, out = guarded((n, h, w), 5)
                assert ops.overlay_objects(fd, md, mirror, overlay=False, out=out) is out
                assert np.array_equal(out.cpu().numpy(), want) and guards_intact(buf, out, 5)
        assert prof.records["k_merge_objects"]["launches"] == 2 and "k_overlay_objects" not in prof.records


def test_one_object_labels_the_pixels_the_single_object_mask_marks():
    """No equivalence with ops.overlay is claimed (that one adds to a channel, this one blends): the labelled pixels are the
    mask's pixels."""
    from fosvos_hip import ops
    n, h, w = 2, 5, 64
    f = C.frames(n, h, w)
    fd = torch.from_numpy(f).to(DEV)
    maps = C.logits(1, n, h, w)
    md = on_device(maps)
    pal = M.davis_palette()
    pal[1] = (0, 0, 255)
    mask = ops.overlay(fd, md[0], overlay=False).cpu().numpy()
    assert set(np.unique(mask).tolist()) == {0, 255}
    got = ops.overlay_objects(fd, md, False, True, device_palette(pal), 1.0).cpu().numpy()
    assert (got[mask == 255] == np.array([255, 0, 0], dtype=np.uint8)).all()  # entry 1 is RGB (0,0,255): blue in BGR first
    assert np.array_equal(got[mask == 0], f[mask == 0])
    assert np.array_equal(ops.overlay_objects(fd, md, overlay=False).cpu().numpy(), mask // 255)


# ------------------------------------------------------------------------------------------ scaled
@pytest.mark.parametrize("size", C.SCALED, ids=C.SCALED_IDS)
def test_overlay_objects_scaled_is_the_definition(size):
    from fosvos_hip import LaunchProfile, ops
    hf, wf, hn, wn = size
    n = C.SCALED_N
    f = C.frames(n, hf, wf)
    fd = torch.from_numpy(f).to(DEV)
    pal = C.random_palette()
    pd = device_palette(pal)
    step = 0
    with LaunchProfile(0) as prof:
        for k in (1, 2, 16):
            maps = C.logits_scaled(k, n, hn, wn)
            labels = np.stack([OO.labels(C.frame_maps(maps, i), hf, wf) for i in range(n)])
            for offsets in (False, True):
                lead = 5 if offsets else GUARD
                frames_d, maps_d = (offset_view(fd, 1) if offsets else fd), on_device(maps, offsets)
                for mirror in (False, True):
                    alpha = C.ALPHAS[step % len(C.ALPHAS)]
                    step += 1
                    want = np.stack([OO.overlay(f[i], C.frame_maps(maps, i), mirror, pal, alpha, hf, wf) for i in range(n)])
                    buf, out = guarded((n, hf, wf, 3), lead)
                    assert ops.overlay_objects(frames_d, maps_d, mirror, True, pd, alpha, out=out, net_size=(hn, wn)) is out
                    got = out.cpu().numpy()
                    assert np.array_equal(got, want), (size, k, mirror, alpha, offsets, int((got != want).sum()))
                    assert guards_intact(buf, out, lead)
                    buf, out = guarded((n, hf, wf), lead)
                    ops.overlay_objects(frames_d, maps_d, mirror, False, pd, alpha, out=out, net_size=(hn, wn))
                    got = out.cpu().numpy()
                    assert np.array_equal(got, labels), (size, k, mirror, offsets, int((got != labels).sum()))
                    assert guards_intact(buf, out, lead)
    assert prof.records["k_overlay_objects_scaled"]["launches"] == 3 * 2 * 2 * 2
    assert "k_overlay_objects" not in prof.records and "k_merge_objects" not in prof.records


# ------------------------------------------------------------------------------------------ arguments, streams
def test_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    n, h, w, hn, wn = 2, 33, 47, 16, 20
    f = torch.from_numpy(C.frames(n, h, w)).to(DEV)
    x = on_device(C.logits(3, n, h, w))
    xs = on_device(C.logits_scaled(3, n, hn, wn))
    out = torch.full((n, h, w, 3), 7, dtype=torch.uint8, device=DEV)
    lab = torch.full((n, h, w), 7, dtype=torch.uint8, device=DEV)
    pal = ops.default_palette(DEV)
    wide = torch.empty((n, 1, h, 2 * w), device=DEV)
    with LaunchProfile(0) as prof:
        for bad in (lambda: ops.overlay_objects(f, [], out=out), lambda: ops.overlay_objects(f, x[:1] * 17, out=out),
                    lambda: ops.overlay_objects(f, [x[0], x[1][:, :, :, :46]], out=out),   # mismatched shapes
                    lambda: ops.overlay_objects(f, [x[0], x[1][:1]], out=out),
                    lambda: ops.overlay_objects(f, [x[0][:, 0], x[1][:, 0]], out=out),
                    lambda: ops.overlay_objects(f, xs, out=out),                           # scaling is never inferred
                    lambda: ops.overlay_objects(f, x, out=out, net_size=(hn, wn)),         # logits not of net_size
                    lambda: ops.overlay_objects(f, [x[0], wide[:, :, :, ::2]], out=out),   # a non-contiguous map
                    lambda: ops.overlay_objects(f, [x[0], x[1].double()], out=out),
                    lambda: ops.overlay_objects(f.int(), x, out=out), lambda: ops.overlay_objects(f[:0], [t[:0] for t in x]),
                    lambda: ops.overlay_objects(f, x, palette=pal[:255], out=out),         # a palette of [255,3]
                    lambda: ops.overlay_objects(f, x, palette=pal.int(), out=out),
                    lambda: ops.overlay_objects(f, x, alpha=-0.1, out=out), lambda: ops.overlay_objects(f, x, alpha=1.5, out=out),
                    lambda: ops.overlay_objects(f, x, alpha=float("nan"), out=out),
                    lambda: ops.overlay_objects(f, x, overlay=False, alpha=1.5, out=lab),
                    lambda: ops.overlay_objects(f, xs, alpha=float("nan"), out=out, net_size=(hn, wn)),
                    lambda: ops.overlay_objects(f, xs, out=out, net_size=(h + 1, wn)),     # net_size larger than the frame
                    lambda: ops.overlay_objects(f, xs, out=out, net_size=(hn, w + 1)),
                    lambda: ops.overlay_objects(f, xs, overlay=False, out=lab, net_size=(h + 1, w)),
                    lambda: ops.overlay_objects(f, x, out=lab), lambda: ops.overlay_objects(f, x, overlay=False, out=out),
                    lambda: ops.overlay_objects(f, x, out=out[:, :, :, :2])):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.overlay_objects(f, [x[0], x[1].cpu()], out=out),             # a map on the CPU
                    lambda: ops.overlay_objects(f.cpu(), x, out=out), lambda: ops.overlay_objects(f, x, palette=pal.cpu(), out=out),
                    lambda: ops.overlay_objects(f, x, out=out.cpu())):
            with pytest.raises(RuntimeError):
                bad()

        # straight through the C ABI: the library's error codes, never a fault
        import ctypes
        L = lib()
        st = torch.cuda.current_stream().cuda_stream

        def table(ts):
            return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])

        def ov(fr=f.data_ptr(), lg=table(x), k=3, n_=n, h_=h, w_=w, p=pal.data_ptr(), alpha=0.5, o=out.data_ptr()):
            return L.fosvos_overlay_objects(fr, lg, k, n_, h_, w_, 1, p, alpha, o, 0, st)

        def ovs(fr=f.data_ptr(), lg=table(xs), k=3, n_=n, hf_=h, wf_=w, hn_=hn, wn_=wn, mode=0, p=pal.data_ptr(), alpha=0.5,
                o=out.data_ptr()):
            return L.fosvos_overlay_objects_scaled(fr, lg, k, n_, hf_, wf_, hn_, wn_, 1, mode, p, alpha, o, 0, st)

        for call in (ov, ovs):
            assert call(k=0) == -2 and b"K=0" in L.fosvos_last_error()
            assert call(k=17) == -2 and call(lg=None) == -2 and call(fr=None) == -2 and call(p=None) == -2 and call(o=None) == -2
            assert call(lg=table([x[0], None, x[2]])) == -2 and b"map 1" in L.fosvos_last_error()
            assert call(lg=table([x[0], x[1].data_ptr() + 2, x[2]])) == -2  # a map off its own alignment
            assert call(alpha=-0.1) == -2 and call(alpha=1.5) == -2 and call(alpha=float("nan")) == -2
            assert call(n_=0) == -1
        assert ov(h_=0) == -1 and ov(w_=-3) == -1
        assert ovs(mode=2) == -2 and ovs(mode=-1) == -2
        assert ovs(hf_=0) == -1 and ovs(hn_=0) == -1 and ovs(wn_=0) == -1 and ovs(hf_=8193) == -1 and ovs(wf_=8193) == -1
        assert ovs(hn_=h + 1) == -1 and b"exceeds" in L.fosvos_last_error()
        assert ovs(wn_=w + 1) == -1
    assert not prof.records, prof.records
    torch.cuda.synchronize()
    assert (out == 7).all() and (lab == 7).all()  # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        ops.overlay_objects(f, x, True, out=out)
        ops.overlay_objects(f, xs, True, out=out, net_size=(hn, wn))
        ops.overlay_objects(f, x, True, out=out, net_size=(h, w))  # the frames' own size: the unscaled launch
        assert ovs(fr=None, p=None, mode=1, alpha=7.0, o=lab.data_ptr()) == 0  # the label map reads neither
    assert prof.records["k_overlay_objects"]["launches"] == 2 and prof.records["k_overlay_objects_scaled"]["launches"] == 2


def test_ops_run_on_the_callers_stream_and_repeat():
    from fosvos_hip import ops
    n, h, w, hn, wn = 2, 48, 86, 24, 43
    f = torch.from_numpy(C.frames(n, h, w)).to(DEV)
    x, xs = on_device(C.logits(3, n, h, w)), on_device(C.logits_scaled(3, n, hn, wn))

    def run():
        return [ops.overlay_objects(f, x, True), ops.overlay_objects(f, x, overlay=False),
                ops.overlay_objects(f, xs, True, net_size=(hn, wn)), ops.overlay_objects(f, xs, overlay=False, net_size=(hn, wn))]

    first = run()
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert np.array_equal(first[0].cpu().numpy(),
                          np.stack([OO.overlay(f[i].cpu().numpy(), [t[i, 0].cpu().numpy() for t in x], True) for i in range(n)]))


# ------------------------------------------------------------------------------------------ ObjectSegmenter
_NETS = {}


def vgg_net(seed):
    """The small-weight VGG of the oracle with the weights of `seed`, built once; it runs at 48 x 86."""
    if seed not in _NETS:
        from networks.osvos_vgg import OSVOS_VGG
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        _NETS[seed] = net.to(DEV).eval()
    return _NETS[seed]


def thin_resnet():
    if "resnet" not in _NETS:
        from networks.osvos_resnet import OSVOS_RESNET
        torch.manual_seed(7)
        _NETS["resnet"] = OSVOS_RESNET(pretrained=False, version=18, scale_down_exponent=3).to(DEV).eval()
    return _NETS["resnet"]


VGG_SIZE = (48, 86)
SEEDS = (2, 3, 4)


def camera_frames(count, h, w, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def logits_of(nets, frame, mirror=True, net_size=None):
    """What the same nets answer when they are called directly on the host's statement of the prepared frame."""
    x = F.prepare_frame(frame, mirror) if net_size is None else R.prepare_frame_scaled(frame, net_size[0], net_size[1], mirror)
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        return [net.forward(xd)[-1][0, 0].cpu().numpy() for net in nets]


def expected(nets, frame, mirror=True, overlay=True, palette=None, alpha=0.5, net_size=None):
    hf, wf = (frame.shape[0], frame.shape[1]) if net_size is not None else (None, None)
    return OO.apply(frame, logits_of(nets, frame, mirror, net_size), mirror, overlay, palette, alpha, hf, wf)


def test_segmenter_apply_is_the_definition():
    from fosvos_hip import LaunchProfile
    from fosvos_hip.stream import ObjectSegmenter
    nets = [vgg_net(s) for s in SEEDS]
    h, w = VGG_SIZE
    frames = camera_frames(2, h, w)
    with ObjectSegmenter(nets, h, w) as seg:  # defaults: mirror, overlay, the DAVIS palette, alpha 0.5
        for frame in frames:
            with LaunchProfile(0) as prof:
                got = seg.apply(frame)
            assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got, expected(nets, frame))
            assert prof.records["k_frame_prep"]["launches"] == 1 and prof.records["k_overlay_objects"]["launches"] == 1
            assert "k_merge_objects" not in prof.records and "k_overlay" not in prof.records
            print("labels of the frame:", np.bincount(OO.labels(logits_of(nets, frame)).ravel(), minlength=4).tolist())
        assert all(net.compute_side_outputs is True for net in nets)  # restored
        # a frame that is on the device already
        assert np.array_equal(seg.apply(torch.from_numpy(frames[1]).to(DEV)), expected(nets, frames[1]))
    pal = C.random_palette()
    with ObjectSegmenter(nets, h, w, depth=1, mirror=False, palette=pal, alpha=0.3) as seg:
        assert np.array_equal(seg.apply(frames[0]), expected(nets, frames[0], False, True, pal, 0.3))
    with ObjectSegmenter(nets, h, w, palette=torch.from_numpy(pal).to(DEV), alpha=1.0) as seg:
        assert np.array_equal(seg.apply(frames[0]), expected(nets, frames[0], True, True, pal, 1.0))
    with ObjectSegmenter(nets, h, w, overlay=False) as seg:
        got = seg.apply(frames[1])
        assert got.shape == (h, w) and np.array_equal(got, expected(nets, frames[1], True, False))
    with ObjectSegmenter(nets[:1], h, w) as seg:  # one object
        assert np.array_equal(seg.apply(frames[0]), expected(nets[:1], frames[0]))


def test_segmenter_with_a_net_size_and_a_mixed_pair():
    from fosvos_hip import LaunchProfile
    from fosvos_hip.stream import ObjectSegmenter
    nets = [vgg_net(s) for s in SEEDS]
    h, w = VGG_SIZE
    frame = camera_frames(1, h, w, seed=8)[0]
    for overlay in (True, False):
        with ObjectSegmenter(nets, h, w, overlay=overlay, net_size=(24, 43)) as seg:
            assert seg.net_size == (24, 43)
            with LaunchProfile(0) as prof:
                got = seg.apply(frame)
            assert got.shape == ((h, w, 3) if overlay else (h, w))
            assert np.array_equal(got, expected(nets, frame, overlay=overlay, net_size=(24, 43)))
            assert prof.records["k_frame_prep_scaled"]["launches"] == 1
            assert prof.records["k_overlay_objects_scaled"]["launches"] == 1 and "k_overlay_objects" not in prof.records
    pair = [vgg_net(2), thin_resnet()]  # a VGG and a thin ResNet-18 on the same image
    frame = camera_frames(1, 64, 96, seed=9)[0]
    with ObjectSegmenter(pair, 64, 96) as seg:
        assert np.array_equal(seg.apply(frame), expected(pair, frame))
    with ObjectSegmenter(pair, 64, 96, overlay=False, mirror=False) as seg:
        assert np.array_equal(seg.apply(frame), expected(pair, frame, False, False))


def test_segmenter_keeps_order():
    from fosvos_hip.stream import ObjectSegmenter
    nets = [vgg_net(s) for s in SEEDS]
    h, w = VGG_SIZE
    frames = camera_frames(7, h, w, seed=11)
    singles = [expected(nets, f) for f in frames]
    assert len({s.tobytes() for s in singles}) == 7  # seven different outputs: a swapped pair would show
    for depth in (1, 2, 3):
        with ObjectSegmenter(nets, h, w, depth=depth) as seg:
            first = list(seg.segment(iter(frames)))
            second = list(seg.segment(frames))
            assert len(first) == len(second) == 7 and seg.pending == 0
            for k in range(7):
                assert np.array_equal(first[k], singles[k]) and np.array_equal(second[k], singles[k]), (depth, k)


def test_segmenter_files():
    from fosvos_hip import ops
    from fosvos_hip.stream import ObjectSegmenter
    nets = [vgg_net(s) for s in SEEDS]
    h, w = VGG_SIZE
    frames = camera_frames(3, h, w, seed=5)
    pal = C.random_palette()
    # the label map as a palette PNG
    for kw in (dict(), dict(palette=pal, huffman="fitted")):
        want = [png_layout.encode_indexed(expected(nets, f, overlay=False), kw.get("palette"), kw.get("huffman", "fixed"))
                for f in frames]
        with ObjectSegmenter(nets, h, w, overlay=False, encode="png", **kw) as seg:
            assert seg.capacity == ops.png_indexed_capacity(h, w) and seg.budget == max(seg.capacity // 4, 1024)
            got = list(seg.segment(frames))
            assert all(isinstance(g, bytes) for g in got) and got == want
            with Image.open(io.BytesIO(got[0])) as im:
                assert im.mode == "P" and im.size == (w, h)
                assert np.array_equal(np.asarray(im), expected(nets, frames[0], overlay=False))
        # a tiny budget forces the second copy and still returns the whole file
        with ObjectSegmenter(nets, h, w, overlay=False, encode="png", budget=64, **kw) as seg:
            assert seg.budget == 64
            assert list(seg.segment(frames)) == want and seg.second_copies == 3
    # the overlay as a JPEG
    want = [jpeg_layout.encode(expected(nets, f), 80) for f in frames]
    with ObjectSegmenter(nets, h, w, encode="jpeg", quality=80) as seg:
        assert seg.capacity == ops.jpeg_capacity(h, w, 3, "4:4:4")
        assert list(seg.segment(frames)) == want
    with ObjectSegmenter(nets, h, w, encode="jpeg", quality=80, budget=100) as seg:
        assert list(seg.segment(frames)) == want and seg.second_copies == 3


def test_segmenter_refusals():
    from fosvos_hip import LaunchProfile
    from fosvos_hip.stream import ObjectSegmenter
    from networks.osvos_vgg import OSVOS_VGG
    nets = [vgg_net(s) for s in SEEDS]
    h, w = VGG_SIZE
    good = camera_frames(1, h, w, seed=5)[0]
    with ObjectSegmenter(nets, h, w) as seg:
        want = seg.apply(good)
        with LaunchProfile(0) as prof:
            for bad in (good[:, :-1], good[:-1], good[:, :, :2], good.astype(np.float32), good.tolist(), torch.from_numpy(good)):
                with pytest.raises(ValueError):
                    seg.submit(bad)
            assert seg.pending == 0
        assert not prof.records, prof.records  # nothing was queued
        assert np.array_equal(seg.apply(good), want)
        # a failing net (the second of three) leaves the segmenter usable and every net as it was
        nets[1].forward = lambda x: (_ for _ in ()).throw(KeyError("no such layer"))
        try:
            with pytest.raises(KeyError):
                seg.submit(good)
        finally:
            del nets[1].forward
        assert seg.pending == 0 and all(net.compute_side_outputs is True for net in nets)
        assert np.array_equal(seg.apply(good), want)
    with pytest.raises(RuntimeError):
        seg.submit(good)  # closed
    for bad in (dict(nets=[nets[0], nets[1], nets[0]]), dict(nets=[]), dict(nets=[nets[0]] * 17),
                dict(encode="jpeg", overlay=False), dict(encode="png", overlay=True), dict(encode="gif"), dict(budget=4096),
                dict(alpha=1.5), dict(alpha=-0.1), dict(alpha=float("nan")), dict(depth=0), dict(net_size=(49, 86)),
                dict(palette=np.zeros((255, 3), np.uint8)), dict(huffman="fitted"), dict(subsampling="4:2:0"),
                dict(overlay=False, encode="png", huffman="best"), dict(overlay=False, encode="png", budget=0)):
        with pytest.raises(ValueError):
            ObjectSegmenter(**{"nets": nets, "height": h, "width": w, **bad})
    with pytest.raises(ValueError):
        ObjectSegmenter([vgg_net(2)] + [OSVOS_VGG(pretrained=0).to(DEV)] * 16, h, w)  # 17 nets (and repeats)
    with pytest.raises(RuntimeError, match="GPU"):
        ObjectSegmenter([nets[0], OSVOS_VGG(pretrained=0)], h, w)  # a CPU net


def test_a_frame_segmenter_on_the_same_net_keeps_its_bytes():
    from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
    nets = [vgg_net(s) for s in SEEDS]
    h, w = VGG_SIZE
    frames = camera_frames(2, h, w, seed=13)
    with FrameSegmenter(nets[0], h, w) as single:
        before = [single.apply(f) for f in frames]
        with ObjectSegmenter(nets, h, w) as seg:
            several = [seg.apply(f) for f in frames]
        after = [single.apply(f) for f in frames]
    for k in range(2):
        assert np.array_equal(before[k], after[k])
        x = logits_of(nets[:1], frames[k])[0]
        assert np.array_equal(before[k], F.apply(frames[k], x, True))
        assert np.array_equal(several[k], expected(nets, frames[k]))


# ------------------------------------------------------------------------------------------ run_webcam
def test_run_webcam_main_with_models(tmp_path):
    import run_webcam
    nets = [vgg_net(s) for s in SEEDS[:2]]
    h, w = VGG_SIZE
    files = []
    for seed in SEEDS[:2]:
        files.append(str(tmp_path / ("seq_%d.pth" % seed)))
        torch.save(O.make_state_dict(seed), files[-1])
    common = ["--variant", "vgg", "--models"] + files + ["--synthetic", "3", "--height", str(h), "--width", str(w)]
    frames = [run_webcam.synthetic_frame(h, w, k) for k in range(3)]
    names = ["%05d.png" % k for k in range(3)]
    rates = run_webcam.main(common + ["--output", str(tmp_path / "overlay")])
    assert len(rates) == 3 and sorted(os.listdir(tmp_path / "overlay")) == names
    for k, name in enumerate(names):
        got = np.asarray(Image.open(str(tmp_path / "overlay" / name)))
        assert got.shape == (h, w, 3) and np.array_equal(got, expected(nets, frames[k])[:, :, ::-1])  # written as RGB
    run_webcam.main(common + ["--no-overlay", "--palette-alpha", "1.0", "--output", str(tmp_path / "labels")])
    assert sorted(os.listdir(tmp_path / "labels")) == names
    for k, name in enumerate(names):
        labels = expected(nets, frames[k], overlay=False)
        assert (tmp_path / "labels" / name).read_bytes() == png_layout.encode_indexed(labels)
        with Image.open(str(tmp_path / "labels" / name)) as im:
            assert im.mode == "P" and np.array_equal(np.asarray(im), labels)
            assert np.array_equal(np.array(im.getpalette(), dtype=np.uint8).reshape(-1, 3), M.davis_palette())
