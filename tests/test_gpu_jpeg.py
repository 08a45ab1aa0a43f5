"""The device JPEG encoder on a real MI355X (csrc/jpeg.hip through ``ops.jpeg_encode``) against the integer statement of its
layout (util/jpeg_layout.py) - byte for byte, so no tolerance anywhere - and ``FrameSegmenter(encode='jpeg')`` end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_cases as C  # noqa: E402
from util import frame_overlay as F, jpeg_layout as J  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


def dirty_workspace():
    from fosvos_hip import ops
    torch.cuda.synchronize()
    for buf in ops._WS._buf.values():
        buf.fill_(FILL)


def encode_checked(frames, quality, want=None, view=False):
    """ops.jpeg_encode of uint8 [N,H,W(,3)] into a buffer filled with 0xA5; returns the files after checking them against the
    layout and the untouched tail.  ``view``: the frames start one byte into their allocation."""
    from fosvos_hip import ops
    n, h, w = frames.shape[:3]
    comps = 3 if frames.ndim == 4 else 1
    cap = ops.jpeg_capacity(h, w, comps)
    assert cap == J.capacity(h, w, comps)
    if view:
        store = torch.zeros((frames.size + 1,), dtype=torch.uint8, device=DEV)
        x = store[1:].view(frames.shape)
        x.copy_(torch.from_numpy(frames))
        assert x.data_ptr() % 2 == 1
    else:
        x = torch.from_numpy(frames).to(DEV)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    dirty_workspace()
    got_out, got_len = ops.jpeg_encode(x, quality, out=out, lengths=lengths)
    assert got_out is out and got_len is lengths
    torch.cuda.synchronize()
    buf, lens = out.cpu().numpy(), lengths.cpu().tolist()
    files = []
    for k in range(n):
        ref = J.encode(frames[k], quality) if want is None else want[k]
        assert lens[k] == len(ref), (k, frames.shape, quality, lens[k], len(ref))
        got = buf[k, :lens[k]].tobytes()
        if got != ref:
            at = next(i for i in range(len(ref)) if got[i] != ref[i])
            raise AssertionError("frame %d of %s at q=%d differs from the layout at byte %d of %d"
                                 % (k, frames.shape, quality, at, len(ref)))
        assert (buf[k, lens[k]:] == FILL).all(), "bytes behind the file were written"
        files.append(got)
    return files


_INPUTS = C.all_inputs()


@pytest.mark.parametrize("case", _INPUTS, ids=[c[0] for c in _INPUTS])
def test_jpeg_encode_is_the_layout_byte_for_byte(case):
    _, frame, q = case
    want = [J.encode(frame, q)]
    encode_checked(frame[None], q, want)
    encode_checked(frame[None], q, want, view=True)


@pytest.mark.parametrize("grey", [False, True], ids=["bgr", "grey"])
def test_jpeg_encode_batch_of_three(grey):
    frames = np.stack([C.picture(61, 107, grey), C.noise(61, 107, grey), C.smooth(61, 107, grey)])
    for q in C.QUALITIES:
        files = encode_checked(frames, q)
        assert len(set(files)) == 3
        encode_checked(frames, q, files, view=True)
        mode, img = C.decode(files[0])
        assert mode == ("L" if grey else "RGB") and img.shape == frames[0].shape


def test_jpeg_encode_views_side_stream_and_repeat():
    from fosvos_hip import ops
    frames = np.stack([C.picture(61, 107), C.noise(61, 107), C.smooth(61, 107)])
    x = torch.from_numpy(frames).to(DEV)
    want = [J.encode(f, 90) for f in frames]
    first_out, first_len = ops.jpeg_encode(x)           # quality 90 is the default
    dirty_workspace()
    second_out, second_len = ops.jpeg_encode(x)
    torch.cuda.synchronize()
    assert torch.equal(first_len, second_len) and first_len.cpu().tolist() == [len(f) for f in want]
    for k, f in enumerate(want):
        assert first_out[k, :len(f)].cpu().numpy().tobytes() == f
        assert torch.equal(first_out[k, :len(f)], second_out[k, :len(f)])
    # views into a caller's buffer: file slots wider than the capacity that start at any byte, lengths behind them
    cap = ops.jpeg_capacity(61, 107, 3)
    for lead, stride in ((1, cap + 3), (2, cap + 1), (3, cap), (0, cap + 2)):
        room = lead + 3 * stride
        room += -room % 4
        store = torch.full((room + 12 + 8,), FILL, dtype=torch.uint8, device=DEV)
        out = store[lead:lead + 3 * stride].view(3, stride)
        lengths = store[room:room + 12].view(torch.int32)
        ops.jpeg_encode(x, 90, out=out, lengths=lengths)
        torch.cuda.synchronize()
        host = store.cpu().numpy()
        assert lengths.cpu().tolist() == [len(f) for f in want]
        keep = np.ones(host.size, dtype=bool)
        for k, f in enumerate(want):
            at = lead + k * stride
            assert host[at:at + len(f)].tobytes() == f, (lead, stride, k)
            keep[at:at + len(f)] = False
        keep[room:room + 12] = False
        assert (host[keep] == FILL).all()            # the slack of every row and everything else is untouched
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out, lengths = ops.jpeg_encode(x)
    side.synchronize()
    for k, f in enumerate(want):
        assert out[k, :len(f)].cpu().numpy().tobytes() == f and int(lengths[k]) == len(f)


def test_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    L = lib()
    n, h, w = 2, 24, 40
    cap, need = L.fosvos_jpeg_capacity_bytes(n, h, w, 3, 444), L.fosvos_jpeg_workspace_bytes(n, h, w, 3, 444)
    assert cap == J.capacity(h, w, 3) and need == n * J.n_intervals(h, w) * 4
    assert L.fosvos_jpeg_capacity_bytes(1, 1080, 1920, 3, 444) == J.capacity(1080, 1920, 3)
    assert L.fosvos_jpeg_capacity_bytes(1, 0, 5, 3, 444) == 0 and L.fosvos_jpeg_capacity_bytes(1, 5, 5, 2, 444) == 0
    assert L.fosvos_jpeg_workspace_bytes(0, 5, 5, 1, 444) == 0
    x = torch.from_numpy(np.stack([C.picture(h, w)] * n)).to(DEV)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.full((need,), FILL, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(b=x.data_ptr(), n_=n, h_=h, w_=w, c_=3, q=90, o=out.data_ptr(), c=cap, l=lengths.data_ptr(), w2=ws.data_ptr(), nb=need):
        return L.fosvos_jpeg_encode(b, n_, h_, w_, c_, 444, q, o, c, l, w2, nb, 0, st)

    with LaunchProfile(0) as prof:
        assert call(nb=need - 1) == -3 and b"workspace" in L.fosvos_last_error()   # a short workspace
        assert call(nb=0) == -3
        assert call(c=cap - 1) == -3 and b"out_stride" in L.fosvos_last_error()
        assert call(q=0) == -2 and b"quality" in L.fosvos_last_error()
        assert call(q=101) == -2
        assert call(c_=2) == -1 and call(c_=4) == -1 and call(c_=0) == -1
        assert call(h_=0) == -1 and call(w_=0) == -1 and call(n_=0) == -1 and call(w_=-2) == -1 and call(h_=65536) == -1
        assert call(b=None) == -2 and call(o=None) == -2 and call(l=None) == -2 and call(w2=None) == -2
        assert call(w2=ws.data_ptr() + 2) == -2
        for bad in (lambda: ops.jpeg_encode(x.float()), lambda: ops.jpeg_encode(x[:, :, :, :2].contiguous()),
                    lambda: ops.jpeg_encode(x[:, :, :, :2]), lambda: ops.jpeg_encode(x[0, 0]),
                    lambda: ops.jpeg_encode(x, 0), lambda: ops.jpeg_encode(x, 101), lambda: ops.jpeg_encode(x, 50.5),
                    lambda: ops.jpeg_encode(x, out=out[:, :cap - 1].contiguous()), lambda: ops.jpeg_encode(x, out=out[:1]),
                    lambda: ops.jpeg_encode(x, lengths=lengths.long()), lambda: ops.jpeg_encode(x, lengths=lengths[:1]),
                    lambda: ops.jpeg_encode(x, lengths=lengths.view(1, n)),
                    lambda: ops.jpeg_encode(torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device=DEV))):
            with pytest.raises(ValueError):
                bad()
        two_devices = [lambda: ops.jpeg_encode(x.cpu()), lambda: ops.jpeg_encode(x, out=out.cpu()),
                       lambda: ops.jpeg_encode(x, lengths=lengths.cpu())]
        if torch.cuda.device_count() > 1:
            two_devices.append(lambda: ops.jpeg_encode(x, out=out.to("cuda:1")))
        for bad in two_devices:
            with pytest.raises(RuntimeError):
                bad()
    assert not any(name.startswith("k_jpeg") for name in prof.records), prof.records
    torch.cuda.synchronize()
    assert (out == FILL).all() and (lengths == -1).all() and (ws == FILL).all()  # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        assert call() == 0
        ops.jpeg_encode(x[..., 0].contiguous())
    assert prof.records["k_jpeg_measure"]["launches"] == 1 and prof.records["k_jpeg_emit"]["launches"] == 1
    assert prof.records["k_jpeg_measure_grey"]["launches"] == 1 and prof.records["k_jpeg_emit_grey"]["launches"] == 1
    want = J.encode(C.picture(h, w), 90)
    assert lengths.cpu().tolist() == [len(want)] * 2 and out[1, :len(want)].cpu().numpy().tobytes() == want


# ------------------------------------------------------------------------------------------ FrameSegmenter(encode='jpeg')
_NET = []


def small_vgg():
    if not _NET:
        from networks.osvos_vgg import OSVOS_VGG
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(2))
        _NET.append(net.to(DEV).eval())
    return _NET[0], (48, 86)


def camera_frames(count, h, w, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def definition(net, frame, **kw):
    with torch.no_grad():
        logits = net.forward(torch.from_numpy(F.prepare_frame(frame, kw.get("mirror", True))).to(DEV))[-1]
    return F.apply(frame, logits[0, 0].cpu().numpy(), kw.get("mirror", True), kw.get("overlay", True), True,
                   kw.get("color", "r"), kw.get("alpha", 1.0))


def test_segmenter_jpeg_is_the_layout_of_the_definition():
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_vgg()
    frames = camera_frames(5, h, w, seed=11)
    for kw, q in ((dict(), 90), (dict(overlay=False), 50), (dict(mirror=False, color="g", alpha=0.5), 100)):
        with FrameSegmenter(net, h, w, depth=2, **kw) as seg:            # encode=None: the arrays, as before
            arrays = list(seg.segment(frames))
            assert seg.encode is None and seg.second_copies == 0
        for k, f in enumerate(frames):
            assert isinstance(arrays[k], np.ndarray) and np.array_equal(arrays[k], definition(net, f, **kw)), (kw, k)
        want = [J.encode(a, q) for a in arrays]
        assert len(set(want)) == 5                                       # five different files: a swapped pair would show
        raw = h * w * (3 if kw.get("overlay", True) else 1)
        for depth, budget in ((1, None), (2, None), (2, 64), (3, 10 ** 9)):
            with FrameSegmenter(net, h, w, depth=depth, encode="jpeg", quality=q, budget=budget, **kw) as seg:
                got = list(seg.segment(iter(frames)))
                assert all(isinstance(g, bytes) for g in got) and got == want, (kw, depth, budget)
                assert seg.apply(frames[3]) == want[3]
                long_files = sum(len(f) > seg.budget for f in want) + (len(want[3]) > seg.budget)
                assert seg.second_copies == long_files
                if budget == 64:
                    assert seg.budget == 64 and seg.second_copies == 6   # every frame took the second copy
                elif budget is None:
                    assert seg.budget == max(raw // 4, 1024)
                else:
                    assert seg.budget == seg.capacity and seg.second_copies == 0
                # submit / result by hand, more frames than slots before the first result
                for f in frames[:depth + 2]:
                    seg.submit(f)
                assert [seg.result() for _ in range(depth + 2)] == want[:depth + 2]
        mode, img = C.decode(want[0])
        assert img.shape == arrays[0].shape


def test_segmenter_jpeg_refuses_bad_arguments_and_survives_an_exception():
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_vgg()
    good = camera_frames(1, h, w, seed=5)[0]
    for bad in (dict(encode="png"), dict(encode="jpeg", quality=0), dict(encode="jpeg", quality=101),
                dict(encode="jpeg", quality=90.0), dict(encode="jpeg", budget=0), dict(budget=100)):
        with pytest.raises(ValueError):
            FrameSegmenter(net, h, w, **bad)
    with FrameSegmenter(net, h, w, depth=2, encode="jpeg", quality=75) as seg:
        want = seg.apply(good)
        assert want == J.encode(definition(net, good), 75)
        with pytest.raises(ValueError):
            seg.submit(good[:-1])
        forward = net.forward
        net.forward = lambda x: (_ for _ in ()).throw(KeyError("no such layer"))
        try:
            with pytest.raises(KeyError):
                seg.submit(good)
        finally:
            del net.forward
        assert net.forward == forward and seg.pending == 0 and net.compute_side_outputs is True
        assert seg.apply(good) == want
    with pytest.raises(RuntimeError):
        seg.submit(good)  # closed


def test_run_webcam_writes_the_device_files(tmp_path):
    import run_webcam
    net, (h, w) = small_vgg()
    ckpt = tmp_path / "vgg.pth"
    torch.save(O.make_state_dict(2), str(ckpt))
    out = tmp_path / "out"
    rates = run_webcam.main(["--variant", "vgg", "--model", str(ckpt), "--synthetic", "3", "--height", str(h), "--width", str(w),
                             "--output", str(out), "--output-format", "jpeg", "--jpeg-quality", "80"])
    assert len(rates) == 3 and sorted(p.name for p in out.iterdir()) == ["%05d.jpg" % k for k in range(3)]
    for k in range(3):
        want = J.encode(definition(net, run_webcam.synthetic_frame(h, w, k)), 80)
        assert (out / ("%05d.jpg" % k)).read_bytes() == want
