"""The 4:2:0 form of the device JPEG encoder on a real MI355X (csrc/jpeg.hip through ``ops.jpeg_encode(...,
subsampling='4:2:0')``) against the integer statement of its layout (util/jpeg_layout.py) - byte for byte, so no tolerance
anywhere - then ``FrameSegmenter(encode='jpeg', subsampling='4:2:0')`` and ``run_webcam --output x.avi`` end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg420_cases as C4  # noqa: E402
import jpeg_cases as C  # noqa: E402
from avi_parse import parse_avi  # noqa: E402
from util import jpeg_layout as J  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
S = "4:2:0"


def dirty_workspace():
    from fosvos_hip import ops
    torch.cuda.synchronize()
    for buf in ops._WS._buf.values():
        buf.fill_(FILL)


def encode_checked(frames, quality, want, view=False):
    """ops.jpeg_encode(4:2:0) of uint8 [N,H,W,3] into a buffer filled with 0xA5; checks files, lengths and the untouched tail.
    ``view``: the frames start one byte into their allocation."""
    from fosvos_hip import ops
    n, h, w = frames.shape[:3]
    cap = ops.jpeg_capacity(h, w, 3, S)
    assert cap == J.capacity(h, w, 3, S)
    if view:
        store = torch.zeros((frames.size + 1,), dtype=torch.uint8, device=DEV)
        x = store[1:].view(frames.shape)
        x.copy_(torch.from_numpy(frames))
    else:
        x = torch.from_numpy(frames).to(DEV)
    out = torch.full((n, cap + 5), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    dirty_workspace()
    got_out, got_len = ops.jpeg_encode(x, quality, out=out, lengths=lengths, subsampling=S)
    assert got_out is out and got_len is lengths
    torch.cuda.synchronize()
    buf, lens = out.cpu().numpy(), lengths.cpu().tolist()
    for k in range(n):
        ref = want[k]
        print("frame %d of %s q=%d: %d bytes, the layout %d" % (k, frames.shape, quality, lens[k], len(ref)))
        assert lens[k] == len(ref), (k, frames.shape, quality, lens[k], len(ref))
        got = buf[k, :lens[k]].tobytes()
        if got != ref:
            at = next(i for i in range(len(ref)) if got[i] != ref[i])
            raise AssertionError("frame %d of %s at q=%d differs from the layout at byte %d of %d"
                                 % (k, frames.shape, quality, at, len(ref)))
        assert (buf[k, lens[k]:] == FILL).all(), "bytes behind the file were written"


@pytest.mark.parametrize("size", C4.SIZES, ids=lambda s: "%dx%d" % s)
def test_jpeg420_is_the_layout_byte_for_byte(size):
    h, w = size
    for content in C4.CONTENTS:
        frame = C4.make(content, h, w)
        for q in C4.QUALITIES:
            want = [J.encode(frame, q, subsampling=S)]
            encode_checked(frame[None], q, want)
            if q == 90:
                encode_checked(frame[None], q, want, view=True)


def test_jpeg420_batch_of_three():
    frames = C4.batch()
    for q in C4.QUALITIES:
        want = [J.encode(f, q, subsampling=S) for f in frames]
        assert len({len(f) for f in want}) == 3
        encode_checked(frames, q, want)
        encode_checked(frames, q, want, view=True)


def test_jpeg420_workload_frame_once():
    frame = C4.workload_frame()
    encode_checked(frame[None], 90, [J.encode(frame, 90, subsampling=S)])


def test_jpeg420_views_with_slack_and_repeat():
    from fosvos_hip import ops
    frames = C4.batch()
    n, h, w = frames.shape[:3]
    x = torch.from_numpy(frames).to(DEV)
    want = [J.encode(f, 90, subsampling=S) for f in frames]
    cap = ops.jpeg_capacity(h, w, 3, S)
    for lead, stride in ((1, cap + 3), (0, cap), (3, cap + 2)):
        room = lead + n * stride
        room += -room % 4
        store = torch.full((room + 4 * n + 8,), FILL, dtype=torch.uint8, device=DEV)
        out = store[lead:lead + n * stride].view(n, stride)
        lengths = store[room:room + 4 * n].view(torch.int32)
        ops.jpeg_encode(x, 90, out=out, lengths=lengths, subsampling=S)
        torch.cuda.synchronize()
        host = store.cpu().numpy()
        assert lengths.cpu().tolist() == [len(f) for f in want]
        keep = np.ones(host.size, dtype=bool)
        for k, f in enumerate(want):
            at = lead + k * stride
            assert host[at:at + len(f)].tobytes() == f, (lead, stride, k)
            keep[at:at + len(f)] = False
        keep[room:room + 4 * n] = False
        assert (host[keep] == FILL).all()            # the slack of every row and everything else is untouched
        dirty_workspace()
        ops.jpeg_encode(x, 90, out=out, lengths=lengths, subsampling=S)   # a second launch into the same buffers
        torch.cuda.synchronize()
        assert np.array_equal(store.cpu().numpy(), host)


def test_444_and_grey_are_what_they_were():
    from fosvos_hip import LaunchProfile, ops
    frames = np.stack([C.picture(61, 107), C.noise(61, 107), C.smooth(61, 107)])
    x = torch.from_numpy(frames).to(DEV)
    for q in (50, 100):
        with LaunchProfile(0) as prof:
            a_out, a_len = ops.jpeg_encode(x, q)
            b_out, b_len = ops.jpeg_encode(x, q, subsampling="4:4:4")
        assert prof.records["k_jpeg_measure"]["launches"] == 2 and prof.records["k_jpeg_emit"]["launches"] == 2
        assert not any(name.endswith("_420") for name in prof.records)
        torch.cuda.synchronize()
        assert a_out.shape == b_out.shape == (3, J.capacity(61, 107, 3)) and torch.equal(a_len, b_len)
        for k, f in enumerate(frames):
            n = int(a_len[k])
            assert a_out[k, :n].cpu().numpy().tobytes() == b_out[k, :n].cpu().numpy().tobytes() == J.encode(f, q)
    assert ops.jpeg_capacity(61, 107, 3) == ops.jpeg_capacity(61, 107, 3, "4:4:4") == J.capacity(61, 107, 3)
    grey = torch.from_numpy(np.stack([C.picture(33, 47, True), C.noise(33, 47, True)])).to(DEV)
    assert ops.jpeg_capacity(33, 47, 1, S) == ops.jpeg_capacity(33, 47, 1) == J.capacity(33, 47, 1)
    with LaunchProfile(0) as prof:
        a_out, a_len = ops.jpeg_encode(grey, 90, subsampling=S)
        b_out, b_len = ops.jpeg_encode(grey, 90, subsampling="4:4:4")
    assert prof.records["k_jpeg_measure_grey"]["launches"] == 2 and not any(name.endswith("_420") for name in prof.records)
    torch.cuda.synchronize()
    assert torch.equal(a_len, b_len) and a_out.shape == b_out.shape
    for k in range(2):
        n = int(a_len[k])
        assert a_out[k, :n].cpu().numpy().tobytes() == b_out[k, :n].cpu().numpy().tobytes() == J.encode(grey[k].cpu().numpy(), 90)


def test_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    L = lib()
    n, h, w = 2, 24, 40
    cap, need = L.fosvos_jpeg_capacity_bytes(n, h, w, 3, 420), L.fosvos_jpeg_workspace_bytes(n, h, w, 3, 420)
    assert cap == J.capacity(h, w, 3, S) and need == n * J.n_intervals(h, w, S) * 4
    assert L.fosvos_jpeg_capacity_bytes(n, h, w, 3, 444) == J.capacity(h, w, 3, "4:4:4")
    assert L.fosvos_jpeg_workspace_bytes(n, h, w, 3, 444) == J.n_intervals(h, w) * 4 * n
    assert L.fosvos_jpeg_capacity_bytes(1, 1080, 1920, 3, 420) == J.capacity(1080, 1920, 3, S)
    assert L.fosvos_jpeg_capacity_bytes(1, 8, 8, 3, 422) == 0 and L.fosvos_jpeg_workspace_bytes(1, 8, 8, 3, 0) == 0
    assert L.fosvos_jpeg_capacity_bytes(1, 0, 8, 3, 420) == 0 and L.fosvos_jpeg_capacity_bytes(1, 8, 8, 2, 420) == 0
    x = torch.from_numpy(np.stack([C4.ramp(h, w)] * n)).to(DEV)
    out = torch.full((n, cap), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.full((need,), FILL, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(s=420, q=90, c=cap, nb=need, c_=3):
        return L.fosvos_jpeg_encode(x.data_ptr(), n, h, w, c_, s, q, out.data_ptr(), c, lengths.data_ptr(), ws.data_ptr(), nb, 0, st)

    with LaunchProfile(0) as prof:
        assert call(s=422) == -2 and b"sampling" in L.fosvos_last_error()
        assert call(s=0) == -2 and call(s=2) == -2
        assert call(nb=need - 1) == -3 and b"workspace" in L.fosvos_last_error()      # a short workspace
        assert call(c=cap - 1) == -3 and b"out_stride" in L.fosvos_last_error()       # a short out
        assert call(q=0) == -2 and call(c_=2) == -1
        for bad in (lambda: ops.jpeg_encode(x, 90, subsampling="4:2:2"), lambda: ops.jpeg_encode(x, 90, subsampling="420"),
                    lambda: ops.jpeg_encode(x, 90, subsampling=None), lambda: ops.jpeg_capacity(h, w, 3, "4:1:1"),
                    lambda: ops.jpeg_encode(x, out=out[:, :cap - 1].contiguous(), subsampling=S),
                    lambda: ops.jpeg_encode(x, out=out[:1], subsampling=S),
                    lambda: ops.jpeg_encode(x, lengths=lengths[:1], subsampling=S)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.jpeg_encode(x.cpu(), subsampling=S), lambda: ops.jpeg_encode(x, out=out.cpu(), subsampling=S),
                    lambda: ops.jpeg_encode(x, lengths=lengths.cpu(), subsampling=S)):
            with pytest.raises(RuntimeError):
                bad()
    assert not any(name.startswith("k_jpeg") for name in prof.records), prof.records
    torch.cuda.synchronize()
    assert (out == FILL).all() and (lengths == -1).all() and (ws == FILL).all()  # none of the refused calls wrote anything
    with LaunchProfile(0) as prof:
        assert call() == 0
    assert prof.records["k_jpeg_measure_420"]["launches"] == 1 and prof.records["k_jpeg_emit_420"]["launches"] == 1
    assert set(name for name in prof.records if name.startswith("k_jpeg")) == {"k_jpeg_measure_420", "k_jpeg_emit_420"}
    want = J.encode(C4.ramp(h, w), 90, subsampling=S)
    assert lengths.cpu().tolist() == [len(want)] * 2 and out[1, :len(want)].cpu().numpy().tobytes() == want


# ------------------------------------------------------------------------------- FrameSegmenter(encode='jpeg', subsampling='4:2:0')
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


def test_segmenter_420_is_the_layout_of_the_arrays():
    from fosvos_hip.stream import FrameSegmenter
    net, (h, w) = small_vgg()
    frames = camera_frames(4, h, w, seed=11)
    with FrameSegmenter(net, h, w, depth=2) as seg:                       # encode=None: the arrays
        arrays = list(seg.segment(frames))
    want = [J.encode(a, 90, subsampling=S) for a in arrays]
    assert len(set(want)) == 4 and all(len(f) > 64 for f in want)
    for depth, budget in ((1, None), (2, None), (2, 64)):
        with FrameSegmenter(net, h, w, depth=depth, encode="jpeg", quality=90, subsampling=S, budget=budget) as seg:
            assert seg.subsampling == S and seg.capacity == J.capacity(h, w, 3, S)
            got = list(seg.segment(iter(frames)))
            assert all(isinstance(g, bytes) for g in got) and got == want, (depth, budget)
            if budget == 64:
                assert seg.budget == 64 and seg.second_copies == 4        # every frame took the second copy
            else:
                assert seg.budget == max(h * w * 3 // 4, 1024)            # the default stays a quarter of the raw size
    with FrameSegmenter(net, h, w, depth=2, encode="jpeg", quality=90) as seg:
        assert seg.subsampling == "4:4:4" and seg.apply(frames[0]) == J.encode(arrays[0], 90)
    for bad in (dict(subsampling=S), dict(encode="jpeg", subsampling="4:2:2"), dict(encode="jpeg", subsampling=None)):
        with pytest.raises(ValueError):
            FrameSegmenter(net, h, w, **bad)


def test_run_webcam_avi_holds_the_files_of_the_directory_run(tmp_path):
    import run_webcam
    net, (h, w) = small_vgg()
    ckpt = tmp_path / "vgg.pth"
    torch.save(O.make_state_dict(2), str(ckpt))
    common = ["--variant", "vgg", "--model", str(ckpt), "--synthetic", "4", "--height", str(h), "--width", str(w),
              "--output-format", "jpeg", "--jpeg-subsampling", "420"]
    assert len(run_webcam.main(common + ["--output", str(tmp_path / "x.avi")])) == 4
    assert len(run_webcam.main(common + ["--output", str(tmp_path / "dir")])) == 4
    files = [(tmp_path / "dir" / ("%05d.jpg" % k)).read_bytes() for k in range(4)]
    got = parse_avi((tmp_path / "x.avi").read_bytes())
    assert got["frames"] == files and (got["width"], got["height"]) == (w, h) and len(set(files)) == 4
    for f in files:
        mode, img = C.decode(f)
        assert mode == "RGB" and img.shape == (h, w, 3)
        assert f[:J.header_bytes(3)] == J.header(h, w, 3, 90, S)
