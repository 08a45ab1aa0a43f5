"""fosvos_jpeg_decode (csrc/jpeg_decode.hip) on the card: byte for byte util/jpeg_read.decode and PIL on the files of
tests/jpeg_read_cases.py, batches, views and side streams, damaged files, refused arguments - then the consumers: the
device-decode loader against ``get_data_loader_test``, ``test_fast`` and ``run_webcam`` with and without the flag."""
import functools
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

import jpeg_cases as J  # noqa: E402
import jpeg_read_cases as C  # noqa: E402
from util import experiment_helper, io_helper, jpeg_read as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
MARGIN = 4096


@functools.lru_cache(maxsize=None)
def reference(data):
    """(the definition's pixels, its status) - computed once per file."""
    return R.decode(data)


def groups():
    """The case files by (height, width, components, sampling): the files of one call."""
    out = {}
    for name, data in C.cases():
        p = R.probe(data)
        out.setdefault((p.height, p.width, p.components, p.subsampling), []).append((name, data))
    return out


GROUPS = groups()


@pytest.mark.parametrize("key", sorted(GROUPS), ids=lambda k: "%dx%d_c%d_%s" % (k[0], k[1], k[2], k[3].replace(":", "")))
def test_decode_is_the_definition_and_pil_byte_for_byte(key):
    from fosvos_hip import ops
    files = [d for _, d in GROUPS[key]]
    frames, status = ops.jpeg_decode(files)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (len(files),) + key[:2] + ((3,) if key[2] == 3 else ())
    assert status.cpu().tolist() == [0] * len(files)
    got = frames.cpu().numpy()
    for k, (name, data) in enumerate(GROUPS[key]):
        want, st = reference(data)
        assert st == 0
        assert np.array_equal(got[k], want), (name, int((got[k] != want).sum()))
        assert np.array_equal(got[k], C.pil_pixels(data)), name


def test_every_case_is_in_a_group():
    assert sum(len(v) for v in GROUPS.values()) == len(C.cases()) == 202


def test_batches_five_files_and_one_two_thirteen_segments():
    from fosvos_hip import ops
    five = [C.pil_file(J.picture(61, 107), 90, "420"), C.pil_file(J.noise(61, 107), 100, "420"), C.pil_file(J.smooth(61, 107), 50, "420", 16),
            C.pil_file(J.checker(61, 107), 100, "420"), C.pil_file(J.noise(61, 107, seed=4), 30, "420", optimize=True)]
    assert len(set(five)) == 5
    frames, status = ops.jpeg_decode(five)
    assert status.cpu().tolist() == [0] * 5
    for k, data in enumerate(five):
        assert np.array_equal(frames[k].cpu().numpy(), reference(data)[0]) and np.array_equal(reference(data)[0], C.pil_pixels(data))
    img = J.picture(*J.MANY)
    mixed = [C.pil_file(img, 90, "444", 0), C.pil_file(img, 50, "444", 203), C.pil_file(img, 100, "444", 32)]
    assert [len(R.probe(d).segments) for d in mixed] == [1, 2, 13]
    frames, status = ops.jpeg_decode(mixed)
    assert status.cpu().tolist() == [0] * 3
    for k, data in enumerate(mixed):
        assert np.array_equal(frames[k].cpu().numpy(), C.pil_pixels(data))


def test_davis_sized_frame_once():
    from fosvos_hip import ops
    data = C.big_file()
    frames, status = ops.jpeg_decode([data, data])
    assert status.cpu().tolist() == [0, 0]
    want = C.pil_pixels(data)
    assert np.array_equal(frames[0].cpu().numpy(), want) and np.array_equal(frames[1].cpu().numpy(), want)


def test_views_side_stream_repeat_and_sentinels():
    from fosvos_hip import ops
    files = [d for _, d in GROUPS[(61, 107, 3, "4:2:0")]][:4]
    n, h, w = len(files), 61, 107
    store = torch.full((MARGIN + n * h * w * 3 + MARGIN,), FILL, dtype=torch.uint8, device=DEV)
    codes = torch.full((3 + n + 3,), -7, dtype=torch.int32, device=DEV)
    out = store[MARGIN:MARGIN + n * h * w * 3].view(n, h, w, 3)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, st = ops.jpeg_decode(files, out=out, status=codes[3:3 + n])
        assert got.data_ptr() == out.data_ptr() and st.data_ptr() == codes[3:3 + n].data_ptr()
        first = out.clone()
        ops.jpeg_decode(files, out=out, status=codes[3:3 + n])
    side.synchronize()
    assert torch.equal(first, out)
    assert codes.cpu().tolist() == [-7] * 3 + [0] * n + [-7] * 3
    assert (store[:MARGIN] == FILL).all() and (store[-MARGIN:] == FILL).all()
    for k, data in enumerate(files):
        assert np.array_equal(out[k].cpu().numpy(), reference(data)[0])
    assert ops.jpeg_decode_workspace(n, h, w, 3, "4:2:0") > 0


def raw_decode(files, workspace_bytes=None, status_fill=-7):
    """The raw binding with sentinel bytes round the frames, the status words and the workspace."""
    from fosvos_hip import lib, ops
    L = lib()
    plans = [R.probe(f) for f in files]
    p = plans[0]
    n, h, w, c = len(files), p.height, p.width, p.components
    sampling = R.SAMPLING_CODE[p.subsampling]
    need = int(L.fosvos_jpeg_decode_workspace_bytes(n, h, w, c, sampling))
    host, n_seg, off_tables, off_bytes, n_bytes = ops.jpeg_decode_pack(files, plans)
    buf = host.to(DEV)
    frame_bytes = n * h * w * c
    frames = torch.full((MARGIN + frame_bytes + MARGIN,), FILL, dtype=torch.uint8, device=DEV)
    ws = torch.full((MARGIN + need + MARGIN,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((4 + n + 4,), status_fill, dtype=torch.int32, device=DEV)
    rc = L.fosvos_jpeg_decode(buf.data_ptr() + off_bytes, n_bytes, buf.data_ptr(), n_seg, buf.data_ptr() + off_tables, n, h, w, c,
                              sampling, frames.data_ptr() + MARGIN, status.data_ptr() + 16, ws.data_ptr() + MARGIN,
                              need if workspace_bytes is None else workspace_bytes, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = bool((frames[:MARGIN] == FILL).all() and (frames[-MARGIN:] == FILL).all() and (ws[:MARGIN] == FILL).all()
                  and (ws[-MARGIN:] == FILL).all() and (status[:4] == status_fill).all() and (status[-4:] == status_fill).all())
    shape = (n, h, w, 3) if c == 3 else (n, h, w)
    return rc, frames[MARGIN:MARGIN + frame_bytes].view(shape).cpu().numpy(), status[4:4 + n].cpu().tolist(), intact, (frames, ws, status)


def test_sentinels_round_frames_workspace_and_status():
    for key in ((7, 9, 1, "4:4:4"), (33, 47, 3, "4:4:4"), (16, 5, 3, "4:2:0"), (61, 107, 3, "4:2:0")):
        files = [d for _, d in GROUPS[key]][:3]
        rc, frames, status, intact, _ = raw_decode(files)
        assert rc == 0 and status == [0, 0, 0] and intact, key
        for k, data in enumerate(files):
            assert np.array_equal(frames[k], reference(data)[0]), key


@pytest.mark.parametrize("which", range(3), ids=[d[0] for d in C.damaged()])
def test_damaged_file_between_two_good_ones(which):
    name, bad, want = C.damaged()[which]
    p = R.probe(bad)
    good = [d for _, d in GROUPS[(p.height, p.width, p.components, p.subsampling)]]
    files = [good[0], bad, good[-1]]
    assert reference(bad)[1] == want
    rc, frames, status, intact, _ = raw_decode(files)
    assert rc == 0 and status == [0, want, 0] and intact
    assert np.array_equal(frames[0], reference(files[0])[0]) and np.array_equal(frames[2], reference(files[2])[0])
    from fosvos_hip import ops
    _, st = ops.jpeg_decode(files)
    assert st.cpu().tolist() == [0, want, 0]


def test_bad_arguments_raise_and_launch_nothing():
    from fosvos_hip import LaunchProfile, lib, ops
    L = lib()
    a = [d for _, d in GROUPS[(33, 47, 3, "4:4:4")]][:2]
    b = [d for _, d in GROUPS[(33, 47, 3, "4:2:0")]][:1]
    g = [d for _, d in GROUPS[(33, 47, 1, "4:4:4")]][:1]
    other = [d for _, d in GROUPS[(61, 107, 3, "4:4:4")]][:1]
    progressive = C.pil_file(J.picture(33, 47), 90, progressive=True)
    assert L.fosvos_jpeg_decode_workspace_bytes(1, 16, 4, 3, 420) == 0 and L.fosvos_jpeg_decode_workspace_bytes(1, 16, 4, 3, 444) > 0
    assert L.fosvos_jpeg_decode_workspace_bytes(1, 8, 8, 2, 444) == 0 and L.fosvos_jpeg_decode_workspace_bytes(1, 8, 8, 3, 422) == 0
    assert L.fosvos_jpeg_decode_workspace_bytes(0, 8, 8, 3, 444) == 0 and L.fosvos_jpeg_decode_workspace_bytes(1, 0, 8, 3, 444) == 0
    out = torch.full((2, 33, 47, 3), FILL, dtype=torch.uint8, device=DEV)
    with LaunchProfile(0) as prof:
        for bad in (lambda: ops.jpeg_decode(a + other), lambda: ops.jpeg_decode(a + b), lambda: ops.jpeg_decode(a + g),
                    lambda: ops.jpeg_decode([a[0], progressive]), lambda: ops.jpeg_decode([b"not a file"]), lambda: ops.jpeg_decode([]),
                    lambda: ops.jpeg_decode(a, out=out[:1]), lambda: ops.jpeg_decode(a, out=out.view(2, 33, 3, 47)),
                    lambda: ops.jpeg_decode(a, status=torch.zeros(3, dtype=torch.int32, device=DEV)),
                    lambda: ops.jpeg_decode(a, status=torch.zeros(2, dtype=torch.int64, device=DEV)),
                    lambda: ops.jpeg_decode_workspace(1, 16, 4, 3, "4:2:0"), lambda: ops.jpeg_decode_workspace(1, 8, 8, 3, "4:2:2")):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ops.jpeg_decode(a, out=out.cpu()), lambda: ops.jpeg_decode(a, status=torch.zeros(2, dtype=torch.int32)),
                    lambda: ops.jpeg_decode(a, device="cpu")):
            with pytest.raises(RuntimeError):
                bad()
        if torch.cuda.device_count() > 1:
            with pytest.raises(RuntimeError):
                ops.jpeg_decode(a, out=out, device="cuda:1")
        need = int(L.fosvos_jpeg_decode_workspace_bytes(2, 33, 47, 3, 444))
        rc, _, status, intact, _ = raw_decode(a, workspace_bytes=need - 1)            # a short workspace
        assert rc == -3 and b"workspace" in L.fosvos_last_error() and status == [-7, -7] and intact
    assert not any(name.startswith("k_jpegd") for name in prof.records), prof.records
    assert (out == FILL).all()
    with LaunchProfile(0) as prof:
        ops.jpeg_decode(a, out=out)
    assert {n: r["launches"] for n, r in prof.records.items() if n.startswith("k_jpegd")} == \
        {"k_jpegd_entropy": 1, "k_jpegd_idct": 1, "k_jpegd_color": 1}
    assert np.array_equal(out[1].cpu().numpy(), reference(a[1])[0])


# ------------------------------------------------------------------------------------------ the consumers
H, W = 48, 86


def davis_tree(root, files, seq="blob"):
    """A DAVIS tree of ``files`` ([(suffix, bytes)]) with the first frame's annotation."""
    (root / "ImageSets" / "480p").mkdir(parents=True)
    (root / "JPEGImages" / "480p" / seq).mkdir(parents=True)
    (root / "Annotations" / "480p" / seq).mkdir(parents=True)
    lines = []
    for k, data in enumerate(files):
        (root / "JPEGImages" / "480p" / seq / ("%05d.jpg" % k)).write_bytes(data)
        lines.append("/JPEGImages/480p/%s/%05d.jpg /Annotations/480p/%s/%05d.png" % (seq, k, seq, k))
    for name in ("trainval.txt", "val.txt", "train.txt"):
        (root / "ImageSets" / "480p" / name).write_text("\n".join(lines) + "\n")
    y, x = np.mgrid[0:H, 0:W]
    mask = (((y - H / 2) ** 2 + (x - W / 2) ** 2) < (H / 3) ** 2).astype(np.uint8) * 255
    Image.fromarray(mask).save(str(root / "Annotations" / "480p" / seq / "00000.png"))
    return root


def frame_files(count, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        img = J.picture(H, W).astype(np.int32) + rng.integers(-20, 21, (H, W, 3)) + 8 * k
        out.append(C.pil_file(np.clip(img, 0, 255).astype(np.uint8), 92, "420"))
    return out


def file_422(seed=9):
    import io
    b = io.BytesIO()
    Image.fromarray(J.noise(H, W, seed=seed)[..., ::-1].copy()).save(b, "JPEG", quality=92, subsampling=1)
    return b.getvalue()


def drain(loader):
    """[('batch', dict) ... ('raised', type)]: what the loader yields, up to and including its first exception."""
    out, it = [], iter(loader)
    while True:
        try:
            out.append(("batch", next(it)))
        except StopIteration:
            return out
        except Exception as e:  # noqa: BLE001 - whatever the host path raises is the yardstick
            out.append(("raised", type(e).__name__))
            return out


def same_batches(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (kind, a), (_, b) in zip(got, want):
        if kind == "raised":
            assert a == b
            continue
        assert sorted(a) == sorted(b) == ["fname", "gt", "image", "seq_name"]
        assert list(a["fname"]) == list(b["fname"]) and list(a["seq_name"]) == list(b["seq_name"])
        assert a["image"].is_cuda and a["image"].dtype == b["image"].dtype == torch.float32 and a["image"].shape == b["image"].shape
        assert torch.equal(a["image"].cpu(), b["image"]), a["fname"]
        assert not a["gt"].is_cuda and a["gt"].dtype == b["gt"].dtype and torch.equal(a["gt"], b["gt"])


def test_loader_yields_the_host_loaders_minibatches(tmp_path):
    files = frame_files(7)
    files[3] = file_422()
    at = C.scan_start(files[5])
    files[5] = files[5][:at + (len(files[5]) - 2 - at) // 2] + b"\xff\xd9"           # a scan cut in half
    assert R.probe(files[3]) is None and R.probe(files[5]) is not None and R.decode(files[5])[1] == 1
    root = davis_tree(tmp_path / "davis", files)
    want = drain(io_helper.get_data_loader_test(root, 1, "blob"))
    loader = io_helper.get_data_loader_test(root, 1, "blob", device_decode=True)
    assert len(loader) == 7 and len(loader.dataset) == 7
    got = drain(loader)
    same_batches(got, want)
    assert len(got) >= 6                                   # five frames and frame 5's fate (PIL raises, or decodes what is there)
    # a window of three files a launch: windows end inside runs, the same minibatches
    from dataloaders.device_decode import DeviceDecodeLoader
    small = DeviceDecodeLoader(loader.dataset, files_per_launch=3)
    held = drain(small)                                    # the tensors stay valid while held
    same_batches(held, want)
    assert small.decoded >= 4 and small.fallbacks >= 1
    from dataloaders.davis_2016 import DAVIS2016
    with pytest.raises(ValueError):
        DeviceDecodeLoader(DAVIS2016(mode="test", db_root_dir=str(root), seq_name="blob", inputRes=(24, 43)))
    with pytest.raises(ValueError):
        io_helper.get_data_loader_test(root, 1, "blob", synthetic=(H, W), device_decode=True)


class Provider:
    def __init__(self, network):
        self.network = network


_NET = []


def small_vgg():
    if not _NET:
        from networks.osvos_vgg import OSVOS_VGG
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(2))
        _NET.append(net.to(DEV).eval())
    return _NET[0]


def test_fast_pass_writes_the_same_files_and_scores(tmp_path):
    files = frame_files(5, seed=1)
    files[2] = file_422()
    root = davis_tree(tmp_path / "davis", files)
    prov = Provider(small_vgg())
    results = []
    for flag in (False, True):
        loader = io_helper.get_data_loader_test(root, 1, "blob", device_decode=True) if flag else io_helper.get_data_loader_test(root, 1, "blob")
        out = tmp_path / ("fast_%d" % flag)
        score = experiment_helper.test_fast(prov, loader, out, io_helper.get_annotations(root, loader), seq_name="blob")
        results.append((score, {p.name: p.read_bytes() for p in sorted((out / "blob").iterdir())}))
        if flag:
            assert loader.decoded == 4 and loader.fallbacks == 1
    assert sorted(results[0][1]) == ["%05d.png" % k for k in range(5)]
    assert results[0][1] == results[1][1]
    timing = ("seconds",)
    assert repr({k: v for k, v in results[0][0].items() if k not in timing}) == \
        repr({k: v for k, v in results[1][0].items() if k not in timing})
    assert results[0][0]["scored"] == [True, False, False, False, False]


def test_run_webcam_directory_with_and_without_the_flag(tmp_path):
    import run_webcam
    small_vgg()
    ckpt = tmp_path / "vgg.pth"
    torch.save(O.make_state_dict(2), str(ckpt))
    src = tmp_path / "src"
    src.mkdir()
    files = frame_files(5, seed=2)
    files[1] = file_422()
    for k, data in enumerate(files):
        (src / ("%05d.jpg" % k)).write_bytes(data)
    Image.fromarray(J.noise(H, W)[..., ::-1].copy()).save(str(src / "00005.png"))
    common = ["--variant", "vgg", "--model", str(ckpt), "--source", str(src), "--output-format", "jpeg"]
    assert len(run_webcam.main(common + ["--output", str(tmp_path / "host")])) == 6
    assert len(run_webcam.main(common + ["--output", str(tmp_path / "device"), "--device-decode"])) == 6
    host = {p.name: p.read_bytes() for p in sorted((tmp_path / "host").iterdir())}
    assert sorted(host) == ["%05d.jpg" % k for k in range(6)] and len(set(host.values())) == 6
    assert host == {p.name: p.read_bytes() for p in sorted((tmp_path / "device").iterdir())}


def test_avi_of_the_device_encoder_reads_back_through_the_device_decoder(tmp_path):
    import run_webcam
    from fosvos_hip import ops
    from util.mjpeg_avi import AviWriter
    h, w = 56, 90                                           # 4 x 6 MCUs of 16 x 16: two restart intervals a file
    frames = np.stack([J.picture(h, w), J.noise(h, w), J.smooth(h, w)])
    out, lengths = ops.jpeg_encode(torch.from_numpy(frames).to(DEV), 90, subsampling="4:2:0")
    payloads = [out[k, :n].cpu().numpy().tobytes() for k, n in enumerate(lengths.cpu().tolist())]
    assert all(len(R.probe(p).segments) == 2 for p in payloads)
    with AviWriter(tmp_path / "x.avi", w, h, 25) as avi:
        for p in payloads:
            avi.write(p)
    got = list(run_webcam.device_decoded_frames(run_webcam.source_items(str(tmp_path / "x.avi"))))
    assert len(got) == 3 and all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
    for g, p in zip(got, payloads):
        assert np.array_equal(g.cpu().numpy(), C.pil_pixels(p))
    common = ["--no-network", "--no-mirror", "--source", str(tmp_path / "x.avi")]
    assert len(run_webcam.main(common + ["--output", str(tmp_path / "device"), "--device-decode"])) == 3
    assert len(run_webcam.main(common + ["--output", str(tmp_path / "host")])) == 3
    for k, p in enumerate(payloads):
        want = C.pil_pixels(p)
        for d in ("device", "host"):
            png = np.asarray(Image.open(str(tmp_path / d / ("%05d.png" % k))))
            assert np.array_equal(png[..., ::-1], want), (d, k)
