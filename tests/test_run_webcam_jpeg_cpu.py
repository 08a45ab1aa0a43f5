"""The JPEG options of run_webcam: parsing, the rejected combinations, the default being the call sequence it was, and what the
loop writes.  The net and the segmenter are stubs.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_cases as C  # noqa: E402
from util import jpeg_layout as J  # noqa: E402


class StubNet:
    def cuda(self):
        return self

    def eval(self):
        return self


class StubSegmenter:
    """Records how it was built; returns every frame as it came - or, with encode='jpeg', the layout's file of it."""
    built = []

    def __init__(self, net, height, width, **kw):
        StubSegmenter.built.append(((type(net).__name__, height, width), kw))
        self.kw = kw

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def segment(self, frames):
        for f in frames:
            yield J.encode(f, self.kw["quality"]) if self.kw.get("encode") == "jpeg" else f


@pytest.fixture
def stubbed(monkeypatch):
    import run_webcam
    from fosvos_hip import stream
    StubSegmenter.built = []
    monkeypatch.setattr(run_webcam, "get_network", lambda *a, **k: StubNet())
    monkeypatch.setattr(stream, "FrameSegmenter", StubSegmenter)
    return run_webcam


def test_options_parse_and_default_to_png():
    import run_webcam
    p = run_webcam.build_parser()
    a = p.parse_args([])
    assert a.output_format == "png" and a.jpeg_quality == 90
    a = p.parse_args(["--output-format", "jpeg", "--jpeg-quality", "75", "--output", "x"])
    assert a.output_format == "jpeg" and a.jpeg_quality == 75 and a.output == "x"
    for bad in (["--output-format", "gif"], ["--jpeg-quality", "high"], ["--output-form", "jpeg"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_jpeg_needs_an_output_directory_and_a_quality_in_range(stubbed, tmp_path):
    with pytest.raises(ValueError, match="--output"):
        stubbed.main(["--synthetic", "1", "--output-format", "jpeg"])
    with pytest.raises(ValueError, match="--output"):
        stubbed.main(["--synthetic", "1", "--no-network", "--output-format", "jpeg"])
    for q in ("0", "101"):
        with pytest.raises(ValueError, match="quality"):
            stubbed.main(["--synthetic", "1", "--output-format", "jpeg", "--jpeg-quality", q, "--output", str(tmp_path)])
    assert StubSegmenter.built == [] and list(tmp_path.iterdir()) == []


def test_default_is_the_call_sequence_it_was(stubbed, tmp_path):
    common = ["--variant", "vgg", "--synthetic", "2", "--height", "10", "--width", "14", "--depth", "3", "--no-mirror", "-oc", "g"]
    was = dict(depth=3, mirror=False, overlay=True, boolean_mask=True, color="g", alpha=1.0)
    stubbed.main(common + ["--output", str(tmp_path / "a")])
    stubbed.main(common + ["--output", str(tmp_path / "b"), "--output-format", "png", "--jpeg-quality", "30"])
    stubbed.main(common)
    assert StubSegmenter.built == [(("StubNet", 10, 14), was)] * 3          # no new argument reaches the segmenter
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["00000.png", "00001.png"]
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["00000.png", "00001.png"]


def test_jpeg_writes_the_returned_bytes_without_pil(stubbed, tmp_path, monkeypatch):
    def no_png(*a, **k):
        raise AssertionError("the PNG writer ran with --output-format jpeg")

    monkeypatch.setattr(stubbed, "write_png", no_png)
    monkeypatch.setattr(stubbed, "write_jpeg_host", no_png)
    monkeypatch.setitem(sys.modules, "PIL", None)       # `import PIL` / `from PIL import ...` now raise ImportError
    monkeypatch.setitem(sys.modules, "PIL.Image", None)
    rates = stubbed.main(["--variant", "vgg", "--synthetic", "3", "--height", "10", "--width", "14", "--output", str(tmp_path),
                          "--output-format", "jpeg", "--jpeg-quality", "60"])
    assert len(rates) == 3
    (net, kw), = StubSegmenter.built
    assert kw == dict(depth=2, mirror=True, overlay=True, boolean_mask=True, color="r", alpha=1.0, encode="jpeg", quality=60)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["%05d.jpg" % k for k in range(3)]
    for k in range(3):
        assert (tmp_path / ("%05d.jpg" % k)).read_bytes() == J.encode(stubbed.synthetic_frame(10, 14, k), 60)


def test_no_network_keeps_the_host_path(stubbed, tmp_path):
    stubbed.main(["--no-network", "--synthetic", "2", "--height", "10", "--width", "14", "--output", str(tmp_path),
                  "--output-format", "jpeg", "--jpeg-quality", "85"])
    assert StubSegmenter.built == []
    assert sorted(p.name for p in tmp_path.iterdir()) == ["00000.jpg", "00001.jpg"]
    for k in range(2):
        frame = np.ascontiguousarray(stubbed.synthetic_frame(10, 14, k)[:, ::-1])   # the mirror
        mode, got = C.decode((tmp_path / ("%05d.jpg" % k)).read_bytes())
        assert mode == "RGB" and got.shape == frame.shape
        assert (tmp_path / ("%05d.jpg" % k)).read_bytes() == C.pil_encode(frame, 85, J.RI)
