"""The 4:2:0 and AVI options of run_webcam: the rejected combinations, what reaches the segmenter, and the host path's file.
The net and the segmenter are stubs.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from avi_parse import parse_avi  # noqa: E402
from util import jpeg_layout as J  # noqa: E402


class StubNet:
    def cuda(self):
        return self

    def eval(self):
        return self


class StubSegmenter:
    """Records how it was built; returns the layout's file of every frame as it came."""
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
            yield J.encode(f, self.kw["quality"], subsampling=self.kw.get("subsampling", "4:4:4"))


@pytest.fixture
def stubbed(monkeypatch):
    import run_webcam
    from fosvos_hip import stream
    StubSegmenter.built = []
    monkeypatch.setattr(run_webcam, "get_network", lambda *a, **k: StubNet())
    monkeypatch.setattr(stream, "FrameSegmenter", StubSegmenter)
    return run_webcam


SMALL = ["--variant", "vgg", "--synthetic", "3", "--height", "24", "--width", "40"]


def test_options_parse():
    import run_webcam
    p = run_webcam.build_parser()
    a = p.parse_args([])
    assert a.jpeg_subsampling == "444" and a.fps == 25
    a = p.parse_args(["--jpeg-subsampling", "420", "--fps", "29.97"])
    assert a.jpeg_subsampling == "420" and a.fps == 29.97
    for bad in (["--jpeg-subsampling", "422"], ["--jpeg-subsampling", "4:2:0"], ["--fps", "fast"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_rejected_combinations(stubbed, tmp_path):
    avi = str(tmp_path / "x.avi")
    with pytest.raises(ValueError, match="avi"):
        stubbed.main(SMALL + ["--output", avi])
    with pytest.raises(ValueError, match="avi"):
        stubbed.main(SMALL + ["--output", avi, "--output-format", "png", "--no-network"])
    with pytest.raises(ValueError, match="subsampling"):
        stubbed.main(SMALL + ["--jpeg-subsampling", "420"])
    with pytest.raises(ValueError, match="subsampling"):
        stubbed.main(SMALL + ["--jpeg-subsampling", "420", "--output", str(tmp_path / "d"), "--output-format", "png"])
    with pytest.raises(ValueError, match="fps"):
        stubbed.main(SMALL + ["--output", avi, "--output-format", "jpeg", "--fps", "0"])
    assert StubSegmenter.built == [] and list(tmp_path.iterdir()) == []


def test_device_path_writes_one_avi_from_the_returned_bytes(stubbed, tmp_path, monkeypatch):
    monkeypatch.setattr(stubbed, "write_jpeg_host", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the host encoder ran")))
    avi = tmp_path / "sub" / "x.AVI"
    rates = stubbed.main(SMALL + ["--output", str(avi), "--output-format", "jpeg", "--jpeg-subsampling", "420", "--jpeg-quality", "70",
                                  "--fps", "30"])
    assert len(rates) == 3
    (net, kw), = StubSegmenter.built
    assert kw == dict(depth=2, mirror=True, overlay=True, boolean_mask=True, color="r", alpha=1.0, encode="jpeg", quality=70,
                      subsampling="4:2:0")
    assert [p.name for p in (tmp_path / "sub").iterdir()] == ["x.AVI"]
    got = parse_avi(avi.read_bytes())
    assert (got["width"], got["height"], got["rate"], got["scale"]) == (40, 24, 30, 1)
    assert got["frames"] == [J.encode(stubbed.synthetic_frame(24, 40, k), 70, subsampling="4:2:0") for k in range(3)]
    # 4:4:4 into an AVI, and 4:2:0 into a directory
    stubbed.main(SMALL + ["--output", str(tmp_path / "y.avi"), "--output-format", "jpeg"])
    assert StubSegmenter.built[-1][1] == dict(depth=2, mirror=True, overlay=True, boolean_mask=True, color="r", alpha=1.0,
                                              encode="jpeg", quality=90)
    assert parse_avi((tmp_path / "y.avi").read_bytes())["frames"] == [J.encode(stubbed.synthetic_frame(24, 40, k), 90) for k in range(3)]
    stubbed.main(SMALL + ["--output", str(tmp_path / "d"), "--output-format", "jpeg", "--jpeg-subsampling", "420"])
    assert StubSegmenter.built[-1][1]["subsampling"] == "4:2:0"
    for k in range(3):
        assert (tmp_path / "d" / ("%05d.jpg" % k)).read_bytes() == J.encode(stubbed.synthetic_frame(24, 40, k), 90, subsampling="4:2:0")


@pytest.mark.parametrize("sub", ["444", "420"])
def test_no_network_host_path_writes_the_layouts_files(stubbed, tmp_path, sub):
    name = {"444": "4:4:4", "420": "4:2:0"}[sub]
    avi = tmp_path / "host.avi"
    stubbed.main(["--no-network", "--synthetic", "2", "--height", "24", "--width", "40", "--output", str(avi), "--output-format", "jpeg",
                  "--jpeg-quality", "85", "--jpeg-subsampling", sub])
    stubbed.main(["--no-network", "--synthetic", "2", "--height", "24", "--width", "40", "--output", str(tmp_path / "d"),
                  "--output-format", "jpeg", "--jpeg-quality", "85", "--jpeg-subsampling", sub])
    assert StubSegmenter.built == []
    want = [J.encode(np.ascontiguousarray(stubbed.synthetic_frame(24, 40, k)[:, ::-1]), 85, subsampling=name) for k in range(2)]
    got = parse_avi(avi.read_bytes())
    assert got["frames"] == want and (got["width"], got["height"], got["rate"], got["scale"]) == (40, 24, 25, 1)
    assert [(tmp_path / "d" / ("%05d.jpg" % k)).read_bytes() for k in range(2)] == want
