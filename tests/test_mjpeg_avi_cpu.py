"""util/mjpeg_avi.AviWriter: the file is read back with the tests' own RIFF reader (tests/avi_parse.py).  No GPU."""
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg420_cases as C4  # noqa: E402
from avi_parse import parse_avi  # noqa: E402
from util import jpeg_layout as J, mjpeg_avi as A  # noqa: E402


def three_files(h=24, w=40):
    """Three JPEG files of one size: lengths of both parities."""
    files = [J.encode(C4.noise(h, w), 90, subsampling="4:2:0"), J.encode(C4.ramp(h, w), 50, subsampling="4:2:0"),
             J.encode(C4.flat(h, w), 90, subsampling="4:2:0"), J.encode(C4.noise(h, w, seed=2), 90), J.encode(C4.ramp(h, w), 100)]
    odd, even = [f for f in files if len(f) & 1], [f for f in files if not len(f) & 1]
    assert odd and even, [len(f) for f in files]
    picked = [odd[0], even[0]] + (odd[1:] + even[1:])[:1]
    assert len({len(f) for f in picked}) == 3
    return picked


@pytest.mark.parametrize("fps", [25, 30, 29.97, 12.5])
def test_round_trip(tmp_path, fps):
    from PIL import Image
    files = three_files()
    path = tmp_path / "x.avi"
    with A.AviWriter(path, 40, 24, fps) as avi:
        for f in files:
            avi.write(f)
        assert avi.frames == 3
    data = path.read_bytes()
    got = parse_avi(data)
    assert got["frames"] == files and (got["width"], got["height"]) == (40, 24)
    assert abs(got["rate"] / got["scale"] - fps) < 1e-4 and got["micro_sec"] == round(1e6 / fps)
    assert len(data) == 12 + 8 + A._HDRL_BYTES + 12 + sum(8 + len(f) + (len(f) & 1) for f in files) + 8 + 16 * 3
    for f in got["frames"]:
        im = Image.open(io.BytesIO(f))
        im.load()
        assert im.size == (40, 24) and im.mode == "RGB"


def test_empty_file_and_edge_cases(tmp_path, monkeypatch):
    path = tmp_path / "empty.avi"
    avi = A.AviWriter(path, 8, 8, 25)
    avi.close()
    avi.close()                                              # twice is harmless
    assert parse_avi(path.read_bytes())["frames"] == []
    size = path.stat().st_size
    with pytest.raises(ValueError, match="closed"):
        avi.write(three_files()[0])
    assert path.stat().st_size == size
    for bad in (dict(width=0, height=8), dict(width=8, height=70000), dict(width=8, height=8, fps=0), dict(width=8, height=8, fps=-1)):
        with pytest.raises(ValueError):
            A.AviWriter(tmp_path / "bad.avi", **bad)
    with A.AviWriter(tmp_path / "y.avi", 40, 24, 25) as avi:
        with pytest.raises(ValueError, match="JPEG"):
            avi.write(b"not a picture")
        assert avi.frames == 0


def test_size_limit_raises_before_the_write(tmp_path, monkeypatch):
    files = three_files()
    assert A.MAX_BYTES == 2 ** 31 - 1
    head = 12 + 8 + A._HDRL_BYTES + 12
    room = head + sum(8 + len(f) + (len(f) & 1) for f in files[:2]) + 8 + 16 * 2     # exactly two frames and their index
    monkeypatch.setattr(A, "MAX_BYTES", room)
    path = tmp_path / "full.avi"
    with A.AviWriter(path, 40, 24, 25) as avi:
        avi.write(files[0])
        avi.write(files[1])
        with pytest.raises(A.AviSizeError, match="past"):
            avi.write(files[2])
        assert avi.frames == 2
    data = path.read_bytes()
    assert len(data) == room and parse_avi(data)["frames"] == files[:2]          # the refused frame left no trace
    monkeypatch.setattr(A, "MAX_BYTES", room - 1)
    with A.AviWriter(tmp_path / "short.avi", 40, 24, 25) as avi:
        avi.write(files[0])
        with pytest.raises(A.AviSizeError):
            avi.write(files[1])
