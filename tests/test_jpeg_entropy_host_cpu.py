"""The entropy decoder of the device JPEG decoder (csrc/jpeg_entropy.h, the text the kernel runs with one wave a segment) as
a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/jpeg_entropy_main.cpp, built
here with the C++ compiler that is found, run as a child process over every good and every damaged case file.  Nothing is
loaded into this process, and the child inherits the environment as it is.  No GPU."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_read_cases as C  # noqa: E402
from util import jpeg_read as R  # noqa: E402

CXX = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)


def write_input(path, plan, data):
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", plan.height, plan.width, plan.components, int(plan.subsampling == "4:2:0"), len(data),
                            len(plan.segments)))
        f.write(R.pack_tables(plan, 0, len(plan.segments)))
        f.write(data)
        f.write(plan.segments.astype("<i4").tobytes())


@pytest.mark.skipif(CXX is None, reason="no C++ compiler")
def test_host_form_under_the_sanitizers(tmp_path):
    exe = tmp_path / "jpeg_entropy_main"
    # the sanitizer runtimes are linked into the program, so it needs no particular library order when it starts
    static = ["-static-libsan"] if "clang" in CXX else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                           ["-o", str(exe), os.path.join(ROOT, "tests", "host", "jpeg_entropy_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    files = list(C.cases()) + [(name, data) for name, data, _ in C.damaged()]
    # rows that point outside the bytes or the grid, and tables of zeros: refused or decoded to a status, never read past
    hostile = []
    name, data = C.cases()[-1]
    plan = R.probe(data)
    for tag, seg in (("offset", [[len(data) - 4, 64, 0, 1]]), ("mcus", [[int(plan.segments[0][0]), 64, 0, 1 << 20]]),
                     ("negative", [[-5, 10, 0, 1]])):
        hostile.append(("hostile_" + tag, data, plan._replace(segments=np.asarray(seg, dtype=np.int32))))
    hostile.append(("hostile_tables", data, plan._replace(dht={})))
    args = []
    for name, data in files:
        write_input(tmp_path / (name + ".in"), R.probe(data), data)
        args += [str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))]
    for name, data, p in hostile:
        write_input(tmp_path / (name + ".in"), p, data)
        args += [str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    for name, data in files:
        plan = R.probe(data)
        want, status = R.coefficients(plan, data)
        raw = (tmp_path / (name + ".out")).read_bytes()
        assert struct.unpack("<i", raw[:4])[0] == status, name
        assert np.array_equal(np.frombuffer(raw[4:], dtype="<i2").reshape(-1, 64), want), name
    statuses = {name: struct.unpack("<i", (tmp_path / (name + ".out")).read_bytes()[:4])[0] for name, _, _ in hostile}
    assert statuses == {"hostile_offset": 1, "hostile_mcus": 1, "hostile_negative": 1, "hostile_tables": 2}
    assert [struct.unpack("<i", (tmp_path / (n + ".out")).read_bytes()[:4])[0] for n, _, _ in C.damaged()] == [1, 2, 3]
