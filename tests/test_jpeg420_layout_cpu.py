"""The 4:2:0 form of the JPEG layout (util/jpeg_layout.py, ``subsampling='4:2:0'``) against PIL's encoder (libjpeg-turbo),
byte for byte, and the guards that the 4:4:4 form did not move.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg420_cases as C4  # noqa: E402
import jpeg_cases as C  # noqa: E402
from util import jpeg_layout as J  # noqa: E402

S = "4:2:0"


@pytest.mark.parametrize("size", C4.SIZES, ids=lambda s: "%dx%d" % s)
def test_layout_is_pils_file_byte_for_byte(size):
    h, w = size
    for content in C4.CONTENTS:
        img = C4.make(content, h, w)
        for q in C4.QUALITIES:
            ours, theirs = J.encode(img, q, subsampling=S), C4.pil_encode_420(img, q)
            assert ours == theirs, (content, size, q, len(ours), len(theirs))
            assert len(ours) <= J.capacity(h, w, 3, S)
            assert J.header(h, w, 3, q, S) == ours[:J.header_bytes(3, S)]
    mode, got = C.decode(J.encode(C4.make("ramp", h, w), 90, subsampling=S))
    assert mode == "RGB" and got.shape == (h, w, 3)


def test_batch_and_workload_frames_are_pils_files():
    for frame in C4.batch():
        for q in C4.QUALITIES:
            assert J.encode(frame, q, subsampling=S) == C4.pil_encode_420(frame, q)
            assert len(J.encode(frame, q, subsampling=S)) <= J.capacity(*C4.BATCH[1:], 3, S)
    frame = C4.workload_frame()
    data = J.encode(frame, 90, subsampling=S)
    assert data == C4.pil_encode_420(frame, 90)
    h, w = C4.WORKLOAD
    assert J.n_mcus(h, w, S) == 1620 and J.n_intervals(h, w, S) == 102 and len(data) <= J.capacity(h, w, 3, S)
    assert J.dummy_blocks(h, w).any() and len(data) < len(J.encode(frame, 90))


def test_inputs_hold_a_stuffed_byte_and_a_dummy_block_with_a_dc():
    """Without these the cases would not test the byte stuffing or the dummy-block rule."""
    stuffed = [name for name, img, q in C4.small_inputs() if b"\xff\x00" in J.scan_bytes(J.encode(img, q, subsampling=S))]
    assert any(name.startswith("noise") and name.endswith("q100") for name in stuffed), stuffed
    copied = []
    for name, img, q in C4.small_inputs():
        coef, dummy = J.coefficients(img, q, S), J.dummy_blocks(*img.shape[:2])
        assert coef.shape == (J.n_mcus(*img.shape[:2], S), 6, 64) and not dummy[:, 0].any() and not dummy[:, 4:].any()
        assert (coef[dummy][:, 1:] == 0).all()
        for k in range(1, 4):
            assert (coef[dummy[:, k], k, 0] == coef[dummy[:, k], k - 1, 0]).all()
        if dummy.any() and (coef[dummy][:, 0] != 0).any():
            copied.append(name)
    assert any("8x8" in n for n in copied) and any("24x40" in n for n in copied) and any("32x136" in n for n in copied), copied
    # the dummy blocks' DC differences are 0 and they end at once: two symbols, ('dc', 0) and EOB
    sym = [s for s in J.symbols(C4.flat(8, 8), 90, S) if s.component == 0]
    assert [(s.kind, s.rs) for s in sym[2:]] == [("dc", 0), ("ac", J.EOB)] * 3 and sym[0].rs != 0
    # two intervals at 16x272: the second starts with a DC that is no difference
    assert {s.interval for s in J.symbols(C4.flat(16, 272), 90, S)} == {0, 1}
    assert J.scan_bytes(J.encode(C4.flat(16, 272), 90, subsampling=S)).count(b"\xff\xd0") == 1


def test_structure_of_the_420_header():
    data = J.encode(C4.ramp(24, 40), 90, subsampling=S)
    seg = dict((m, p) for m, p in J.segments(data) if m in (0xC0, 0xDD))
    assert seg[0xC0][5:] == bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]) and seg[0xDD] == bytes([0, J.RI_420])
    assert J.RI_420 == 16 and J.RI_420 * 6 == J.RI * 3
    assert J.n_mcus(24, 40, S) == 2 * 3 and J.n_mcus(24, 40) == 3 * 5 and J.n_intervals(16, 272, S) == 2
    assert J.capacity(24, 40, 3, S) == J.header_bytes(3) + 416 * 6 * 6 + 2 * 1
    assert J.capacity(480, 854, 3, S) == 629 + 416 * 6 * 1620 + 2 * 102


def test_default_is_444_and_grey_ignores_the_argument():
    for name, img, q in C.all_inputs()[::7]:
        assert J.encode(img, q) == J.encode(img, q, subsampling="4:4:4") == C.pil_encode(img, q, J.RI), name
    for h, w in C4.SIZES:
        grey = C.picture(h, w, grey=True)
        for q in (50, 100):
            assert J.encode(grey, q, subsampling=S) == J.encode(grey, q, subsampling="4:4:4") == J.encode(grey, q)
        assert J.capacity(h, w, 1, S) == J.capacity(h, w, 1) and J.header(h, w, 1, 90, S) == J.header(h, w, 1, 90)
        assert J.capacity(h, w, 3) == J.capacity(h, w, 3, "4:4:4") and J.header(h, w, 3, 90) == J.header(h, w, 3, 90, "4:4:4")
        assert (J.coefficients(grey, 90, S) == J.coefficients(grey, 90)).all()
        assert J.symbols(grey, 90, S) == J.symbols(grey, 90)


def test_unknown_subsampling_raises():
    img = C4.ramp(16, 16)
    for bad in ("4:2:2", "420", 2, None, ""):
        for call in (lambda: J.encode(img, 90, subsampling=bad), lambda: J.capacity(16, 16, 3, bad), lambda: J.n_mcus(16, 16, bad),
                     lambda: J.n_intervals(16, 16, bad), lambda: J.header(16, 16, 3, 90, bad), lambda: J.header_bytes(3, bad),
                     lambda: J.blocks(img, bad), lambda: J.coefficients(img, 90, bad), lambda: J.symbols(img, 90, bad),
                     lambda: J.encode(img[..., 0], 90, subsampling=bad)):
            with pytest.raises(ValueError):
                call()
