"""The definition of the device JPEG decoder (util/jpeg_read.py) against PIL (libjpeg-turbo) byte for byte, what ``probe``
refuses, the status of damaged files, ``AviReader``, and the flag.  No GPU."""
import io
import os
import struct
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_cases as J  # noqa: E402
import jpeg_read_cases as C  # noqa: E402
from util import jpeg_read as R  # noqa: E402

CASES = C.cases()


def check_plan(plan, data):
    """The segment table covers every MCU exactly once, in order, and its bytes lie inside the scan."""
    mh, mw = R.n_mcus(plan.height, plan.width, plan.components, plan.subsampling)
    seg = plan.segments
    assert seg.dtype == np.int32 and seg.shape[1] == 4 and len(seg) == (-(-mh * mw // plan.restart_interval) if plan.restart_interval else 1)
    covered = np.zeros(mh * mw, dtype=np.int32)
    for off, length, first, count in seg.tolist():
        covered[first:first + count] += 1
        assert plan.scan[0] <= off and off + length <= plan.scan[1] and count > 0
    assert (covered == 1).all()
    assert data[plan.scan[1]:plan.scan[1] + 2] == b"\xff\xd9"
    total, grids = R.block_layout(plan)
    seen = np.zeros(total, dtype=np.int32)
    for m in range(mh * mw):
        for _, index in R.mcu_blocks(plan, m):
            seen[index] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("case", range(0, len(CASES), 16), ids=lambda k: CASES[k][0])
def test_decode_is_pils_byte_for_byte(case):
    for name, data in CASES[case:case + 16]:
        plan = R.probe(data)
        assert plan is not None, name
        check_plan(plan, data)
        want = C.pil_pixels(data)
        got, status = R.decode(data)
        assert status == 0 and got.dtype == np.uint8 and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int(np.abs(got.astype(int) - want).max()))
        assert (plan.height, plan.width) == want.shape[:2] and plan.components == (3 if want.ndim == 3 else 1)
        assert plan.subsampling == ("4:2:0" if "_420_" in name else "4:4:4") and plan.restart_interval == (16 if name.endswith("ri16") else 32 if name.endswith("ri32") else 0)


def test_the_cases_hold_what_they_are_meant_to():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names) and len(names) == 202
    plans = {n: R.probe(d) for n, d in CASES}
    assert max(len(p.segments) for p in plans.values()) >= 13                    # RST0..RST7 and round again
    assert any(p.dht[(1, 0)] != R.probe(CASES[0][1]).dht[(1, 0)] for p in plans.values())   # optimize=True: fitted tables
    assert not any("420" in n and "x4_" in n for n in names)


def test_davis_sized_frame():
    data = C.big_file()
    got, status = R.decode(data)
    assert status == 0 and got.shape == (480, 854, 3) and np.array_equal(got, C.pil_pixels(data))


# ------------------------------------------------------------------------------------------ what probe refuses
def replace_segment(data, marker, make, nth=0):
    """``data`` with the nth segment of ``marker`` replaced by ``make(payload)`` (None: dropped)."""
    out, seen = bytearray(data[:2]), 0
    for m, at, p, n in C.segments_of(data):
        seg = data[at:p + n]
        if m == marker:
            if seen == nth:
                payload = make(data[p:p + n])
                seg = b"" if payload is None else bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload
            seen += 1
        out += seg
    return bytes(out) + data[C.scan_start(data):]


def refusals():
    colour, grey = J.picture(33, 47), J.picture(33, 47, True)
    base, base420, basegrey = C.pil_file(colour, 90), C.pil_file(colour, 90, "420"), C.pil_file(grey, 90)
    restart = C.pil_file(J.picture(61, 107), 90, "444", 16)
    out = {}
    out["progressive"] = C.pil_file(colour, 90, progressive=True)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(colour[..., ::-1])).save(b, "JPEG", quality=90, subsampling=1)
    out["422"] = b.getvalue()
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(colour[..., ::-1])).convert("CMYK").save(b, "JPEG", quality=90)
    out["cmyk"] = b.getvalue()
    out["420_width_4"] = C.pil_file(J.picture(16, 4), 90, "420")
    out["12_bit"] = replace_segment(base, 0xC0, lambda p: b"\x0c" + p[1:])
    sof = [s for s in C.segments_of(base) if s[0] == 0xC0][0]
    out["sof1"] = base[:sof[1] + 1] + b"\xc1" + base[sof[1] + 2:]
    out["dqt_16_bit"] = replace_segment(base, 0xDB, lambda p: bytes([0x10 | p[0]]) + b"".join(b"\x00" + bytes([v]) for v in p[1:65]) + p[65:])
    out["adobe"] = base[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + base[2:]
    rgb = replace_segment(replace_segment(replace_segment(base, 0xE0, lambda p: None), 0xC0,
                                          lambda p: p[:6] + b"R" + p[7:9] + b"G" + p[10:12] + b"B" + p[13:]),
                          0xDA, lambda p: p[:1] + b"R" + p[2:3] + b"G" + p[4:5] + b"B" + p[6:])
    out["ids_rgb_without_jfif"] = rgb
    out["two_of_three_in_scan"] = replace_segment(base, 0xDA, lambda p: b"\x02" + p[1:5] + p[7:])
    out["spectral_selection"] = replace_segment(base, 0xDA, lambda p: p[:-3] + b"\x00\x05\x00")
    at = restart.index(b"\xff\xd1", C.scan_start(restart))
    out["rst_out_of_order"] = restart[:at + 1] + b"\xd2" + restart[at + 2:]
    out["rst_without_dri"] = replace_segment(restart, 0xDD, lambda p: None)
    out["rst_one_missing"] = restart[:at] + restart[at + 2:]
    out["dri_without_rst"] = replace_segment(base, 0xC0, lambda p: p) [:2] + b"\xff\xdd\x00\x04\x00\x02" + base[2:]
    out["dht_oversubscribed"] = replace_segment(basegrey, 0xC4, lambda p: p[:1] + b"\x03" + p[2:])
    out["dht_short_payload"] = replace_segment(basegrey, 0xC4, lambda p: p[:-1])
    out["dht_dc_symbol_16"] = replace_segment(basegrey, 0xC4, lambda p: p[:17] + b"\x10" + p[18:])
    out["dht_missing"] = replace_segment(basegrey, 0xC4, lambda p: None, nth=1)
    out["dqt_missing"] = replace_segment(basegrey, 0xDB, lambda p: None)
    out["length_past_the_end"] = base[:200]
    out["no_sos"] = base[:C.segments_of(base)[-1][1]] + b"\xff\xd9"
    out["no_eoi"] = base[:-2]
    out["no_soi"] = base[2:]
    out["ff_ff_in_scan"] = base420[:C.scan_start(base420) + 5] + b"\xff\xff" + base420[C.scan_start(base420) + 5:]
    out["other_marker_in_scan"] = base[:C.scan_start(base) + 5] + b"\xff\xc4" + base[C.scan_start(base) + 5:]
    out["zero_height"] = replace_segment(base, 0xC0, lambda p: p[:1] + b"\x00\x00" + p[3:])
    out["empty"] = b""
    out["png"] = b"\x89PNG\r\n\x1a\n" + bytes(64)
    return out


REFUSALS = refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_probe_refuses(name):
    data = REFUSALS[name]
    assert R.probe(data) is None
    assert R.decode(data) == (None, -1)


def test_probe_takes_the_files_the_refusals_were_made_of():
    for data in (C.pil_file(J.picture(33, 47), 90), C.pil_file(J.picture(33, 47, True), 90), C.pil_file(J.picture(16, 5), 90, "420"),
                 C.pil_file(J.picture(61, 107), 90, "444", 16)):
        assert R.probe(data) is not None
    # trailing bytes behind EOI and a fill byte in front of a marker are harmless, as they are to libjpeg
    data = C.pil_file(J.picture(33, 47), 90)
    assert R.probe(data + b"tail") is not None and np.array_equal(R.decode(data + b"tail")[0], C.pil_pixels(data))
    assert R.probe(data[:2] + b"\xff" + data[2:]) is not None


# ------------------------------------------------------------------------------------------ damaged files
@pytest.mark.parametrize("which", range(3), ids=[d[0] for d in C.damaged()])
def test_damaged_files_give_their_status(which):
    name, data, want = C.damaged()[which]
    plan = R.probe(data)
    assert plan is not None
    coef, status = R.coefficients(plan, data)
    assert status == want
    img, st = R.decode(data)
    assert st == want and img.shape[:2] == (plan.height, plan.width)
    if name == "run":
        assert not coef.any()                        # the failing block stays zero
    if name == "cut":
        total, _ = R.block_layout(plan)
        filled = coef.any(axis=1)
        assert filled.any() and not filled.all()     # blocks in front of the error are kept, those behind are zero


def test_status_5_for_a_product_beyond_16_bits():
    data = C.pil_file(J.checker(24, 40, True), 100)
    plan = R.probe(data)
    coef, status = R.coefficients(plan, data)
    assert status == 0 and R.reconstruct(plan, coef)[1] == 0
    big = plan._replace(quant=(plan.quant[0] * 255,))
    assert np.abs(coef.astype(np.int32) * big.quant[0]).max() > 32767
    assert R.reconstruct(big, coef)[1] == 5


# ------------------------------------------------------------------------------------------ AviReader, the flag
def test_avi_reader_returns_what_the_writer_was_given(tmp_path):
    from util.mjpeg_avi import AviReader, AviWriter
    files = [C.pil_file(J.picture(24, 40), q, "420", 16) for q in (1, 50, 90)] + [C.pil_file(J.noise(24, 40), 100)]
    files[0] += b"\x00" * (1 - (len(files[0]) & 1))          # an odd and an even length: the padding byte
    files[1] += b"\x00" * (len(files[1]) & 1)
    assert len(files[0]) & 1 == 1 and len(files[1]) & 1 == 0
    with AviWriter(tmp_path / "x.avi", 40, 24, fps=12.5) as w:
        for f in files:
            w.write(f)
    r = AviReader(tmp_path / "x.avi")
    assert list(r) == files and len(r) == 4 and (r.width, r.height) == (40, 24) and float(r.fps) == 12.5 and r[2] == files[2]
    whole = (tmp_path / "x.avi").read_bytes()
    for name, bad in (("short", whole[:100]), ("riff", b"RIFX" + whole[4:]), ("cut", whole[:len(whole) // 2]),
                      ("codec", whole.replace(b"vidsMJPG", b"vidsH264")), ("chunk", whole.replace(b"00dc", b"01wb", 1))):
        (tmp_path / (name + ".avi")).write_bytes(bad)
        with pytest.raises(ValueError):
            AviReader(tmp_path / (name + ".avi"))


def test_device_decode_flag_is_parsed_and_refuses_synthetic():
    from util import args_helper, io_helper
    assert args_helper.parse_args(True, ["--device-decode"]).device_decode is True
    assert args_helper.parse_args(True, []).device_decode is False
    with pytest.raises(SystemExit):
        args_helper.parse_args(True, ["--device-decode", "--synthetic"])
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--device-decode"])        # a flag of the online script
    with pytest.raises(ValueError):
        io_helper.get_data_loader_test("/nowhere", 1, "blob", synthetic=(48, 86), device_decode=True)
    import run_webcam
    assert run_webcam.build_parser().parse_args(["--device-decode", "--source", "x"]).device_decode is True
    with pytest.raises(ValueError):
        run_webcam.main(["--device-decode", "--synthetic", "2"])


def test_pack_tables_is_the_record_of_the_header():
    data = C.pil_file(J.picture(33, 47), 90, "420", 16)
    plan = R.probe(data)
    rec = R.pack_tables(plan, 7, len(plan.segments))
    assert len(rec) == R.TABLES_BYTES == 192 + 8 + 8 + 8 * 272
    assert np.array_equal(np.frombuffer(rec[:64], np.uint8), plan.quant[0]) and np.array_equal(np.frombuffer(rec[64:128], np.uint8), plan.quant[1])
    assert rec[192:198] == bytes([0, 1, 1, 4, 5, 5]) and struct.unpack("<ii", rec[200:208]) == (7, len(plan.segments))
    assert rec[208:208 + len(plan.dht[(0, 0)])] == plan.dht[(0, 0)] and rec[208 + 5 * 272:208 + 5 * 272 + 16] == plan.dht[(1, 1)][:16]
