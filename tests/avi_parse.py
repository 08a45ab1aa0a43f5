"""A small RIFF / AVI reader for the tests of util/mjpeg_avi.py: it checks every size on the way and returns what it found."""
import struct


def riff_tree(data, at, end):
    """[(fourcc, payload offset, size, children or None)] of the chunks in data[at:end]; a LIST's fourcc is its type."""
    out = []
    while at < end:
        assert at + 8 <= end, "a chunk header runs past its parent"
        tag, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        assert at + 8 + size <= end, (tag, size, "runs past its parent")
        if tag in (b"RIFF", b"LIST"):
            out.append((data[at + 8:at + 12], at + 12, size - 4, riff_tree(data, at + 12, at + 8 + size)))
        else:
            out.append((tag, at + 8, size, None))
        at += 8 + size + (size & 1)
    assert at in (end, end + 1), "the chunks do not fill their parent"
    return out


def parse_avi(data):
    """dict(width, height, frames=[bytes], micro_sec, scale, rate, ...) of an AVI 1.0 file with one MJPG stream; asserts that
    every size, count and index entry is consistent."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    (kind, _, _, top), = riff_tree(data, 0, len(data))
    assert kind == b"AVI " and [c[0] for c in top] == [b"hdrl", b"movi", b"idx1"]
    hdrl, movi, idx1 = top
    assert [c[0] for c in hdrl[3]] == [b"avih", b"strl"] and [c[0] for c in hdrl[3][1][3]] == [b"strh", b"strf"]
    avih, (strh, strf) = hdrl[3][0], hdrl[3][1][3]
    assert avih[2] == 56 and strh[2] == 56 and strf[2] == 40
    a = struct.unpack("<14I", data[avih[1]:avih[1] + 56])
    h = struct.unpack("<4s4sIHHIIIIIIiI4H", data[strh[1]:strh[1] + 56])
    f = struct.unpack("<IiiHH4sIiiII", data[strf[1]:strf[1] + 40])
    assert h[0] == b"vids" and h[1] == b"MJPG" and f[0] == 40 and f[3] == 1 and f[4] == 24 and f[5] == b"MJPG"
    frames = [data[at:at + size] for tag, at, size, _ in movi[3]]
    assert all(tag == b"00dc" for tag, _, _, _ in movi[3])
    assert a[3] & 0x10 and a[4] == h[9] == len(frames) and a[6] == 1           # has an index; frame counts; one stream
    assert a[8] == f[1] == h[15] and a[9] == f[2] == h[16] and f[6] == f[1] * f[2] * 3
    assert a[7] == h[10] == max([len(x) for x in frames] or [0])
    assert idx1[2] == 16 * len(frames)
    movi_tag = movi[1] - 4
    for k, (tag, at, size, _) in enumerate(movi[3]):
        ckid, flags, off, n = struct.unpack("<4sIII", data[idx1[1] + 16 * k:idx1[1] + 16 * k + 16])
        assert ckid == b"00dc" and flags == 0x10 and movi_tag + off == at - 8 and n == size
        assert data[movi_tag + off:movi_tag + off + 4] == b"00dc"
        assert at % 2 == 0                                                      # chunks start at even offsets
    return dict(width=a[8], height=a[9], frames=frames, micro_sec=a[0], scale=h[6], rate=h[7])
