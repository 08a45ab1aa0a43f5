"""The fitted-Huffman form of the PNG layout (util/png_layout.py, ``encode(img, huffman='fitted')``), without a GPU: the files
decode (PIL checks every CRC and the Adler-32, ``zlib`` the deflate stream), no segment grows, the code lengths are a complete
code of at most 15 bits, the depth limiter works, and the default output is the unchanged fixed form."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from util import args_helper, png_layout as P  # noqa: E402


def ellipse_map(h, w, noise, seed=0):
    """0 outside and 255 inside an ellipse; ``noise`` > 0 puts a noisy ramp on the edge."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = ((y - 0.5 * h) / (0.3 * h + 1)) ** 2 + ((x - 0.5 * w) / (0.25 * w + 1)) ** 2
    z = (1.0 - d) * 40.0 + (rng.normal(0.0, noise, (h, w)) if noise else 0.0)
    return (np.clip(255.0 / (1.0 + np.exp(-np.clip(z, -700, 700))), 0, 255) + 0.5).astype(np.uint8) if noise else \
        np.where(z >= 0, 255, 0).astype(np.uint8)


def no_equal_neighbours(counts):
    """A byte sequence in which value v occurs counts[v] times and no two neighbours are equal (the most frequent value
    first): the values by falling count into the even places, then into the odd ones."""
    order = sorted(range(len(counts)), key=lambda v: (-counts[v], v))
    flat = np.concatenate([np.full(counts[v], v, dtype=np.uint8) for v in order])
    out = np.empty(flat.size, dtype=np.uint8)
    n_even = (flat.size + 1) // 2
    out[0::2], out[1::2] = flat[:n_even], flat[n_even:]
    assert (out[1:] != out[:-1]).all()
    return out


def chain_counts(kind):
    """Sixteen literal counts which, with the end of block's 1, are 'fibonacci' 1,1,1,2,3,5,...,987 (sum 2584) or 'lucas'
    1,1,1,3,4,7,...,1364 (sum 3570).  Value 0 is the most frequent: a filtered stream starts with the filter byte 0."""
    seq = [1, 2] if kind == "fibonacci" else [1, 3]
    while len(seq) < 15:
        seq.append(seq[-1] + seq[-2])
    return sorted([1] + seq, reverse=True)


def chain_segment(kind, pad_to=None):
    seg = no_equal_neighbours(chain_counts(kind))
    assert seg[0] == 0
    if pad_to is not None:  # "padded to the cut": one run of a seventeenth value
        seg = np.concatenate([seg, np.full(pad_to - seg.size, 200, dtype=np.uint8)])
    return seg


def chain_image(kind, pad_to=None):
    """The [1, W] image whose filtered stream is ``chain_segment``."""
    return chain_segment(kind, pad_to)[1:].reshape(1, -1)


def long_runs_with_rests(h, w):
    """Long runs alternating with rests of 1 and 2 bytes."""
    flat = np.empty(h * w, dtype=np.uint8)
    at, k = 0, 0
    lengths = [700, 1, 300, 2, 1025, 1, 259, 2, 4100, 1, 260, 2]
    while at < flat.size:
        flat[at:at + lengths[k % len(lengths)]] = (37 * k + 5) % 251
        at, k = at + lengths[k % len(lengths)], k + 1
    return flat.reshape(h, w)


def cases():
    rng = np.random.default_rng(11)
    return {
        "1x1": np.array([[77]], dtype=np.uint8),
        "stream4095": rng.integers(0, 16, (1, 4094), dtype=np.uint8) * 17,
        "stream4096": ellipse_map(1, 4095, 2.0),
        "stream4097": rng.integers(0, 4, (1, 4096), dtype=np.uint8) * 85,
        "37x53_noisy_ellipse": ellipse_map(37, 53, 2.0),
        "96x160_noisy_ellipse": ellipse_map(96, 160, 2.0),
        "96x160_two_valued": ellipse_map(96, 160, 0),
        "96x160_constant": np.full((96, 160), 255, dtype=np.uint8),
        "96x160_noise16": rng.integers(0, 16, (96, 160), dtype=np.uint8) * 17,
        "96x160_noise256": rng.integers(0, 256, (96, 160), dtype=np.uint8),
        "96x160_runs_and_rests": long_runs_with_rests(96, 160),
        "fibonacci": chain_image("fibonacci"),
        "fibonacci_padded": chain_image("fibonacci", P.SEG_BYTES),
        "lucas": chain_image("lucas"),
        "lucas_padded": chain_image("lucas", P.SEG_BYTES),
    }


CASES = cases()


def idat_stream(file):
    return b"".join(data for tag, data in P.chunks(file) if tag == b"IDAT")


def kraft_numerator(lengths):
    return sum(1 << (P.MAX_CODE_BITS - int(v)) for v in lengths if v)


def todays_file(img):
    """The fixed-form file rebuilt from ``encode_segments`` with no help from ``encode``."""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    h, w = img.shape
    parts = [P.SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))]
    for s, (data, _stored) in enumerate(P.encode_segments(img)):
        parts.append(chunk(b"IDAT", (P.ZLIB_HEADER if s == 0 else b"") + data))
    adler = zlib.adler32(P.filtered_stream(img).tobytes()) & 0xffffffff
    return b"".join(parts + [chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", adler)), chunk(b"IEND", b"")])


@pytest.mark.parametrize("name", list(CASES))
def test_fitted_file_decodes_and_is_no_longer(name):
    img = CASES[name]
    fitted, fixed = P.encode(img, huffman="fitted"), P.encode(img, huffman="fixed")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(fitted))), img)
    assert zlib.decompress(idat_stream(fitted)) == P.filtered_stream(img).tobytes()
    tags_fitted, tags_fixed = P.chunks(fitted), P.chunks(fixed)
    assert tags_fitted[0] == tags_fixed[0] and tags_fitted[0][0] == b"IHDR"
    assert [t for t, _ in tags_fitted] == [t for t, _ in tags_fixed]
    # segment by segment: never longer, and shorter exactly where the fitted form was taken
    for (d1, form), (d0, stored) in zip(P.encode_segment_forms(img, "fitted"), P.encode_segments(img)):
        assert len(d1) <= len(d0) and (form == "fitted") == (len(d1) < len(d0))
        assert form == "fitted" or (d1 == d0 and form == ("stored" if stored else "fixed"))
    assert len(fitted) <= len(fixed) <= P.max_file_bytes(*img.shape)


@pytest.mark.parametrize("name", list(CASES))
def test_default_and_fixed_are_todays_bytes(name):
    img = CASES[name]
    assert P.encode(img) == P.encode(img, huffman="fixed") == todays_file(img)
    assert [f for _, f in P.encode_segment_forms(img)] == ["stored" if s else "fixed" for _, s in P.encode_segments(img)]


@pytest.mark.parametrize("name", list(CASES))
def test_lengths_are_a_complete_code_of_at_most_15_bits(name):
    stream = P.filtered_stream(CASES[name])
    for at in range(0, stream.size, P.SEG_BYTES):
        seg = stream[at:at + P.SEG_BYTES]
        counts, lengths = P.segment_histogram(seg), P.fitted_lengths(seg)
        assert lengths.shape == (P.N_LITLEN,) and ((lengths > 0) == (counts > 0)).all()
        assert lengths.max() <= P.MAX_CODE_BITS and kraft_numerator(lengths) == 1 << P.MAX_CODE_BITS
        # canonical: within a length the codes rise with the symbol, and they are prefix free (complete + distinct)
        codes = P.canonical_codes(lengths)
        used = np.flatnonzero(lengths)
        assert len({(int(lengths[s]), int(codes[s])) for s in used}) == used.size


def test_forms_chosen():
    rng = np.random.default_rng(5)
    noise16 = rng.integers(0, 16, P.SEG_BYTES, dtype=np.uint8) * 17
    data, form = P.segment_data_mode(noise16, "fitted")
    assert form == "fitted" and 8.0 * len(data) / noise16.size < 4.3   # 16 equally likely values: about 4 bits a byte
    noise256 = rng.integers(0, 256, P.SEG_BYTES, dtype=np.uint8)
    assert P.segment_data_mode(noise256, "fitted") == (P.segment_data(noise256)[0], "stored")
    constant = np.full(P.SEG_BYTES, 255, dtype=np.uint8)
    assert len(P.segment_data_mode(constant, "fitted")[0]) <= len(P.segment_data(constant)[0])
    for name in ("96x160_two_valued", "96x160_constant"):
        assert len(P.encode(CASES[name], huffman="fitted")) <= len(P.encode(CASES[name]))
    with pytest.raises(ValueError):
        P.encode(CASES["1x1"], huffman="dynamic")


def test_depth_limiter():
    """Under the stated tie rule (a leaf before a merged node of equal weight) the Fibonacci counts 1,1,1,2,3,...,987 do NOT
    reach 16: the two 2s and every later tie split the chain in two, the tree is 9 deep.  The chain needs every leaf to be
    strictly heavier than the node made two steps earlier: the counts 1,1,1,3,4,7,...,1364 (Lucas numbers, sum 3570 <= 4097)
    give 16, the limiter halves them once, and the segment still decodes."""
    fib = P.segment_histogram(chain_segment("fibonacci"))
    assert sorted(fib[fib > 0]) == [1, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]
    assert P.huffman_depths(fib).max() == 9
    lucas = P.segment_histogram(chain_segment("lucas"))
    assert lucas.sum() == 3570 and np.count_nonzero(lucas) == 17
    assert P.huffman_depths(lucas).max() == 16                       # the limiter is exercised ...
    lengths = P.huffman_lengths(lucas)
    assert lengths.max() <= P.MAX_CODE_BITS and kraft_numerator(lengths) == 1 << P.MAX_CODE_BITS
    assert np.array_equal(lengths, P.huffman_depths((lucas + 1) // 2))  # ... by one halving
    assert np.array_equal(lengths, P.fitted_lengths(chain_segment("lucas")))
    padded = P.segment_histogram(chain_segment("lucas", P.SEG_BYTES))
    print("lucas segment padded to the cut: depth", int(P.huffman_depths(padded).max()))
    for kind in ("fibonacci", "lucas"):
        for pad in (None, P.SEG_BYTES):
            seg = chain_segment(kind, pad)
            data = P.segment_data_fitted(seg)
            assert zlib.decompressobj(-15).decompress(data) == seg.tobytes()


def test_code_length_code_and_sequence():
    assert len(P.CL_LENGTHS) == 19 and sorted(P.CL_ORDER) == list(range(19))
    assert sum(1 << (5 - v) for v in P.CL_LENGTHS) == 1 << 5        # complete: zlib rejects anything else
    seq = P.code_length_sequence([3, 0, 0, 5] + [0] * 3 + [7] + [0] * 10 + [1] + [0] * 11 + [2] + [0] * 140 + [1])
    assert seq == [(3, 0, 0), (0, 0, 0), (0, 0, 0), (5, 0, 0), (17, 0, 3), (7, 0, 0), (17, 7, 3), (1, 0, 0), (18, 0, 7),
                   (2, 0, 0), (18, 127, 7), (0, 0, 0), (0, 0, 0), (1, 0, 0)]
    assert P.code_length_sequence([0] * 149 + [1]) == [(18, 127, 7), (18, 0, 7), (1, 0, 0)]


def test_png_fitted_flag_parsing():
    args = args_helper.parse_args(True, ["--synthetic", "--fast-test", "--png-fitted"])
    assert args.fast_test and args.png_fitted
    assert not args_helper.parse_args(True, ["--synthetic", "--fast-test"]).png_fitted
    with pytest.raises(SystemExit):
        args_helper.parse_args(True, ["--synthetic", "--png-fitted"])
    with pytest.raises(SystemExit):
        args_helper.parse_args(False, ["--synthetic", "--png-fitted"])   # an online flag


def test_fast_pass_host_path_writes_fitted_files(tmp_path):
    """CPU logits take ``png_layout.encode(..., huffman=png_huffman)``: the same pixels and scores, files no larger."""
    import torch
    from util import experiment_helper, io_helper

    class Net:
        def forward(self, x):
            x = x.cpu()  # test_fast moves the frame to the GPU where there is one; this net, and its logits, stay on the host
            g = torch.Generator().manual_seed(int(x.abs().sum() * 10) % 1000)
            base = (x[:, :1] - x[:, :1].flatten(1).median(dim=1).values.view(-1, 1, 1, 1)) * 4
            return [base + torch.randn(base.shape, generator=g)]

    class Provider:
        network = Net()

    out = {}
    for mode in ("fixed", "fitted"):
        loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=(24, 40), n_frames=3)
        score = experiment_helper.test_fast(Provider(), loader, tmp_path / mode, loader.dataset.annotation, seq_name="blob",
                                            png_huffman=mode)
        assert experiment_helper.last_fast["png_huffman"] == mode
        files = sorted((tmp_path / mode / "blob").iterdir())
        out[mode] = (score, [np.asarray(Image.open(str(f))) for f in files], experiment_helper.last_fast["png_bytes"])
    timed = ("seconds",)
    assert {k: v for k, v in out["fixed"][0].items() if k not in timed} == \
        {k: v for k, v in out["fitted"][0].items() if k not in timed}
    assert all(np.array_equal(a, b) for a, b in zip(out["fixed"][1], out["fitted"][1]))
    assert out["fitted"][2] <= out["fixed"][2]
    with pytest.raises(ValueError):
        experiment_helper.test_fast(Provider(), loader, tmp_path / "bad", png_huffman="best")
