"""The island cases of the byte-oriented kernels, alone (no GPU): tests/io_island_cases.py's references run and give the
declared shapes, every case has the structural property it is listed for (computed from the reference or from the restated
size formulas, not assumed), every operand sits where its entry's alignment rule allows, and for every entry the detector of
tests/islands.py notices a planted fault in a fake op - the reference run on the island's own tensors plus one store one
element behind an output, or one read in front of an input that enters the output the way the operation uses that input."""
import zlib

import numpy as np
import pytest
import torch

import io_island_cases as C
import islands as I

entries = pytest.mark.parametrize("entry", C.ENTRIES)


def _forms(entry, **where):
    return [f for f in C.forms(entry) if all(f.args.get(k, f.props.get(k)) == v for k, v in where.items())]


# ------------------------------------------------------------------------------------------ every case, every entry
@entries
def test_the_reference_runs_and_gives_the_declared_outputs(entry):
    assert C.forms(entry)
    for f in C.forms(entry):
        want = f.expected()
        declared = {o.name: o for o in f.ops if o.kind in ("out", "inout")}
        assert set(want) == set(declared), (f.tag, sorted(want), sorted(declared))
        for name, o in declared.items():
            assert want[name].shape == o.shape and want[name].dtype == o.dtype, (f.tag, name, want[name].shape, want[name].dtype)
        assert f.expected() is want  # computed once, shared, read-only
        assert not any(a.flags.writeable for a in want.values())


@entries
def test_every_operand_sits_at_an_alignment_its_entry_accepts(entry):
    rule = C.ALIGN[entry]
    off16 = aligned = 0
    for f in C.forms(entry):
        assert {o.name for o in f.ops} <= set(rule), f.tag
        for o in f.ops:
            assert o.offset % rule[o.name] == 0 and 0 <= o.offset < 256, (f.tag, o.name, o.offset)
            assert o.offset % o.dtype.itemsize == 0
            # flat islands: 64 KiB hold the margin rule of a map, 17 of the operand's rows and a pixel (tests/islands.py)
            interleaved = len(o.shape) >= 3 and o.shape[-1] == 3  # [.., H, W, 3]: a row is W pixels of three bytes
            row = o.dtype.itemsize * (3 * o.shape[-2] if interleaved else o.shape[-1])
            assert len(o.shape) == 1 or 17 * row + 16 <= I.FLAT_MARGIN, (f.tag, o.name, row)  # (file slots, workspaces: no rows)
        if f.tag.endswith("least"):
            # the least alignment: a checked alignment exactly, an unchecked operand at its type's (a byte at an odd address)
            for o in f.ops:
                if rule[o.name] > 1:
                    assert o.offset == rule[o.name], (f.tag, o.name)
                else:
                    assert o.offset % 2 == 1 or o.offset == 12, (f.tag, o.name)  # (12: the augmentation's mask, as the issue sets it)
            off16 += any(o.offset % 16 for o in f.ops)
        else:
            assert all(o.offset == 0 for o in f.ops), f.tag
            aligned += 1
    assert off16 >= 1 and aligned >= 1, entry


def test_forms_with_frames_hold_a_frame_boundary():
    for entry in C.ENTRIES:
        if entry == "augment_sample":  # one sample a call
            continue
        assert any(f.args["N"] >= 2 for f in C.forms(entry)), entry
        for f in C.forms(entry):
            if f.args["N"] == 1:  # only the shapes the issue lists with one frame
                assert (f.args.get("H", f.args.get("Hf")), f.args.get("W", f.args.get("Wf"))) in ((9, 461), (33, 130), (17, 530))


# ------------------------------------------------------------------------------------------ the properties of the shapes
def test_paint_shapes_split_vectors_and_cross_a_workgroup():
    (n0, h0, w0), (n1, h1, w1) = C.PAINT_SHAPES
    assert (3 * w0) % C.STREAM_GROUP_PX and (h0 * w0) % C.STREAM_GROUP_PX and (3 * h0 * w0) % 16 and n0 == 2
    per_group = C.STREAM_GROUP_PX * C.STREAM_THREADS
    assert per_group == 4096 and per_group < n1 * h1 * w1 <= 2 * per_group and (h1 * w1) % C.STREAM_GROUP_PX
    for entry in ("overlay", "overlay_scaled"):
        seen = set()
        for f in C.forms(entry):
            assert f.props["band"] == 0, (f.tag, f.props)  # exact expected bits in the soft modes
            assert f.has("frames") == (f.args["mode"] < 2)  # the mask modes carry no frames operand
            seen.add((f.args["mode"], f.args["mirror"]))
        assert seen == {(m, k) for m in range(4) for k in (0, 1)}
        out = np.concatenate([f.expected()["out"].reshape(-1) for f in C.forms(entry) if f.args["mode"] == 1])
        assert len(np.unique(out)) > 100  # the soft overlay is no constant


def test_scaled_shapes_are_ragged_and_longer_than_a_chunk():
    (n, hf, wf, hn, wn), (_, hf2, wf2, hn2, wn2), (_, hf3, wf3, hn3, wn3) = C.SCALED_SHAPES
    assert wn == C.SCALE_COLS + 3 and hn % C.SCALE_ROWS and hf % hn and wf % wn and n == 2
    assert wf2 > C.SCALE_CHUNK_PX and wn2 > C.SCALE_COLS and hn2 % C.SCALE_ROWS and wf2 % wn2
    assert (hf3, wf3) == (hn3, wn3)
    for entry in ("frame_prep_scaled", "overlay_scaled"):
        assert {(f.args["Hf"], f.args["Wf"], f.args["Hn"], f.args["Wn"]) for f in C.forms(entry)} == {s[1:] for s in C.SCALED_SHAPES}


def test_prob_bytes_paths():
    scalar, vector, wide = C.forms("prob_bytes")
    for f in (scalar, vector, wide):
        assert f.props["band"] == 0
    hw = lambda f: f.args["H"] * f.args["W"]  # noqa: E731
    assert hw(scalar) % 4 and scalar.op("logits").offset == 4
    assert hw(vector) % 4 == 0 and vector.op("logits").offset == 0 and vector.op("out").offset == 0
    assert hw(wide) > C.EVAL_THREADS and hw(wide) % 4  # the scalar path: a pixel a thread, more than one workgroup
    k = scalar.props["constant_frame"]
    x = scalar.op("logits").data
    assert x[k].min() == x[k].max() and (scalar.expected()["out"][k] == 0).all()
    assert np.array_equal(scalar.expected()["minmax"][k], np.array([x[k].min()] * 2, np.float32))
    for f in (vector, wide):
        out = f.expected()["out"]
        assert out.min() == 0 and out.max() == 255


def test_jf_shapes_split_words_rows_and_tiles():
    (n0, h0, w0), (n1, h1, w1) = C.JF_SHAPES
    words0, words1 = -(-w0 // C.JF_WORD), -(-w1 // C.JF_WORD)
    assert words0 == 2 and w0 % C.JF_WORD == 6 and h0 > C.JF_TILE_ROWS and n0 == 2
    assert (h0 * words0 * 8) % 64  # frame 1's bit planes begin mid-line
    assert words1 == 9 and words1 > C.JF_TILE_WORDS and h1 > C.JF_TILE_ROWS
    assert max(C.JF_RADII) == 63 and 63 > max(h0, h1) and min(C.JF_RADII) == 1
    for entry in ("jf_counts", "jf_counts_labels"):
        assert {f.args["radius"] for f in C.forms(entry)} == set(C.JF_RADII)
        for f in C.forms(entry):
            counts = f.expected()["counts"].reshape(-1, 6)
            assert (counts.max(axis=0) > 0).all(), (f.tag, counts.tolist())  # every counter counts something
            k = f.args.get("K", 1)
            assert f.op("workspace").shape[0] == 2 * f.args["N"] * k * f.args["H"] * (-(-f.args["W"] // 64)) * 8
    for f in C.forms("jf_counts_labels"):
        assert f.op("pred").data.max() == C.JF_K + 1  # a label that belongs to no object


def test_merge_cases_hold_ties_and_an_empty_pixel():
    assert {(f.args["K"], f.tag.endswith("least")) for f in C.forms("merge_objects")} == {(1, True), (3, True), (1, False), (3, False)}
    for f in C.forms("merge_objects"):
        k, hw = f.args["K"], f.args["H"] * f.args["W"]
        maps = np.stack([f.op("map%d" % i).data[:, 0] for i in range(k)])
        labels = f.expected()["labels"]
        assert (labels[:, 0, 1] == 0).all() and (maps[:, :, 0, 1] < 0).all()
        assert set(np.unique(labels)) == set(range(k + 1))
        if f.tag.endswith("least"):
            assert hw % 4 and f.op("map0").offset == 4 and f.op("labels").offset == 3  # the 1-pixel path
        else:
            assert hw % 4 == 0  # the 4-pixel path
        if k > 1:
            tie = (maps[0] == maps[1]) & (maps[0] >= 0) & (maps[0] >= maps[2])
            assert tie.sum() > 5 and (labels[tie] == 1).all()  # the lowest id wins
            tie = (maps[1] == maps[2]) & (maps[1] >= 0) & (maps[1] > maps[0])
            assert tie.sum() > 2 and (labels[tie] == 2).all()


@pytest.mark.parametrize("entry", ["png_encode", "png_encode_indexed"])
def test_png_cases(entry):
    indexed = entry == "png_encode_indexed"
    streams = [h * (w + 1) for _, h, w in C.PNG_SHAPES]
    assert streams[0] < C.PNG_SEG and streams[1] == C.PNG_SEG and streams[2] == C.PNG_SEG + 64
    assert [C.png_layout.n_segments(h, w) for _, h, w in C.PNG_SHAPES] == [1, 1, 2]
    fitted_somewhere = fixed_somewhere = False
    seen = set()
    for f in C.forms(entry):
        n, h, w, cap = f.args["N"], f.args["H"], f.args["W"], f.args["capacity"]
        assert cap == 65 + h * (w + 1) + 17 * C.png_layout.n_segments(h, w) + (780 if indexed else 0)
        files = C.png_files(f, f.inputs())
        want = f.expected()
        assert want["lengths"].tolist() == [len(d) for d in files] and max(len(d) for d in files) <= cap and n == 2
        for k, d in enumerate(files):  # the file, then the pre-fill as it was
            at = k * cap
            assert bytes(want["out"][at:at + len(d)]) == d
            assert np.array_equal(want["out"][at + len(d):at + cap], f.op("out").data[at + len(d):at + cap])
            assert [t for t, _ in C.png_layout.chunks(d)].count(b"IDAT") == C.png_layout.n_segments(h, w) + 1
        if f.tag.endswith("least"):
            start = f.op("out").offset
            assert start % 4 and (start + cap) % 4, f.tag  # neither file begins on a dword boundary
        mode = C.png_layout.HUFFMAN_MODES[f.args["huffman"]]
        kinds = [form for img in f.op("bytes").data for _, form in C.png_layout.encode_segment_forms(img, mode)]
        if f.props["content"] == "noise":
            assert set(kinds) == {"stored"} and max(len(d) for d in files) == cap  # the longest file there is
        if f.props["content"] == "constant":
            # frame 0 is one long run a segment: a literal and ceil(4095 / 258) = 16 matches of at most 18 bits, 40 bytes
            # with the block's frame, beside the 17 bytes of the chunk and the stored header the bound counts
            assert "stored" not in kinds and not f.op("bytes").data[0].any()
            assert len(files[0]) <= 65 + 57 * C.png_layout.n_segments(h, w) + (780 if indexed else 0)
        fixed_somewhere |= f.props["content"] == "blobs" and "fixed" in kinds
        fitted_somewhere |= f.props["content"] == "blobs" and "fitted" in kinds
        seen.add((h, w, f.props["content"], f.args["huffman"], f.props["prefill"]))
    assert fitted_somewhere and fixed_somewhere
    assert len(seen) == 3 * 3 * 2 * 2
    # the two pre-fills of a case differ, the files in them do not
    for f in _forms(entry, prefill=0):
        if not f.tag.endswith("least"):
            continue
        g = next(x for x in _forms(entry, prefill=1) if x.tag == f.tag.replace("prefill0", "prefill1"))
        assert not np.array_equal(f.op("out").data, g.op("out").data)
        assert C.png_files(f, f.inputs()) == C.png_files(g, g.inputs())


def test_jpeg_cases():
    J = C.jpeg_layout
    forms = C.forms("jpeg_encode")
    stuffed = 0
    for f in forms:
        a = f.args
        comps, sampling, shapes = C.JPEG_KINDS[f.props["kind"]]
        name = "4:2:0" if sampling == 420 else "4:4:4"
        files = C.jpeg_files(f, f.inputs())
        want = f.expected()
        stride = a["out_stride"]
        side = 16 if sampling == 420 else 8
        mcus = (-(-a["H"] // side)) * (-(-a["W"] // side))
        blocks = mcus * (6 if sampling == 420 else comps)
        ri = C.JPEG_RI_420 if sampling == 420 else C.JPEG_RI
        intervals = -(-mcus // ri)
        assert stride == J.header_bytes(comps) + 416 * blocks + 2 * intervals
        assert f.op("workspace").shape[0] == 4 * a["N"] * intervals and a["N"] == 2
        assert want["lengths"].tolist() == [len(d) for d in files] and max(len(d) for d in files) <= stride
        for k, d in enumerate(files):
            at = k * stride
            assert bytes(want["out"][at:at + len(d)]) == d and d[:2] == b"\xff\xd8" and d[-2:] == b"\xff\xd9"
            assert np.array_equal(want["out"][at + len(d):at + stride], f.op("out").data[at + len(d):at + stride])
            scan = J.scan_bytes(d)
            rst = sum(scan.count(bytes([0xFF, 0xD0 + i])) for i in range(8))
            assert rst == intervals - 1, (f.tag, rst)
            if a["quality"] == 100 and f.props["content"] == "noise":
                assert scan.count(b"\xff\x00") >= 1, f.tag
                stuffed += 1
        first = (a["H"], a["W"]) == shapes[0][1:]
        if first:
            assert intervals == 1 and a["H"] % side and a["W"] % side  # replication on both sides
            if sampling == 420:
                assert J.dummy_blocks(a["H"], a["W"]).any() and (-(-a["H"] // 2)) % 8  # dummy luma blocks, a replicated chroma row
        else:
            assert mcus == ri + 1 and intervals == 2
        if f.tag.endswith("least"):
            assert f.op("frames").offset == 1 and f.op("out").offset == 1
    assert stuffed >= 6
    least = [f for f in forms if f.tag.endswith("least")]
    assert {(f.props["kind"], f.args["H"], f.args["W"], f.args["quality"], f.props["content"], f.props["prefill"]) for f in least} == \
        {(kind, s[1], s[2], q, c, p) for kind, (_, _, shapes) in C.JPEG_KINDS.items() for s in shapes for q in C.JPEG_QUALITIES
         for c in C.JPEG_CONTENTS for p in C.PREFILLS}
    for f in _forms("jpeg_encode", prefill=0):
        if f.tag.endswith("least"):
            g = next(x for x in forms if x.tag == f.tag.replace("prefill0", "prefill1"))
            assert not np.array_equal(f.op("out").data, g.op("out").data) and C.jpeg_files(f, f.inputs()) == C.jpeg_files(g, g.inputs())


def test_augment_cases():
    forms = C.forms("augment_sample")
    assert {((f.args["H"], f.args["W"]), (f.args["OH"], f.args["OW"]), f.args["flip"]) for f in forms if f.tag.endswith("least")} == \
        {(s[0], s[2], flip) for s in C.AUGMENT_SIZES for flip in (0, 1)}
    (a, _, a_out), (b, _, b_out), (c, _, c_out) = C.AUGMENT_SIZES
    assert a_out[0] < a[0] and a_out[1] < a[1] and b_out[0] > b[0] and b_out[1] > b[1] and c_out == c
    for f in forms:
        assert f.props["copy"] == ((f.args["H"], f.args["W"]) == (f.args["OH"], f.args["OW"]))
        assert f.has("col_taps") == (not f.props["copy"])
        assert (3 * f.args["W"]) % 16  # no frame row begins where the one before it did
        if f.tag.endswith("least"):
            assert f.op("frame").offset == 7 and f.op("mask").offset == 12
            if f.has("col_taps"):
                assert f.op("col_taps").offset == 16 and f.op("col_w").offset == 16
        assert len(np.unique(f.expected()["gt"])) == 3
    flipped = {f.args["flip"]: f for f in forms if f.tag.startswith("13x17 -> 10x13") and f.tag.endswith("least")}
    assert not np.array_equal(flipped[0].expected()["image"], flipped[1].expected()["image"])


def test_gate_cases():
    for n, h, w in C.GATE_SHAPES:
        assert h > C.GATE_BATCH and h % C.GATE_BATCH and w > C.GATE_COL_THREADS and w % C.GATE_COL_THREADS
        assert max(C.GATE_DISTANCES) > max(h, w)
    assert C.GATE_SHAPES[1][1] > 2 * C.GATE_BATCH and set(C.GATE_DISTANCES) >= {0, 1, 5} and set(C.ERODES) == {0, 2}
    a, b = C.gate_masks(2, 19, 70, "a"), C.gate_masks(2, 19, 70, "b")
    assert not a[1].any() and b[0].all() and a[0].any() and not a[0].all() and b[1].sum() == 1
    seen = set()
    for f in C.forms("distance_gate"):
        n, h, w = f.args["N"], f.args["H"], f.args["W"]
        assert f.op("workspace").shape[0] == (4 * n + 15) // 16 * 16 + (2 * n * h * w + 15) // 16 * 16
        seen.add((n, h, w, f.args["distance"], f.args["invert"], f.props["masks"]))
    assert seen >= {(n, h, w, d, inv, m) for n, h, w in C.GATE_SHAPES for d in C.GATE_DISTANCES for inv in (0, 1)
                    for m in (("a", "b") if n == 2 else ("a",))}
    out = np.concatenate([f.expected()["out"].reshape(-1) for f in C.forms("distance_gate")])
    assert 0.2 < out.mean() < 0.8
    classes = np.zeros(3, np.int64)
    seen = set()
    for f in C.forms("adapt_labels"):
        n, h, w = f.args["N"], f.args["H"], f.args["W"]
        assert f.op("workspace").shape[0] == (4 * n + 15) // 16 * 16 + (2 * n * h * w + 15) // 16 * 16 + n * h * w
        want = f.expected()
        assert (want["counts"].sum(axis=1) == h * w).all()
        classes += want["counts"].sum(axis=0)
        seen.add((n, h, w, f.args["neg_distance"], f.args["erode"], f.props["masks"]))
    assert seen >= {(n, h, w, d, e, m) for n, h, w in C.GATE_SHAPES for d in C.GATE_DISTANCES for e in C.ERODES
                    for m in (("a", "b") if n == 2 else ("a",))}
    assert (classes > 1000).all(), classes


# ------------------------------------------------------------------------------------------ the detector on a known fault
_MEMO = {}


def _reference_on(form, isl):
    """The reference of ``form`` run on the island's own tensors (equal inputs are computed once)."""
    inputs = {o.name: isl.view(o.name).numpy().copy() for o in form.ops if o.kind in ("in", "inout")}
    key = (form.entry, form.tag) + tuple(zlib.crc32(v.tobytes()) for v in inputs.values())
    if key not in _MEMO:
        _MEMO[key] = C.reference(form, inputs)
    return _MEMO[key]


def _element(isl, o, at):
    raw = isl.arena[at:at + o.dtype.itemsize].numpy().tobytes()
    return np.frombuffer(raw, dtype=o.dtype)[0]


def _fake(form, fault=None, name=None, distance=1):
    def call(isl):
        stray = None
        if fault == "read":
            o = form.op(name)
            v = _element(isl, o, isl.start[name] - distance * o.dtype.itemsize)
            use = C.STRAY_USE.get((form.entry, name))
            stray = use(v, form) if use else float(v)
        for out_name, arr in _reference_on(form, isl).items():
            isl.view(out_name).copy_(torch.from_numpy(np.array(arr)))
        if fault == "store":
            es = form.op(name).dtype.itemsize
            isl.arena[isl.end[name]:isl.end[name] + es] += 1
        if fault == "read":
            first = next(o for o in form.ops if o.kind in ("out", "inout"))
            flat = isl.view(first.name).reshape(-1)
            if first.dtype.kind == "f":
                flat[0] += stray
            else:
                add = 0 if np.isnan(stray) else int(stray)
                bits = 8 * first.dtype.itemsize
                v = (int(flat[0]) + add) % (1 << bits)
                flat[0] = v - (1 << bits) if first.dtype.kind == "i" and v >= 1 << (bits - 1) else v
    return call


def _run(form, *fault):
    return I.run_case(form.tag, C.island_operands(form, I, torch), _fake(form, *fault), C.island_expected(form, torch),
                      device="cpu", seed=form.seed, attribute=False)


@entries
def test_the_three_runs_notice_a_planted_fault(entry):
    form = C.forms(entry)[0]
    assert form.tag.endswith("least")
    clean = _run(form)
    assert clean.ok(), clean.lines()
    for o in form.ops:
        if o.kind in ("out", "inout", "ws"):
            r = _run(form, "store", o.name)
            for k in I.RUNS:
                assert any("margin of %s, back" % o.name in m and " 1 elements behind" in m for m in r.fails[k]), \
                    (o.name, k, r.fails[k])
        if o.kind == "in":
            distance = 1
            if (entry, o.name) in C.STRAY_USE:
                # a comparison launders the NaN of run N, and of run B's large values all but the sign: take the nearest
                # element in front of the input where run B planted a positive one
                isl = I.Islands(C.island_operands(form, I, torch), "B", "cpu", seed=form.seed)
                front = isl.arena[isl.start[o.name] - 64 * 4:isl.start[o.name]].view(torch.float32).flip(0)
                distance = 1 + int((front > 0).nonzero()[0])
            r = _run(form, "read", o.name, distance)
            assert not r.ok(), (entry, o.name, "a read %d elements in front of the input went unnoticed" % distance)
            assert any(m.startswith("output") for k in I.RUNS for m in r.fails[k])
            if C.STRAY_USE.get((entry, o.name)) is C._positive:
                assert r.ok("Z") and r.ok("N") and not r.ok("B")  # only run B sees a read that ends in `x >= threshold`
