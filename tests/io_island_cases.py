"""The island cases of the byte-oriented kernels (not a test module): the case tables, the operand generators and the CPU
references shared by tests/test_io_island_cases_cpu.py (the cases and the detector alone, no GPU) and
tests/test_gpu_io_islands.py (the kernels on islands, tests/islands.py).

An ENTRY is one C entry point of include/fosvos_hip.h; a FORM is one call of it: its operands, each at an offset from a
256-byte boundary, its scalar arguments and the structural properties it is listed for.  Every operand of a form sits at
the LEAST alignment its entry accepts (``ALIGN`` restates the FOSVOS_REQUIRE lines of csrc/ and the header: byte operands at
1 or 3, fp32 and int32 operands at 4, checked alignments at exactly what is checked), and every entry has one form with
everything at offset 0, where the 16-byte paths are taken.  Forms that take frames use N >= 2, so that a frame boundary
lies inside an operand.

``reference(form, inputs)`` maps the input arrays (name -> numpy array; an in-out operand's pre-fill is an input) to the
expected bits of every output, from the numpy and integer definitions under fosvos_amd/util and dataloaders.  The size
formulas of the workspaces and file slots are restated here (``*_bytes``); the GPU test asserts that the library reports
the same numbers, so a changed constant moves both or fails loudly.

The soft paint modes and the probability bytes round an fp64 value that goes through exp(): a byte whose fp64 value lies
within 1e-9 of its rounding boundary may be decided by an ulp of exp().  The generators pick, among seeded inputs, the
first whose band is empty (``props['band'] == 0``, asserted on the CPU), so the expected bits are exact everywhere."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import custom_transforms as T  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016, MEANVAL  # noqa: E402
from util import davis_measures as M  # noqa: E402
from util import experiment_helper, jpeg_layout, object_merge, online_adapt, png_layout  # noqa: E402
from util import frame_overlay as FO  # noqa: E402
from util import frame_resample as FR  # noqa: E402

U8, I32, F32 = np.uint8, np.int32, np.float32
BAND = 1e-9

# ---- constants of the kernels the shapes are derived from (csrc/): a changed constant fails the CPU test's properties
STREAM_GROUP_PX, STREAM_THREADS = 16, 256          # stream.hip: kGroup pixels a thread, threads a workgroup
SCALE_ROWS, SCALE_COLS, SCALE_CHUNK_PX = 4, 64, 1024  # stream.hip: kScaleRows, output columns, kScaleChunkPx
EVAL_THREADS = 256                                 # eval.hip: kEvalThreads
JF_TILE_ROWS, JF_TILE_WORDS, JF_WORD = 16, 8, 64   # eval.hip: kJfTileRows, kJfTileWords, pixels a word
PNG_SEG = png_layout.SEG_BYTES                     # png.hip: kSeg
PNG_WS_SEGMENT, PNG_WS_LENGTHS = 16, 288           # png.hip: kWsWords, kLenWords in bytes
JPEG_RI, JPEG_RI_420 = jpeg_layout.RI, jpeg_layout.RI_420
GATE_BATCH, GATE_COL_THREADS = 16, 64              # adapt.hip: kGateBatch, kGateColThreads

# ---- the least alignment every operand's entry accepts (FOSVOS_REQUIRE lines and include/fosvos_hip.h)
ALIGN = {
    "frame_prep": {"frames": 1, "image": 4},
    "overlay": {"frames": 1, "logits": 4, "out": 1},
    "frame_prep_scaled": {"frames": 1, "image": 4},
    "overlay_scaled": {"frames": 1, "logits": 4, "out": 1},
    "prob_bytes": {"logits": 4, "minmax": 4, "out": 1},
    "jf_counts": {"logits": 4, "gt": 1, "counts": 4, "workspace": 8},
    "jf_counts_labels": {"pred": 1, "gt": 1, "counts": 4, "workspace": 8},
    "merge_objects": {"map0": 4, "map1": 4, "map2": 4, "labels": 1},
    "png_encode": {"bytes": 1, "out": 1, "lengths": 4, "workspace": 4},
    "png_encode_indexed": {"bytes": 1, "palette": 1, "out": 1, "lengths": 4, "workspace": 4},
    "jpeg_encode": {"frames": 1, "out": 1, "lengths": 4, "workspace": 4},
    "augment_sample": {"frame": 1, "mask": 1, "col_taps": 16, "col_w": 16, "row_taps": 4, "row_w": 4, "col_near": 4,
                       "row_near": 4, "img_lut": 4, "gt_lut": 4, "image": 4, "gt": 4},
    "distance_gate": {"mask": 1, "out": 1, "workspace": 16},
    "adapt_labels": {"logits": 4, "last_mask": 1, "label": 4, "void_px": 1, "counts": 4, "workspace": 16},
}
ENTRIES = tuple(ALIGN)


class Op:
    """One operand of a form.  kind "in" / "inout": ``data`` is the numpy array; "out": shape and dtype; "ws": nbytes."""

    def __init__(self, name, kind, data=None, shape=None, dtype=None, offset=0):
        self.name, self.kind, self.offset = name, kind, offset
        self.data = None if data is None else np.ascontiguousarray(data)
        self.shape = tuple(self.data.shape if data is not None else shape)
        self.dtype = np.dtype(self.data.dtype if data is not None else dtype)


class Form:
    def __init__(self, entry, tag, ops, args=None, props=None):
        self.entry, self.tag, self.ops, self.args, self.props = entry, tag, ops, dict(args or {}), dict(props or {})
        self._expected = None

    def op(self, name):
        return next(o for o in self.ops if o.name == name)

    def has(self, name):
        return any(o.name == name for o in self.ops)

    def inputs(self):
        return {o.name: o.data for o in self.ops if o.kind in ("in", "inout")}

    def expected(self):
        """name -> numpy array, the bits every output (and in-out operand) must hold.  Computed once, never changed."""
        if self._expected is None:
            self._expected = reference(self, self.inputs())
            for a in self._expected.values():
                a.setflags(write=False)
        return self._expected

    @property
    def seed(self):
        return zlib.crc32((self.entry + " " + self.tag).encode()) & 0xFFFF


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _off(entry, name, least):
    """The offset of an operand: 0 in the aligned form, else the least alignment its entry accepts (a byte operand at 1)."""
    return ALIGN[entry][name] if least else 0


def _byte_off(entry, name, least, odd=1):
    return odd if least else 0


def _frames(n, h, w, key):
    f = _rng("frames", n, h, w, key).integers(0, 256, (n, h, w, 3), dtype=U8)
    flat = f.reshape(-1)
    flat[::7] = 0
    flat[3::11] = 255
    return f


def _logits(shape, key, zeros=True):
    """float32 of both signs, no value with 0 < |x| < 1e-6, with planted +0.0 and -0.0."""
    x = (3.0 * _rng("logits", shape, key).standard_normal(shape)).astype(F32)
    small = np.abs(x) < 1e-6
    x[small] = np.where(np.signbit(x[small]), F32(-2e-6), F32(2e-6))
    if zeros:
        flat = x.reshape(-1)
        flat[::5] = 0.0
        flat[2::13] = -0.0
    return x


# ====================================================================================================== references
def _ref_frame_prep(f, a, i):
    return {"image": np.concatenate([FO.prepare_frame(fr, bool(a["mirror"])) for fr in i["frames"]])}


def _ref_frame_prep_scaled(f, a, i):
    return {"image": np.concatenate([FR.prepare_frame_scaled(fr, a["Hn"], a["Wn"], bool(a["mirror"])) for fr in i["frames"]])}


_COLOR = {v: k for k, v in FO.COLOR_CHANNEL.items()}


def _paint(a, frame, logit, scaled):
    overlay_on, boolean = a["mode"] < 2, a["mode"] % 2 == 0
    if overlay_on:
        fn = FR.overlay_scaled if scaled else FO.overlay
        return fn(frame, logit, bool(a["mirror"]), boolean, _COLOR[a["channel"]], a["alpha"])
    if scaled:
        return FR.mask_bytes_scaled(logit, a["Hf"], a["Wf"], boolean)
    return FO.mask_bytes(logit, boolean)


def _ref_overlay(f, a, i, scaled=False):
    n = i["logits"].shape[0]
    frames = i.get("frames", [None] * n)
    return {"out": np.stack([_paint(a, frames[k], i["logits"][k, 0], scaled) for k in range(n)])}


def _ref_overlay_scaled(f, a, i):
    return _ref_overlay(f, a, i, True)


def prob_scaled(x):
    """(bytes, the clipped fp64 value in front of the rounding) of one frame: the fp64 definition of fosvos_prob_bytes."""
    p = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    cmin, cmax = p.min(), p.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1.0
    scaled = ((p - cmin) * (255.0 / cscale)).clip(0, 255)
    return (scaled + 0.5).astype(U8), scaled


def _ref_prob_bytes(f, a, i):
    x = i["logits"]
    out = np.stack([experiment_helper.bytescale(1.0 / (1.0 + np.exp(-x[k, 0].astype(np.float64)))) for k in range(x.shape[0])])
    assert np.array_equal(out, np.stack([prob_scaled(x[k, 0])[0] for k in range(x.shape[0])]))
    minmax = np.stack([np.array([x[k].min(), x[k].max()], dtype=F32) for k in range(x.shape[0])])
    return {"minmax": minmax, "out": out.astype(U8)}


def _ref_jf_counts(f, a, i):
    x, g = i["logits"], i["gt"]
    return {"counts": np.stack([M.jf_counts_numpy(x[k, 0] >= 0, g[k] != 0, a["radius"]) for k in range(x.shape[0])]).astype(I32)}


def _ref_jf_counts_labels(f, a, i):
    p, g = i["pred"], i["gt"]
    return {"counts": np.stack([object_merge.jf_counts_labels_numpy(p[k], g[k], a["K"], a["radius"])
                                for k in range(p.shape[0])]).astype(I32)}


def _ref_merge_objects(f, a, i):
    return {"labels": object_merge.merge_labels(np.stack([i["map%d" % k][:, 0] for k in range(a["K"])]))}


def _files_into(prefill, files, stride):
    out = prefill.copy()
    for n, data in enumerate(files):
        assert len(data) <= stride
        out[n * stride:n * stride + len(data)] = np.frombuffer(data, dtype=U8)
    return {"out": out, "lengths": np.array([len(d) for d in files], dtype=I32)}


def png_files(form, inputs):
    mode = png_layout.HUFFMAN_MODES[form.args["huffman"]]
    if form.entry == "png_encode_indexed":
        return [png_layout.encode_indexed(img, inputs["palette"], mode) for img in inputs["bytes"]]
    return [png_layout.encode(img, mode) for img in inputs["bytes"]]


def _ref_png(f, a, i):
    return _files_into(i["out"], png_files(f, i), a["capacity"])


def jpeg_files(form, inputs):
    a = form.args
    return [jpeg_layout.encode(fr, a["quality"], "4:2:0" if a["sampling"] == 420 else "4:4:4") for fr in inputs["frames"]]


def _ref_jpeg(f, a, i):
    return _files_into(i["out"], jpeg_files(f, i), a["out_stride"])


def _dataset():
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    return ds


def _ref_augment(f, a, i):
    """The numpy definition tests/test_gpu_resident_set.py compares with: convert, mirror, resize, to tensor."""
    image, gt = _dataset().convert_raw(i["frame"], i["mask"])
    if a["flip"]:
        image, gt = np.ascontiguousarray(image[:, ::-1]), np.ascontiguousarray(gt[:, ::-1])
    sc = a["scale"]
    image, gt = T.resize(image, sc, sc), T.resize(gt, sc, sc)
    return {"image": np.ascontiguousarray(image.transpose(2, 0, 1)[None]).astype(F32),
            "gt": np.ascontiguousarray(gt[None, None]).astype(F32)}


def _ref_distance_gate(f, a, i):
    return {"out": np.stack([online_adapt.far_from(m, a["distance"], bool(a["invert"])) for m in i["mask"]])}


def _ref_adapt_labels(f, a, i):
    res = [online_adapt.adapt_labels(i["logits"][k, 0], i["last_mask"][k], a["pos_logit"], a["neg_distance"], a["erode"])
           for k in range(i["logits"].shape[0])]
    return {"label": np.stack([r[0] for r in res])[:, None].astype(F32), "void_px": np.stack([r[1] for r in res])[:, None],
            "counts": np.stack([r[2] for r in res]).astype(I32)}


_REFERENCES = {"frame_prep": _ref_frame_prep, "overlay": _ref_overlay, "frame_prep_scaled": _ref_frame_prep_scaled,
               "overlay_scaled": _ref_overlay_scaled, "prob_bytes": _ref_prob_bytes, "jf_counts": _ref_jf_counts,
               "jf_counts_labels": _ref_jf_counts_labels, "merge_objects": _ref_merge_objects, "png_encode": _ref_png,
               "png_encode_indexed": _ref_png, "jpeg_encode": _ref_jpeg, "augment_sample": _ref_augment,
               "distance_gate": _ref_distance_gate, "adapt_labels": _ref_adapt_labels}


def reference(form, inputs):
    out = _REFERENCES[form.entry](form, form.args, inputs)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


# ====================================================================================================== 1. prep, overlay
PAINT_SHAPES = [(2, 5, 37), (1, 9, 461)]


def _soft_band(a, frame, logit, scaled):
    """How many pixels of one frame lie within BAND of the rounding boundary of a soft byte."""
    if a["mode"] % 2 == 0:
        return 0
    if scaled:
        p = FR.prediction_scaled(logit, a["Hf"], a["Wf"], False)
    else:
        p = FO.prediction(logit, False)
    if a["mode"] == 1:
        v = FO.mirrored(frame, bool(a["mirror"]))[:, :, a["channel"]].astype(np.float64) + (np.float64(a["alpha"]) * 255.0) * p
        return int(((np.abs(v - np.rint(v)) <= BAND) & (v < 255.0 + BAND)).sum())
    v = 255 * p + 0.5
    return int((np.abs(v - np.rint(v)) <= BAND).sum())


def _paint_form(entry, n, hf, wf, hn, wn, mode, mirror, least):
    scaled = entry == "overlay_scaled"
    a = {"N": n, "mirror": mirror, "mode": mode, "channel": (mode + mirror + hf) % 3, "alpha": 0.5 if mode == 1 else 1.0}
    a.update({"Hf": hf, "Wf": wf, "Hn": hn, "Wn": wn} if scaled else {"H": hf, "W": wf})
    for attempt in range(16):
        frames = _frames(n, hf, wf, (entry, attempt))
        # soft forms: no planted zeros (sigmoid(0) = 0.5 puts 255 p + 0.5 on an integer: 128 exactly, no ulp decides it)
        logits = _logits((n, 1, hn, wn), (entry, mode, attempt), zeros=mode % 2 == 0)
        band = sum(_soft_band(a, frames[k], logits[k, 0], scaled) for k in range(n))
        if band == 0:
            break
    ops = []
    if mode < 2:
        ops.append(Op("frames", "in", frames, offset=_byte_off(entry, "frames", least, 1)))
    ops.append(Op("logits", "in", logits, offset=_off(entry, "logits", least)))
    ops.append(Op("out", "out", shape=(n, hf, wf, 3) if mode < 2 else (n, hf, wf), dtype=U8, offset=_byte_off(entry, "out", least, 3)))
    tag = "%dx%dx%d%s mode%d mirror%d %s" % (n, hf, wf, " net %dx%d" % (hn, wn) if scaled else "", mode, mirror,
                                            "least" if least else "aligned")
    return Form(entry, tag, ops, a, {"band": band, "attempt": attempt})


def _prep_form(entry, n, hf, wf, hn, wn, mirror, least):
    scaled = entry == "frame_prep_scaled"
    a = {"N": n, "mirror": mirror}
    a.update({"Hf": hf, "Wf": wf, "Hn": hn, "Wn": wn} if scaled else {"H": hf, "W": wf})
    ops = [Op("frames", "in", _frames(n, hf, wf, entry), offset=_byte_off(entry, "frames", least, 3)),
           Op("image", "out", shape=(n, 3, hn, wn), dtype=F32, offset=_off(entry, "image", least))]
    tag = "%dx%dx%d%s mirror%d %s" % (n, hf, wf, " net %dx%d" % (hn, wn) if scaled else "", mirror, "least" if least else "aligned")
    return Form(entry, tag, ops, a)


def forms_frame_prep():
    out = [_prep_form("frame_prep", n, h, w, h, w, m, True) for n, h, w in PAINT_SHAPES for m in (0, 1)]
    return out + [_prep_form("frame_prep", 2, 5, 37, 5, 37, 0, False)]


def forms_overlay():
    out = [_paint_form("overlay", n, h, w, h, w, mode, m, True) for n, h, w in PAINT_SHAPES for mode in range(4) for m in (0, 1)]
    return out + [_paint_form("overlay", 2, 5, 37, 5, 37, mode, 1, False) for mode in (0, 3)]


# ====================================================================================================== 2. the scaled pair
SCALED_SHAPES = [(2, 23, 150, 10, 67), (2, 6, 1100, 5, 70), (2, 5, 37, 5, 37)]


def forms_frame_prep_scaled():
    out = [_prep_form("frame_prep_scaled", *s, m, True) for s in SCALED_SHAPES for m in (0, 1)]
    return out + [_prep_form("frame_prep_scaled", *SCALED_SHAPES[0], 1, False)]


def forms_overlay_scaled():
    out = [_paint_form("overlay_scaled", *s, mode, m, True) for s in SCALED_SHAPES for mode in range(4) for m in (0, 1)]
    return out + [_paint_form("overlay_scaled", *SCALED_SHAPES[0], mode, 0, False) for mode in (1, 2)]


# ====================================================================================================== 3. prob_bytes
def _prob_form(n, h, w, least, constant_frame):
    for attempt in range(16):
        x = _logits((n, 1, h, w), ("prob", attempt), zeros=False)
        if constant_frame is not None:
            x[constant_frame] = F32(-0.25)
        band = 0
        for k in range(n):
            frac = (prob_scaled(x[k, 0])[1] + 0.5) % 1.0
            band += int(((frac < BAND) | (frac > 1.0 - BAND)).sum()) if x[k].min() != x[k].max() else 0
        if band == 0:
            break
    ops = [Op("logits", "in", x, offset=_off("prob_bytes", "logits", least)),
           Op("minmax", "out", shape=(n, 2), dtype=F32, offset=_off("prob_bytes", "minmax", least)),
           Op("out", "out", shape=(n, h, w), dtype=U8, offset=_byte_off("prob_bytes", "out", least, 3))]
    return Form("prob_bytes", "%dx%dx%d %s" % (n, h, w, "least" if least else "aligned"), ops, {"N": n, "H": h, "W": w},
                {"band": band, "constant_frame": constant_frame})


def forms_prob_bytes():
    return [_prob_form(2, 5, 37, True, 1), _prob_form(2, 8, 40, False, None), _prob_form(1, 33, 130, True, None)]


# ====================================================================================================== 4. J and F counts
JF_SHAPES = [(2, 19, 70), (1, 17, 530)]
JF_RADII = (1, 8, 63)
JF_K = 3


def jf_workspace_bytes(n, h, w, k=1):
    return 2 * n * k * h * (-(-w // JF_WORD)) * 8


def _blob_mask(h, w, key, density=0.35):
    """A ragged mask: an ellipse xor seeded speckle, so that the contours are long and cross words, rows and tiles."""
    y, x = np.mgrid[0:h, 0:w]
    r = _rng("blob", h, w, key)
    cy, cx = h * (0.35 + 0.3 * r.random()), w * (0.3 + 0.4 * r.random())
    inside = ((y - cy) / (0.4 * h + 1)) ** 2 + ((x - cx) / (0.3 * w + 1)) ** 2 <= 1
    return inside ^ (r.random((h, w)) < density * 0.2)


def _jf_form(n, h, w, radius, least):
    pred = np.stack([_blob_mask(h, w, ("pred", k)) for k in range(n)])
    gt = np.stack([_blob_mask(h, w, ("gt", k)) for k in range(n)])
    mag = (0.5 + 3.0 * _rng("jf", n, h, w).random((n, h, w))).astype(F32)
    logits = np.where(pred, mag, -mag).astype(F32)[:, None]
    logits[:, 0, ::3, ::4] = np.where(pred[:, ::3, ::4], F32(0.0), F32(-1e-30))  # exactly 0 is object
    gtb = (gt * (1 + 127 * (np.arange(n) % 3))[:, None, None]).astype(U8)         # any non-zero byte counts
    e = "jf_counts"
    ops = [Op("logits", "in", logits, offset=_off(e, "logits", least)), Op("gt", "in", gtb, offset=_byte_off(e, "gt", least, 3)),
           Op("counts", "out", shape=(n, 6), dtype=I32, offset=_off(e, "counts", least)),
           Op("workspace", "ws", shape=(jf_workspace_bytes(n, h, w),), dtype=U8, offset=_off(e, "workspace", least))]
    return Form(e, "%dx%dx%d r%d %s" % (n, h, w, radius, "least" if least else "aligned"), ops,
                {"N": n, "H": h, "W": w, "radius": radius})


def _label_map(n, h, w, key):
    lab = np.zeros((n, h, w), U8)
    for k in range(n):
        for obj in range(1, JF_K + 2):  # one label above K: it belongs to no object
            lab[k][_blob_mask(h, w, (key, k, obj), density=0.1) & (_rng(key, k, obj).random((h, w)) < 0.6)] = obj
    return lab


def _jf_labels_form(n, h, w, radius, least):
    e = "jf_counts_labels"
    ops = [Op("pred", "in", _label_map(n, h, w, "p"), offset=_byte_off(e, "pred", least, 1)),
           Op("gt", "in", _label_map(n, h, w, "g"), offset=_byte_off(e, "gt", least, 3)),
           Op("counts", "out", shape=(n, JF_K, 6), dtype=I32, offset=_off(e, "counts", least)),
           Op("workspace", "ws", shape=(jf_workspace_bytes(n, h, w, JF_K),), dtype=U8, offset=_off(e, "workspace", least))]
    return Form(e, "%dx%dx%d K%d r%d %s" % (n, h, w, JF_K, radius, "least" if least else "aligned"), ops,
                {"N": n, "K": JF_K, "H": h, "W": w, "radius": radius})


def forms_jf_counts():
    return [_jf_form(*s, r, True) for s in JF_SHAPES for r in JF_RADII] + [_jf_form(*JF_SHAPES[0], 8, False)]


def forms_jf_counts_labels():
    return [_jf_labels_form(*s, r, True) for s in JF_SHAPES for r in JF_RADII] + [_jf_labels_form(*JF_SHAPES[0], 8, False)]


# ====================================================================================================== 5. merge_objects
def _merge_form(k_maps, n, h, w, least):
    e = "merge_objects"
    maps = [_logits((n, 1, h, w), ("merge", k), zeros=True) for k in range(k_maps)]
    if k_maps > 1:
        maps[1][:, 0, ::2, ::3] = maps[0][:, 0, ::2, ::3]      # ties between maps 0 and 1 (some of them >= 0)
        maps[2][:, 0, 1::2, 1::5] = maps[1][:, 0, 1::2, 1::5]  # and between 1 and 2 (off the planted zeros)
    for m in maps:
        m[:, 0, 0, 1] = -1.0                                   # a pixel with no logit >= 0
    ops = [Op("map%d" % k, "in", maps[k], offset=_off(e, "map%d" % k, least)) for k in range(k_maps)]
    ops.append(Op("labels", "out", shape=(n, h, w), dtype=U8, offset=_byte_off(e, "labels", least, 3)))
    return Form(e, "K%d %dx%dx%d %s" % (k_maps, n, h, w, "least" if least else "aligned"), ops, {"K": k_maps, "N": n, "H": h, "W": w})


def forms_merge_objects():
    return [_merge_form(k, 2, 5, 37, True) for k in (1, 3)] + [_merge_form(k, 2, 8, 40, False) for k in (1, 3)]


# ====================================================================================================== 6. PNG files
PNG_SHAPES = [(2, 3, 5), (2, 64, 63), (2, 65, 63)]
PNG_CONTENTS = ("constant", "noise", "blobs")
PREFILLS = (0, 1)


def png_capacity_bytes(h, w, indexed=False):
    return png_layout.max_file_bytes_indexed(h, w) if indexed else png_layout.max_file_bytes(h, w)


def png_workspace_bytes(n, h, w, huffman):
    return n * png_layout.n_segments(h, w) * (PNG_WS_SEGMENT + (PNG_WS_LENGTHS if huffman else 0))


def _png_image(content, n, h, w, indexed):
    if content == "constant":
        return np.stack([np.full((h, w), 200 if k else 0, U8) for k in range(n)])
    if content == "noise":
        return _rng("png noise", n, h, w).integers(0, 256, (n, h, w), dtype=U8)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        if indexed:  # label blobs 0..3
            img = np.zeros((h, w), U8)
            for obj in (1, 2, 3):
                img[((y - h * 0.3 * obj + k) / (0.25 * h + 1)) ** 2 + ((x - w * 0.25 * obj) / (0.2 * w + 1)) ** 2 <= 1] = obj
        else:        # smooth blobs like a probability map
            d = ((y - 0.45 * h - k) / (0.3 * h + 1)) ** 2 + ((x - 0.5 * w + 2 * k) / (0.28 * w + 1)) ** 2
            img = (255.0 / (1.0 + np.exp(6.0 * (d - 1.0))) + 0.5).astype(U8)
        out.append(img)
    return np.stack(out)


def _file_offset(stride):
    """1 or 3: the one at which the second frame's slot does not begin on a 4-byte boundary either."""
    return 1 if (1 + stride) % 4 else 3


def _prefill(nbytes, key):
    return _rng("prefill", key).integers(0, 256, nbytes, dtype=U8)


def _png_form(entry, n, h, w, content, huffman, prefill, least=True):
    indexed = entry == "png_encode_indexed"
    cap = png_capacity_bytes(h, w, indexed)
    ops = [Op("bytes", "in", _png_image(content, n, h, w, indexed), offset=_byte_off(entry, "bytes", least, 3))]
    if indexed:
        ops.append(Op("palette", "in", object_merge.davis_palette(), offset=_byte_off(entry, "palette", least, 1)))
    ops += [Op("out", "inout", _prefill(n * cap, (entry, h, w, prefill)), offset=_file_offset(cap) if least else 0),
            Op("lengths", "out", shape=(n,), dtype=I32, offset=_off(entry, "lengths", least)),
            Op("workspace", "ws", shape=(png_workspace_bytes(n, h, w, huffman),), dtype=U8, offset=_off(entry, "workspace", least))]
    tag = "%dx%dx%d %s huffman%d prefill%d %s" % (n, h, w, content, huffman, prefill, "least" if least else "aligned")
    return Form(entry, tag, ops, {"N": n, "H": h, "W": w, "huffman": huffman, "capacity": cap},
                {"content": content, "prefill": prefill})


def _png_forms(entry):
    out = [_png_form(entry, *s, c, hm, p) for s in PNG_SHAPES for c in PNG_CONTENTS for hm in (0, 1) for p in PREFILLS]
    return out + [_png_form(entry, *PNG_SHAPES[2], "blobs", 1, 0, least=False)]


def forms_png_encode():
    return _png_forms("png_encode")


def forms_png_encode_indexed():
    return _png_forms("png_encode_indexed")


# ====================================================================================================== 7. JPEG files
JPEG_KINDS = {"colour444": (3, 444, [(2, 9, 13), (2, 8, 264)]), "grey": (1, 444, [(2, 9, 13), (2, 8, 264)]),
              "colour420": (3, 420, [(2, 17, 35), (2, 16, 272)])}
JPEG_QUALITIES = (100, 30)
JPEG_CONTENTS = ("noise", "flat")


def _sampling_name(components, sampling):
    return "4:2:0" if sampling == 420 and components == 3 else "4:4:4"


def jpeg_capacity_bytes(h, w, components, sampling):
    return jpeg_layout.capacity(h, w, components, _sampling_name(components, sampling))


def jpeg_workspace_bytes(n, h, w, components, sampling):
    return 4 * n * jpeg_layout.n_intervals(h, w, _sampling_name(components, sampling))


def _jpeg_form(kind, n, h, w, quality, content, prefill, least=True):
    e = "jpeg_encode"
    comps, sampling, _ = JPEG_KINDS[kind]
    shape = (n, h, w, 3) if comps == 3 else (n, h, w)
    if content == "noise":
        frames = _rng("jpeg", kind, h, w).integers(0, 256, shape, dtype=U8)
    else:
        frames = np.empty(shape, U8)
        for k in range(n):
            frames[k] = np.array([40, 200, 90], U8)[:comps] + 17 * k if comps == 3 else 128 + 31 * k
    stride = jpeg_capacity_bytes(h, w, comps, sampling)
    ops = [Op("frames", "in", frames, offset=_byte_off(e, "frames", least, 1)),
           Op("out", "inout", _prefill(n * stride, (kind, h, w, prefill)), offset=1 if least else 0),
           Op("lengths", "out", shape=(n,), dtype=I32, offset=_off(e, "lengths", least)),
           Op("workspace", "ws", shape=(jpeg_workspace_bytes(n, h, w, comps, sampling),), dtype=U8, offset=_off(e, "workspace", least))]
    tag = "%s %dx%dx%d q%d %s prefill%d %s" % (kind, n, h, w, quality, content, prefill, "least" if least else "aligned")
    return Form(e, tag, ops, {"N": n, "H": h, "W": w, "components": comps, "sampling": sampling, "quality": quality,
                              "out_stride": stride}, {"kind": kind, "content": content, "prefill": prefill})


def forms_jpeg_encode():
    out = [_jpeg_form(kind, *s, q, c, p) for kind, (_, _, shapes) in JPEG_KINDS.items() for s in shapes for q in JPEG_QUALITIES
           for c in JPEG_CONTENTS for p in PREFILLS]
    return out + [_jpeg_form("colour420", 2, 17, 35, 100, "noise", 0, least=False)]


# ====================================================================================================== 8. augment_sample
AUGMENT_SIZES = [((13, 17), 0.77, (10, 13)), ((13, 17), 1.56, (20, 27)), ((24, 40), 1, (24, 40))]
_AUG_TABLES = (("col_taps", I32), ("col_w", F32), ("row_taps", I32), ("row_w", F32), ("col_near", I32), ("row_near", I32))


def _augment_form(size, scale, out_size, flip, least):
    e = "augment_sample"
    h, w = size
    r = _rng("augment", size)
    frame = r.integers(0, 256, (h, w, 3), dtype=U8)
    mask = np.where(r.random((h, w)) > 0.5, 255, 0).astype(U8)
    mask[h // 3:, :w // 2] = 128
    plan = T.resize_plan(h, w, scale, scale)
    assert (plan["oh"], plan["ow"]) == tuple(out_size)
    oh, ow = out_size
    ramp = np.repeat(np.arange(256, dtype=U8)[:, None, None], 3, axis=2)
    img_lut = np.ascontiguousarray(_dataset().convert_raw(ramp, None)[0].reshape(256, 3)).astype(F32)
    gt_lut = (np.arange(256, dtype=F32) / F32(max(float(mask.max()), 1e-8))).astype(F32)
    ops = [Op("frame", "in", frame, offset=7 if least else 0), Op("mask", "in", mask, offset=12 if least else 0)]
    if not plan["copy"]:
        ops += [Op(name, "in", np.ascontiguousarray(plan[name], dtype=dt), offset=_off(e, name, least)) for name, dt in _AUG_TABLES]
    ops += [Op("img_lut", "in", img_lut, offset=_off(e, "img_lut", least)), Op("gt_lut", "in", gt_lut, offset=_off(e, "gt_lut", least)),
            Op("image", "out", shape=(1, 3, oh, ow), dtype=F32, offset=_off(e, "image", least)),
            Op("gt", "out", shape=(1, 1, oh, ow), dtype=F32, offset=_off(e, "gt", least))]
    tag = "%dx%d -> %dx%d flip%d %s" % (h, w, oh, ow, flip, "least" if least else "aligned")
    return Form(e, tag, ops, {"H": h, "W": w, "OH": oh, "OW": ow, "flip": flip, "scale": scale}, {"copy": plan["copy"]})


def forms_augment_sample():
    out = [_augment_form(*s, flip, True) for s in AUGMENT_SIZES for flip in (0, 1)]
    return out + [_augment_form(*AUGMENT_SIZES[0], 1, False)]


# ====================================================================================================== 9. gate, labels
GATE_SHAPES = [(2, 19, 70), (1, 33, 130)]
GATE_DISTANCES = (0, 1, 5, 200)   # 200: larger than both sides of every shape
ERODES = (0, 2)


def gate_workspace_bytes(n, h, w, labels=False):
    r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    return r16(4 * n) + r16(2 * n * h * w) + (n * h * w if labels else 0)


def _ellipse(h, w):
    y, x = np.mgrid[0:h, 0:w]
    m = ((((y - 0.45 * h) / (0.2 * h + 0.5)) ** 2 + ((x - 0.5 * w) / (0.16 * w + 0.5)) ** 2) <= 1.0).astype(U8) * 7
    m[0, w - 1] = 1  # a stray pixel
    return m


def gate_masks(n, h, w, which):
    """uint8 [N,H,W].  N = 2: set "a" = (ellipse with a stray pixel, empty), set "b" = (full, one corner pixel)."""
    corner = np.zeros((h, w), U8)
    corner[h - 1, w - 1] = 1
    frames = {"a": [_ellipse(h, w), np.zeros((h, w), U8)], "b": [np.full((h, w), 255, U8), corner]}[which]
    return np.stack(frames[:n])


def _mask_sets(n):
    return ("a", "b") if n == 2 else ("a",)


def _gate_form(n, h, w, distance, invert, which, least):
    e = "distance_gate"
    ops = [Op("mask", "in", gate_masks(n, h, w, which), offset=_byte_off(e, "mask", least, 1)),
           Op("out", "out", shape=(n, h, w), dtype=U8, offset=_byte_off(e, "out", least, 3)),
           Op("workspace", "ws", shape=(gate_workspace_bytes(n, h, w),), dtype=U8, offset=_off(e, "workspace", least))]
    tag = "%dx%dx%d masks %s d%d invert%d %s" % (n, h, w, which, distance, invert, "least" if least else "aligned")
    return Form(e, tag, ops, {"N": n, "H": h, "W": w, "distance": distance, "invert": invert}, {"masks": which})


def forms_distance_gate():
    out = [_gate_form(n, h, w, d, inv, which, True) for n, h, w in GATE_SHAPES for d in GATE_DISTANCES for inv in (0, 1)
           for which in _mask_sets(n)]
    return out + [_gate_form(2, 19, 70, 5, 0, "a", False)]


def _adapt_form(n, h, w, neg_distance, erode, which, least):
    e = "adapt_labels"
    masks = gate_masks(n, h, w, which)
    r = _rng("adapt", n, h, w)
    x = (np.where(np.roll(masks, 3, axis=2) != 0, 6.0, -6.0) + r.normal(0.0, 3.0, (n, h, w))).astype(F32)[:, None]
    pos_logit = float(F32(np.log(0.97 / 0.03)))
    x[:, 0, 1, 2] = F32(pos_logit)  # equality counts
    ops = [Op("logits", "in", x, offset=_off(e, "logits", least)), Op("last_mask", "in", masks, offset=_byte_off(e, "last_mask", least, 3)),
           Op("label", "out", shape=(n, 1, h, w), dtype=F32, offset=_off(e, "label", least)),
           Op("void_px", "out", shape=(n, 1, h, w), dtype=U8, offset=_byte_off(e, "void_px", least, 1)),
           Op("counts", "out", shape=(n, 3), dtype=I32, offset=_off(e, "counts", least)),
           Op("workspace", "ws", shape=(gate_workspace_bytes(n, h, w, True),), dtype=U8, offset=_off(e, "workspace", least))]
    tag = "%dx%dx%d masks %s D%d E%d %s" % (n, h, w, which, neg_distance, erode, "least" if least else "aligned")
    return Form(e, tag, ops, {"N": n, "H": h, "W": w, "pos_logit": pos_logit, "neg_distance": neg_distance, "erode": erode},
                {"masks": which})


def forms_adapt_labels():
    out = [_adapt_form(n, h, w, d, e, which, True) for n, h, w in GATE_SHAPES for d in GATE_DISTANCES for e in ERODES
           for which in _mask_sets(n)]
    return out + [_adapt_form(2, 19, 70, 5, 2, "a", False)]


# ====================================================================================================== the table
_FORMS = {"frame_prep": forms_frame_prep, "overlay": forms_overlay, "frame_prep_scaled": forms_frame_prep_scaled,
          "overlay_scaled": forms_overlay_scaled, "prob_bytes": forms_prob_bytes, "jf_counts": forms_jf_counts,
          "jf_counts_labels": forms_jf_counts_labels, "merge_objects": forms_merge_objects, "png_encode": forms_png_encode,
          "png_encode_indexed": forms_png_encode_indexed, "jpeg_encode": forms_jpeg_encode,
          "augment_sample": forms_augment_sample, "distance_gate": forms_distance_gate, "adapt_labels": forms_adapt_labels}
assert tuple(_FORMS) == ENTRIES
_CACHE = {}


def forms(entry):
    """The forms of one entry, built once (and with them their expected bits) and shared by whoever asks."""
    if entry not in _CACHE:
        _CACHE[entry] = _FORMS[entry]()
        tags = [f.tag for f in _CACHE[entry]]
        assert len(set(tags)) == len(tags), entry
    return _CACHE[entry]


# ====================================================================================================== islands
def island_operands(form, I, torch):
    """The form's operands as tests/islands.py operands (all of them flat: 64 KiB of margin on either side)."""
    out = []
    for o in form.ops:
        if o.kind == "in":
            out.append(I.inp(o.name, torch.from_numpy(o.data), is_map=False, offset=o.offset))
        elif o.kind == "inout":
            out.append(I.inout(o.name, torch.from_numpy(o.data), is_map=False, offset=o.offset))
        elif o.kind == "out":
            out.append(I.out(o.name, o.shape, getattr(torch, o.dtype.name), is_map=False, offset=o.offset))
        else:
            out.append(I.workspace(o.name, o.shape[0], offset=o.offset))
    return out


def island_expected(form, torch):
    return {k: torch.from_numpy(np.array(v)) for k, v in form.expected().items()}


# How a stray element of an fp32 input would enter the output, by the operation's own use of that input: a comparison
# launders a NaN, and only the sign of a large value survives it.  Byte and table inputs are taken as integers.
def _threshold(v, form):
    return float(v >= 0)


def _sigmoid_byte(v, form):
    p = 1.0 / (1.0 + np.exp(-np.float64(v)))
    return 0.0 if np.isnan(p) else float(int(255 * p + 0.5))


def _positive(v, form):
    return float(v >= F32(form.args["pos_logit"]))


STRAY_USE = {("overlay", "logits"): _threshold, ("overlay_scaled", "logits"): _threshold, ("prob_bytes", "logits"): _sigmoid_byte,
             ("jf_counts", "logits"): _threshold, ("merge_objects", "map0"): _threshold, ("merge_objects", "map1"): _threshold,
             ("merge_objects", "map2"): _threshold, ("adapt_labels", "logits"): _positive}
