"""Block matching and the mask warp on a real MI355X: ``ops.motion_luma`` / ``motion_estimate`` / ``motion_warp``
(csrc/motion.hip) against the numpy definition (util/block_motion.py) - exact equality, no tolerance anywhere -, the three
entries on islands, their argument faults, ``test_fast(clean=, motion=)`` on the real seeded OSVOS_VGG and
``FrameSegmenter(clean=, motion=)``.  tests/block_motion_cases.py holds the shapes, the contents and the definition's
answers, each computed once."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_motion_cases as C  # noqa: E402
import islands as I  # noqa: E402
import mask_crf_cases as CC  # noqa: E402
import test_ensemble_cases as EC  # noqa: E402
import test_gpu_test_pass_calls as PC  # noqa: E402
from util import block_motion as B, experiment_helper, frame_overlay as F, frame_resample as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8, I8, I32 = torch.uint8, torch.int8, torch.int32


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the shared references are read-only


def options(block=16, search=8, zero_bias=8):
    from fosvos_hip.options import MotionOptions
    return MotionOptions(block=block, search=search, zero_bias=zero_bias)


# ------------------------------------------------------------------------------------------ the ops against the definition
@pytest.mark.parametrize("content", list(C.CONTENTS))
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.SHAPE_IDS)
def test_estimate_is_the_definition(shape, content):
    from fosvos_hip import ops
    missed = []
    for n in C.BATCHES:
        for block in C.BLOCKS:
            for search in C.SEARCHES:
                prev, cur, field, cost = C.reference(content, n, shape, block, search)
                prev_t, cur_t = dev(prev), dev(cur)
                got_f, got_c = ops.motion_estimate(prev_t, cur_t, options(block, search, C.CONTENTS[content]))
                assert got_f.dtype == I8 and got_c.dtype == I32
                assert tuple(got_f.shape) == field.shape and tuple(got_c.shape) == cost.shape
                gf, gc = got_f.cpu().numpy(), got_c.cpu().numpy()
                if not (np.array_equal(gf, field) and np.array_equal(gc, cost)):
                    bad = np.argwhere((gf != field).any(-1) | (gc != cost))
                    k = tuple(bad[0])
                    missed.append("n %d block %d search %d: %d blocks differ, first %s: (%s, %d) for (%s, %d)" % (
                        n, block, search, len(bad), k, tuple(gf[k]), gc[k], tuple(field[k]), cost[k]))
                assert np.array_equal(prev_t.cpu().numpy(), prev) and np.array_equal(cur_t.cpu().numpy(), cur)
    assert not missed, (shape, content, missed)


def test_the_contents_exercise_what_they_are_for():
    """On the host: the planted shift is the two-tile case's answer wherever it can be, the ties are ties, and the largest
    score there is reaches the key."""
    h, w = C.TWO_TILES
    assert h > 2 * C.TILE[0] and w > 2 * C.TILE[1] and h % C.TILE[0] and w % C.TILE[1] and h % 8 and w % 8
    _, _, field, cost = C.reference("planted", 1, C.TWO_TILES, 16, 16)
    inside = C.inside_blocks(h, w, 16, C.SHIFT)
    assert inside.sum() >= 8 and (field[0][inside] == np.array(C.SHIFT, np.int8)).all() and not cost[0][inside].any()
    _, _, field, cost = C.reference("opposite", 1, C.TWO_TILES, 16, 16)
    assert not field.any() and cost.max() == 255 * 256
    _, _, field, cost = C.reference("checker", 1, C.TWO_TILES, 16, 7)
    assert (np.abs(field.astype(int)).sum(-1) == 1).all() and not cost.any()


def test_luma_is_the_definition():
    from fosvos_hip import ops
    for n, h, w in ((2, 19, 70), (1,) + C.TWO_TILES):
        image = CC.image(n, h, w, "nonfinite")
        assert not np.isfinite(image).all()
        got = ops.motion_luma(dev(image))
        assert got.dtype == U8 and tuple(got.shape) == (n, h, w)
        assert np.array_equal(got.cpu().numpy(), B.luma(image))
    scaled = R.prepare_frame_scaled(np.random.default_rng(4).integers(0, 256, (38, 140, 3), dtype=np.uint8), 19, 70)   # averaged bytes
    assert np.array_equal(ops.motion_luma(dev(scaled)).cpu().numpy(), B.luma(scaled))


@pytest.mark.parametrize("block", C.BLOCKS)
def test_warp_is_the_definition(block):
    from fosvos_hip import ops
    for n, (h, w) in ((1, (5, 7)), (2, (19, 70)), (3, C.TWO_TILES)):
        rng = np.random.default_rng([n, h, w])
        mask = (rng.integers(0, 3, (n, h, w), dtype=np.uint8) * 127).astype(np.uint8)     # 0, 127 and 254: non-zero is set
        field = C.random_field(n, h, w, block)
        assert field.max() == 127 and (field.min() == -128 or field.size == 2)     # (a frame of one block holds one vector)
        want = np.stack([B.warp(mask[k], field[k], block) for k in range(n)])
        mask_t = dev(mask)
        got = ops.motion_warp(mask_t, dev(field), block)
        assert got.dtype == U8 and np.array_equal(got.cpu().numpy(), want) and (want.max() == 1 or field.size == 2)
        assert np.array_equal(mask_t.cpu().numpy(), mask)


def test_the_ops_write_into_the_callers_tensors():
    from fosvos_hip import ops
    prev, cur, field, cost = C.reference("random", 3, (37, 150), 16, 7)
    o = options(16, 7)
    f = torch.full(field.shape, 99, dtype=I8, device=DEV)
    c = torch.full(cost.shape, -1, dtype=I32, device=DEV)
    got = ops.motion_estimate(dev(prev), dev(cur), o, field=f, cost=c)
    assert got[0] is f and got[1] is c and np.array_equal(f.cpu().numpy(), field) and np.array_equal(c.cpu().numpy(), cost)
    # consecutive planes of ONE buffer: two views one frame apart, as the test pass hands them over
    planes = dev(np.concatenate([prev[:1], cur]))
    want = B.estimate(planes[:-1].cpu().numpy(), planes[1:].cpu().numpy(), options=o)
    got = ops.motion_estimate(planes[:-1], planes[1:], o, field=f, cost=c)
    assert np.array_equal(f.cpu().numpy(), want[0]) and np.array_equal(c.cpu().numpy(), want[1])
    default = ops.motion_estimate(dev(prev), dev(cur))
    assert np.array_equal(default[0].cpu().numpy(), B.estimate(prev, cur)[0])
    image = CC.image(2, 19, 70, "random")
    y = torch.full((2, 19, 70), 7, dtype=U8, device=DEV)
    assert ops.motion_luma(dev(image), out=y) is y and np.array_equal(y.cpu().numpy(), B.luma(image))
    mask, fld = dev(np.ones((1, 19, 70), np.uint8)), dev(C.random_field(1, 19, 70, 8))
    out = torch.full((1, 19, 70), 9, dtype=U8, device=DEV)
    assert ops.motion_warp(mask, fld, 8, out=out) is out
    assert np.array_equal(out.cpu().numpy()[0], B.warp(np.ones((19, 70), np.uint8), fld.cpu().numpy()[0], 8))


# ------------------------------------------------------------------------------------------ islands
@pytest.mark.parametrize("shape", [(19, 70), C.TWO_TILES], ids=["19x70", "two_tiles"])
def test_the_entries_touch_nothing_outside_their_operands(shape):
    """Search 16: the halo reaches past every edge of the frame, and past the first and the last frame of the batch.  The int8
    field travels as its bytes (the island helper knows byte operands)."""
    import fosvos_hip
    from fosvos_hip import check, ops
    L = fosvos_hip.lib()
    n, (h, w) = 2, shape
    stream = torch.cuda.current_stream(0).cuda_stream
    report = I.Report("motion %dx%dx%d" % (n, h, w))
    for block in C.BLOCKS:
        prev, cur, field, cost = C.reference("random", n, shape, block, 16)
        operands = [I.inp("prev", torch.from_numpy(prev.copy()), is_map=False, offset=1), I.inp("cur", torch.from_numpy(cur.copy()), is_map=False, offset=3),
                    I.out("field", field.shape, U8, is_map=False, offset=1), I.out("cost", cost.shape, I32, is_map=False, offset=4)]

        def estimate(isl):
            check(L.fosvos_motion_estimate(isl.ptr("prev"), isl.ptr("cur"), n, h, w, block, 16, 8, isl.ptr("field"), isl.ptr("cost"), 0,
                                           stream), "motion_estimate")
        report.add(I.run_case("estimate block %d" % block, operands, estimate,
                              {"field": torch.from_numpy(field.copy()).view(U8), "cost": torch.from_numpy(cost.copy())}, device=DEV, seed=block))
        mask = (np.random.default_rng(block).integers(0, 2, (n, h, w), dtype=np.uint8) * 255).astype(np.uint8)
        fld = C.random_field(n, h, w, block)
        want = np.stack([B.warp(mask[k], fld[k], block) for k in range(n)])
        operands = [I.inp("mask", torch.from_numpy(mask), is_map=False, offset=1), I.inp("field", torch.from_numpy(fld).view(U8), is_map=False, offset=1),
                    I.out("out", (n, h, w), U8, is_map=False, offset=3)]

        def warp(isl):
            check(L.fosvos_motion_warp(isl.ptr("mask"), isl.ptr("field"), n, h, w, block, isl.ptr("out"), 0, stream), "motion_warp")
        report.add(I.run_case("warp block %d" % block, operands, warp, {"out": torch.from_numpy(want)}, device=DEV, seed=block))
    image = CC.image(n, h, w, "nonfinite")
    operands = [I.inp("image", torch.from_numpy(image), is_map=False, offset=4), I.out("out", (n, h, w), U8, is_map=False, offset=1)]

    def luma(isl):
        check(L.fosvos_motion_luma(isl.ptr("image"), ops._mean_bgr(), n, h, w, isl.ptr("out"), 0, stream), "motion_luma")
    report.add(I.run_case("luma", operands, luma, {"out": torch.from_numpy(B.luma(image))}, device=DEV, seed=1))
    report.done()


# ------------------------------------------------------------------------------------------ argument faults
def test_a_fault_raises_before_any_launch():
    from fosvos_hip import ops
    plane = torch.zeros((2, 19, 70), dtype=U8, device=DEV)
    field = torch.zeros((2, 2, 5, 2), dtype=I8, device=DEV)
    image = torch.zeros((2, 3, 19, 70), device=DEV)
    faults = [
        (lambda: ops.motion_luma(image[:, :2]), ValueError, "contiguous"),
        (lambda: ops.motion_luma(image[0]), ValueError, r"\[N,3,H,W\]"),
        (lambda: ops.motion_luma(image.double()), ValueError, "expected torch.float32"),
        (lambda: ops.motion_luma(image, out=plane[:1]), ValueError, "out must be"),
        (lambda: ops.motion_luma(image.cpu()), RuntimeError, "tensor must live on the GPU"),
        (lambda: ops.motion_estimate(plane, plane[:1]), ValueError, "cur_y must be"),
        (lambda: ops.motion_estimate(plane.int(), plane), ValueError, "expected torch.uint8"),
        (lambda: ops.motion_estimate(plane, plane, {"block": 16}), ValueError, "MotionOptions"),
        (lambda: ops.motion_estimate(plane, plane, field=field.view(2, 2, 10)), ValueError, "field must be"),
        (lambda: ops.motion_estimate(plane, plane, options(8), field=field), ValueError, "field must be"),
        (lambda: ops.motion_estimate(plane, plane, cost=torch.zeros((2, 2, 5), device=DEV)), ValueError, "expected torch.int32"),
        (lambda: ops.motion_estimate(plane.cpu(), plane), RuntimeError, "tensor must live on the GPU"),
        (lambda: ops.motion_warp(plane, field, 12), ValueError, "block must be one of"),
        (lambda: ops.motion_warp(plane, field, 8), ValueError, "field must be"),
        (lambda: ops.motion_warp(plane, field.view(U8), 16), ValueError, "expected torch.int8"),
        (lambda: ops.motion_warp(plane, field, 16, out=plane), ValueError, "must not overlap"),
        (lambda: ops.motion_warp(plane, field.cpu(), 16), RuntimeError, "tensor must live on the GPU"),
    ]
    import test_gpu_mask_crf as T
    with T.recording() as rec:       # ``ops.lib()`` replaced: launches are counted and forwarded
        for call, kind, text in faults:
            with pytest.raises(kind, match=text):
                call()
    assert rec.launches == []


def test_the_c_entries_refuse_their_faults():
    import fosvos_hip
    from fosvos_hip import ops
    L = fosvos_hip.lib()
    stream = torch.cuda.current_stream(0).cuda_stream
    plane = torch.zeros((1, 19, 70), dtype=U8, device=DEV)
    other = torch.zeros((1, 19, 70), dtype=U8, device=DEV)
    field = torch.zeros((1, 2, 5, 2), dtype=I8, device=DEV)
    cost = torch.zeros((1, 2, 5), dtype=I32, device=DEV)
    image = torch.zeros((1, 3, 19, 70), device=DEV)
    p, o, f, c, im = (t.data_ptr() for t in (plane, other, field, cost, image))
    cases = [(lambda: L.fosvos_motion_estimate(p, o, 1, 19, 70, 12, 8, 8, f, c, 0, stream), "block 12"),
             (lambda: L.fosvos_motion_estimate(p, o, 1, 19, 70, 16, 17, 8, f, c, 0, stream), "search 17"),
             (lambda: L.fosvos_motion_estimate(p, o, 1, 19, 70, 16, 0, 8, f, c, 0, stream), "search 0"),
             (lambda: L.fosvos_motion_estimate(p, o, 1, 19, 70, 16, 8, 256, f, c, 0, stream), "zero_bias 256"),
             (lambda: L.fosvos_motion_estimate(p, o, 1, 19, 70, 16, 8, 8, f, c + 1, 0, stream), "4-byte aligned"),
             (lambda: L.fosvos_motion_estimate(p, None, 1, 19, 70, 16, 8, 8, f, c, 0, stream), "null pointer"),
             (lambda: L.fosvos_motion_estimate(p, o, 1, 19, 8193, 16, 8, 8, f, c, 0, stream), "sides of 1..8192"),
             (lambda: L.fosvos_motion_warp(p, f, 1, 19, 70, 16, p, 0, stream), "must not overlap"),
             (lambda: L.fosvos_motion_warp(p, f, 1, 19, 70, 16, p + 19 * 70 - 1, 0, stream), "must not overlap"),
             (lambda: L.fosvos_motion_warp(p, f, 1, 19, 70, 4, o, 0, stream), "block 4"),
             (lambda: L.fosvos_motion_warp(p, f, 0, 19, 70, 16, o, 0, stream), "N=0"),
             (lambda: L.fosvos_motion_luma(im + 2, ops._mean_bgr(), 1, 19, 70, o, 0, stream), "4-byte aligned"),
             (lambda: L.fosvos_motion_luma(im, None, 1, 19, 70, o, 0, stream), "null pointer")]
    for call, text in cases:
        assert call() != 0 and text in L.fosvos_last_error().decode(), text


# ------------------------------------------------------------------------------------------ the test pass on the real net
SIZE = PC.SIZE


class GateByDefinition:
    """A net whose ``forward`` applies ``block_motion.gate_sequence`` behind ``net``, one call after the other: the chain's
    state (the last luma plane and kept mask) is carried from call to call on the host.  A pass WITHOUT ``clean`` and
    ``motion`` over this net is what a pass with them must equal."""

    def __init__(self, net, seed, clean, motion):
        self.net, self.seed, self.clean, self.motion = net, seed, clean, motion
        self.before, self.kept = (None, None), []

    def forward(self, x):
        out = self.net.forward(x)[-1].detach().float().cpu().contiguous().numpy()
        images = x.detach().float().cpu().contiguous().numpy()
        cleaned, kept = B.gate_sequence(images, out[:, 0], self.seed if self.before[0] is None else None, self.clean, self.motion,
                                        *self.before)
        self.before = (B.luma(images[-1]), kept[-1])
        self.kept += list(kept.astype(np.uint8))
        return [torch.from_numpy(cleaned[:, None]).to(DEV)]


@contextlib.contextmanager
def kept_masks(monkeypatch):
    """Every ``kept`` mask ``ops.clean_components`` writes, in call order (read back after the call: the pass's own waits are
    not what this test is about)."""
    from fosvos_hip import ops
    masks, original = [], ops.clean_components

    def clean_components(*args, **kwargs):
        out = original(*args, **kwargs)
        masks.extend(kwargs["kept"].cpu().numpy())
        return out
    with monkeypatch.context() as m:
        m.setattr(ops, "clean_components", clean_components)
        yield masks


@pytest.mark.parametrize("extra", ["alone", "crf_ensemble"])
def test_fast_with_motion_writes_the_definitions_files(extra, tmp_path, monkeypatch):
    """7 frames of 48x80 in groups of 3, 3 and 1, two frames a forward call - which keeps each frame's arithmetic, so the
    comparison with the host chain of the same logits is byte for byte."""
    from fosvos_hip.options import CleanOptions, CrfOptions, EnsembleOptions
    clean, motion = CleanOptions(temporal_radius=2, min_area=2), options(8, 7, 8)
    kw, net_of = {}, lambda net: net
    if extra == "crf_ensemble":
        crf, ens = CrfOptions(iterations=2, radius=3), EnsembleOptions(flip=True)
        kw = {"crf": crf, "ensemble": ens}
        net_of = lambda net: CC.CrfByDefinition(EC.EnsembleByDefinition(net, ens.views(), device=DEV), crf, device=DEV)  # noqa: E731
    prov = PC.Provider(PC.Recorder())
    loader = PC.blob_loader(7)
    seed = loader.dataset.annotation("blob", "00000")
    with kept_masks(monkeypatch) as kept:
        score = experiment_helper.test_fast(prov, loader, tmp_path / "motion", loader.dataset.annotation, group=3, forward_batch=2,
                                            seq_name="blob", clean=clean, clean_seed=seed, motion=motion, **kw)
    assert score["motion"] == motion.as_dict() == experiment_helper.last_fast["motion"] and score["clean"] == clean.as_dict()
    assert experiment_helper.last_fast["group_sizes"] == [3, 3, 1]
    by_definition = GateByDefinition(net_of(prov.network), (np.asarray(seed) != 0).astype(np.uint8), clean, motion)
    loader = PC.blob_loader(7)
    want = experiment_helper.test_fast(CC.Provider(by_definition), loader, tmp_path / "definition", loader.dataset.annotation, group=3,
                                       forward_batch=2, seq_name="blob")
    files = CC.files_of(tmp_path / "motion")
    assert sorted(files) == ["blob/%05d.png" % k for k in range(7)]
    assert files == CC.files_of(tmp_path / "definition")
    assert len(kept) == 7 == len(by_definition.kept) and all(np.array_equal(a, b) for a, b in zip(kept, by_definition.kept))
    for key in ("counts", "J", "F", "J_stats", "F_stats", "J&F", "fnames", "scored"):
        assert score[key] == want[key], key
    assert "motion" not in want


class Recorder(PC.Recorder):
    """The recorder of tests/test_gpu_test_pass_calls.py with the motion ops logged as well."""

    @contextlib.contextmanager
    def active(self, monkeypatch):
        from fosvos_hip import ops
        with super().active(monkeypatch):
            with monkeypatch.context() as m:
                for name in ("motion_luma", "motion_estimate", "motion_warp"):
                    m.setattr(ops, name, self._op(name, getattr(ops, name)))
                yield self


def test_fast_call_order(tmp_path, monkeypatch):
    """5 frames in groups of 3 and 2: per group ONE luma and ONE estimate, per frame a warp (not for the very first) and a
    clean call, then the sequence as without motion - and no host wait beyond that one's.  Without ``motion`` the calls are
    the ones tests/test_gpu_test_pass_calls.py pins."""
    from fosvos_hip.options import CleanOptions
    clean = CleanOptions(temporal_radius=1)
    rec = Recorder()
    prov = PC.Provider(rec)
    loader = PC.blob_loader(5)
    seed = loader.dataset.annotation("blob", "00000")
    with rec.active(monkeypatch):
        experiment_helper.test_fast(prov, loader, tmp_path / "a", loader.dataset.annotation, group=3, seq_name="blob", clean=clean,
                                    clean_seed=seed, motion=options())
    frame = [("motion_warp", ("out",)), ("clean_components", ("out", "kept"))]
    expected = []
    for g, n in enumerate([3, 2]):
        expected += [("forward", min(2, n - k)) for k in range(0, n, 2)]      # two frames a forward call
        expected += [("motion_luma", ("out",)), ("motion_estimate", ())]
        expected += (frame[1:] if g == 0 else frame) + (n - 1) * frame
        expected += [("jf_counts", ("out",)), ("prob_bytes", ()), ("png_encode", ("out", "lengths"))]
        expected += [PC.EVENT_WAIT] if g > 0 else []
    expected += [PC.EVENT_WAIT, PC.READ_BACK]
    assert rec.log == expected
    for kw in ({}, {"motion": None}):
        rec = Recorder()
        prov = PC.Provider(rec)
        loader = PC.blob_loader(5)
        with rec.active(monkeypatch):
            score = experiment_helper.test_fast(prov, loader, tmp_path / "b", loader.dataset.annotation, group=2, seq_name="blob",
                                                clean=clean, clean_seed=seed, **kw)
        assert rec.log == PC.fast_expected([2, 2, 1], True, ("out", "kept"))
        assert "motion" not in score and "motion" not in experiment_helper.last_fast


# ------------------------------------------------------------------------------------------ FrameSegmenter(clean=, motion=)
class PlantedNet(torch.nn.Module):
    """A net whose answer to its k-th call is the k-th planted map, whatever it is shown."""

    def __init__(self, maps):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.maps = torch.from_numpy(np.array(maps, order="C"))[:, None]       # a copy: the shared maps are read-only
        self.at = 0

    def forward(self, x):
        out = self.maps[self.at:self.at + 1].clone().to(self.anchor.device)
        self.at += 1
        return [out]


@pytest.mark.parametrize("scaled", [False, True], ids=["frame_size", "net_size"])
def test_segmenter_with_motion_is_the_definitions_track(scaled):
    """Six frames of the pan, a hand-set seed before the first and before the fourth, at depth 1 and 2: the mask bytes are
    those of ``block_motion.track`` on the images the net saw and the maps it answered."""
    from fosvos_hip.options import CleanOptions
    from fosvos_hip.stream import FrameSegmenter
    scale = 2 if scaled else 1
    frames, logits, disks, blob = C.pan(6, scale)
    hn, wn = logits.shape[1:]
    hf, wf = scale * hn, scale * wn
    size = dict(net_size=(hn, wn)) if scaled else {}
    clean, motion = CleanOptions(temporal_radius=2), options(16, 16, 8)
    seen = [R.prepare_frame_scaled(f, hn, wn)[0] if scaled else F.prepare_frame(f)[0] for f in frames]
    reseed = {3: disks[3]}
    want, kept = B.track(list(zip(seen, logits)), disks[0], clean, motion, reseed=reseed)
    assert [C.iou(kept[t], disks[t]) for t in range(6)] == [1.0] * 6 and not any(kept[t][blob].any() for t in range(1, 6))
    plain, _ = C.chain_without_motion(logits, disks[0], 2)
    assert not np.array_equal(plain, want)

    def paint(frame, x):
        return R.apply_scaled(frame, x, False, False, True, "r", 1.0) if scaled else F.apply(frame, x, False, False, True, "r", 1.0)

    def run(depth, motion):
        outs = []
        with FrameSegmenter(PlantedNet(logits).to(DEV), hf, wf, depth=depth, mirror=False, overlay=False, clean=clean, motion=motion,
                            **size) as seg:
            seg.seed(disks[0].astype(np.uint8))
            for k, frame in enumerate(frames):
                if k in reseed:
                    seg.seed(reseed[k].astype(np.uint8))
                if len(seg._flight) == depth:
                    outs.append(seg.result())
                seg.submit(frame)
            while seg.pending:
                outs.append(seg.result())
        return outs

    for depth in (1, 2):
        got = run(depth, motion)
        for k, frame in enumerate(frames):
            assert np.array_equal(got[k], paint(frame, want[k])), (depth, k)
    # without motion: the chain as it was, whose third frame has lost the object
    got = run(2, None)
    cleaned = np.concatenate([C.chain_without_motion(logits[:3], disks[0], 2)[0], C.chain_without_motion(logits[3:], disks[3], 2)[0]])
    for k, frame in enumerate(frames):
        assert np.array_equal(got[k], paint(frame, cleaned[k])), k
