"""The block-matching definition (util/block_motion.py) on the host: the vectorised form against the per-block loop, the
properties the issue names - a planted shift is recovered, the tie order, the zero bias, ragged frames, the warp's border rule,
the prototype pan -, MotionOptions, every refusal of the Python faces, and the order of the device calls of a test-pass group
and of a stream frame under a recording stand-in for ``ops`` that computes by the definitions.  No GPU; every comparison is
exact equality."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_motion_cases as C  # noqa: E402
from util import args_helper, block_motion as B, experiment_helper, mask_components, mask_crf  # noqa: E402

NO_CPU = "tensor must live on the GPU (the HIP path has no CPU fallback)"


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ luma
def test_luma_is_the_weighted_sum_of_the_frames_bytes():
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)
    frames[0, 0, 0], frames[0, 0, 1], frames[0, 0, 2] = (255, 255, 255), (0, 0, 0), (255, 0, 0)
    y = B.luma(C.prepared(frames))
    f = frames.astype(np.int64)
    assert y.dtype == np.uint8 and y.shape == (2, 9, 13)
    assert np.array_equal(y, (29 * f[..., 0] + 150 * f[..., 1] + 77 * f[..., 2] + 128) >> 8)
    assert (y[0, 0, 0], y[0, 0, 1], y[0, 0, 2]) == (255, 0, (29 * 255 + 128) >> 8)
    assert np.array_equal(B.luma(C.prepared(frames)[1]), y[1])
    image = C.prepared(frames)[0]
    image[:, 1, 1] = np.nan
    image[:, 1, 2] = (np.inf, -np.inf, 1e30)
    g = mask_crf.guide_levels(image)
    assert B.luma(image)[1, 1] == 0 and B.luma(image)[1, 2] == (29 * 255 + 77 * 255 + 128) >> 8 and tuple(g[:, 1, 2]) == (255, 0, 255)
    with pytest.raises(ValueError):
        B.luma(np.zeros((3, 4, 5), np.float64))


# ------------------------------------------------------------------------------------------ the two forms of the definition
LOOP_CASES = [("random", 1, (5, 7), 16, 16), ("random", 1, (5, 7), 8, 1), ("random", 2, (19, 70), 16, 16),
              ("random", 1, (19, 70), 8, 7), ("random", 1, (37, 150), 16, 7), ("random", 1, (37, 150), 8, 16),
              ("planted", 1, (37, 150), 16, 16), ("flat", 1, (37, 150), 8, 7), ("stripes", 1, (37, 150), 16, 7),
              ("checker", 1, (19, 70), 8, 7), ("opposite", 1, (19, 70), 16, 16), ("random", 1, C.TWO_TILES, 16, 7)]


@pytest.mark.parametrize("case", LOOP_CASES, ids=["%s_n%d_%dx%d_b%d_s%d" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4]) for c in LOOP_CASES])
def test_vectorised_is_the_loop(case):
    content, n, shape, block, search = case
    prev, cur, field, cost = C.reference(*case)
    hb, wb = B.grid(shape[0], shape[1], block)
    assert field.shape == (n, hb, wb, 2) and field.dtype == np.int8 and cost.shape == (n, hb, wb) and cost.dtype == np.int32
    assert same(B.estimate_loop(prev, cur, block, search, C.CONTENTS[content]), (field, cost))
    assert same(B.estimate(prev[0], cur[0], block, search, C.CONTENTS[content]), (field[0], cost[0]))     # [H,W] in, no batch axis out


@pytest.mark.parametrize("block", C.BLOCKS)
@pytest.mark.parametrize("shift", [C.SHIFT, (-5, -14), (-3, 16)])
def test_planted_shift_is_recovered(shift, block):
    """Every block whose shifted square lies in the frame answers the shift with cost 0.  The frame's last block is ONE pixel
    (97 = 6 * 16 + 1 = 12 * 8 + 1, 161 = 10 * 16 + 1 = 20 * 8 + 1): among 1089 random bytes one equal to it lies nearer than
    the shift with probability 1 - (255/256)^1088 = 0.99, and the definition's order then prefers it.  So the statement is made
    of the blocks of at least 8 pixels - every other block of this frame -, where such a coincidence has probability
    1089 * 2^-64; a shift down and right moves that corner block out of the frame anyway."""
    h, w = 97, 161
    prev, cur = C.planted(1, h, w, shift, np.random.default_rng(7))
    field, cost = B.estimate(prev[0], cur[0], block, 16, 8)
    inside = C.inside_blocks(h, w, block, shift)
    if shift == C.SHIFT and block == 16:
        assert inside.size == 77 and int(inside.sum()) == 45 and not inside[-1, -1]
    inside[-1, -1] = False
    if shift == C.SHIFT and block == 16:
        assert inside.size == 77 and int(inside.sum()) == 45
    assert inside.any() and not inside.all()
    assert np.array_equal(field[inside], np.broadcast_to(np.array(shift, np.int8), (int(inside.sum()), 2)))
    assert not cost[inside].any()
    if block == 16 and shift == C.SHIFT:
        assert same(B.estimate_loop(prev[0], cur[0], block, 16, 8), (field, cost))


def test_flat_frames_stand_still():
    prev, cur, field, cost = C.reference("flat", 3, (37, 150), 16, 16)
    assert C.CONTENTS["flat"] == 0 and not field.any() and not cost.any()


def test_stripes_take_the_shortest_then_the_smallest_vector():
    """Every dx = 1 mod 4 matches exactly at every dy: the smallest dy^2 + dx^2 is (0, 1); without it, among (0, -3) ... the
    order falls to dy, then dx."""
    prev, cur, field, cost = C.reference("stripes", 1, (37, 150), 16, 7)
    assert np.array_equal(field[0, :, :-1], np.broadcast_to(np.array((0, 1), np.int8), field[0, :, :-1].shape)) and not cost[0, :, :-1].any()
    # the last column of blocks (6 pixels wide at block 16: 150 = 9 * 16 + 6) cannot move right by 1: next is (0, -3)
    assert np.array_equal(field[0, :, -1], np.broadcast_to(np.array((0, -3), np.int8), field[0, :, -1].shape))
    # equal scores everywhere: (0, 0) is the shortest
    wide = np.full((48, 48), 9, np.uint8)
    field, cost = B.estimate(wide, np.full((48, 48), 10, np.uint8), 16, 1, 0)
    assert tuple(field[1, 1]) == (0, 0) and cost[1, 1] == 256
    # equal dy^2 + dx^2: where the previous frame's centre block alone differs, (-16, 0), (0, -16), (0, 16) and (16, 0) all
    # leave it at cost 0 and 256 from the centre: the smallest dy answers
    odd = wide.copy()
    odd[16:32, 16:32] = 200
    field, cost = B.estimate(odd, wide, 16, 16, 0)
    assert tuple(field[1, 1]) == (-16, 0) and cost[1, 1] == 0
    odd[0:16, 16:32] = 200                                        # ... and with the block above spoilt too: the smallest dx
    field, cost = B.estimate(odd, wide, 16, 16, 0)
    assert tuple(field[1, 1]) == (0, -16) and cost[1, 1] == 0


def test_zero_bias_decides_small_gains():
    """Block 16, zero_bias 8: a non-zero vector pays (8 * 256) >> 4 = 128.  A candidate that beats (0, 0) by 127 loses, one
    that beats it by 129 wins; at exactly 128 the scores tie and (0, 0) is the shorter."""
    for gain, wins in ((127, False), (128, False), (129, True)):
        # the frame is one block high: block (0, 1) (columns 16..31) can only go to (0, -1), (0, 0) or (0, 1)
        prev = np.zeros((16, 48), np.uint8)
        cur = np.zeros((16, 48), np.uint8)
        cur[0, 20] = 200
        prev[0, 21] = 200                            # (0, 1) matches it; (0, 0) and (0, -1) see both pixels apart: SAD 400
        prev[5, 32], prev[6, 32] = 200, 200 - gain   # column 32 is seen from (0, 1) alone: its SAD is 400 - gain
        field, cost = B.estimate(prev, cur, 16, 1, 8)
        assert (tuple(field[0, 1]) == (0, 1)) == wins, gain
        assert cost[0, 1] == (400 - gain if wins else 400)
        assert same(B.estimate_loop(prev, cur, 16, 1, 8), (field, cost))
        free, _ = B.estimate(prev, cur, 16, 1, 0)
        assert tuple(free[0, 1]) == (0, 1)


@pytest.mark.parametrize("shape", C.SHAPES[:3], ids=C.SHAPE_IDS[:3])
def test_ragged_frames(shape):
    h, w = shape
    for block in C.BLOCKS:
        prev, cur, field, cost = C.reference("random", 1, shape, block, 16)
        hb, wb = B.grid(h, w, block)
        assert field.shape == (1, hb, wb, 2)
        ys, xs = np.arange(hb)[:, None] * block, np.arange(wb)[None, :] * block
        ye, xe = np.minimum(ys + block, h), np.minimum(xs + block, w)
        dy, dx = field[0, ..., 0].astype(int), field[0, ..., 1].astype(int)
        assert (ys + dy >= 0).all() and (ye + dy <= h).all() and (xs + dx >= 0).all() and (xe + dx <= w).all()   # never clamped
    if shape == (5, 7):
        assert not field.any()              # one block that fills the frame cannot move


# ------------------------------------------------------------------------------------------ warp
def test_warp_by_zero_is_the_mask_as_a_bit():
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 4, (37, 150), dtype=np.uint8) * 85
    for block in C.BLOCKS:
        out = B.warp(mask, np.zeros(B.grid(37, 150, block) + (2,), np.int8), block)
        assert out.dtype == np.uint8 and np.array_equal(out, (mask != 0).astype(np.uint8))
    assert np.array_equal(B.warp(mask != 0, np.zeros((3, 10, 2), np.int8), 16), (mask != 0).astype(np.uint8))


def test_warp_reads_nothing_outside_the_frame():
    mask = np.ones((19, 70), np.uint8)
    for v in (127, -128, -127):
        for pair in ((v, 0), (0, v), (v, v), (v, -v if v != -128 else 127)):
            field = np.empty((2, 5, 2), np.int8)
            field[...] = pair
            assert not B.warp(mask, field, 16).any()
    field = np.zeros((2, 5, 2), np.int8)
    field[0, 0] = (3, -2)                   # rows 0..15 of block column 0 read (y + 3, x - 2): columns 0, 1 fall outside
    out = B.warp(mask, field, 16)
    assert not out[:16, :2].any() and out[:16, 2:16].all() and out[16:].all()
    one = C.random_field(1, 37, 150, 8)[0]
    rng = np.random.default_rng(5)
    m = rng.integers(0, 2, (37, 150), dtype=np.uint8)
    want = np.zeros_like(m)
    for y in range(37):
        for x in range(150):
            sy, sx = y + int(one[y // 8, x // 8, 0]), x + int(one[y // 8, x // 8, 1])
            want[y, x] = m[sy, sx] != 0 if 0 <= sy < 37 and 0 <= sx < 150 else 0
    assert np.array_equal(B.warp(m, one, 8), want)
    for bad in (lambda: B.warp(m, one, 16), lambda: B.warp(m, one.astype(np.int16), 8), lambda: B.warp(m, one, 4),
                lambda: B.warp(m.astype(np.float32), one, 8)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ the prototype case
def test_the_pan_loses_the_object_without_motion_and_keeps_it_with():
    from fosvos_hip.options import MotionOptions
    images, logits, disks, blob = C.prototype()
    _, plain = C.chain_without_motion(logits, disks[0], 2)
    ious = [C.iou(plain[t], disks[t]) for t in range(5)]
    assert ious[0] == 1.0 and 0.0 in ious
    assert [round(v, 2) for v in ious] == [1.0, 0.0, 0.79, 0.0, 0.0]
    motion = MotionOptions(block=16, search=16, zero_bias=8)
    cleaned, kept = B.gate_sequence(images, logits, disks[0], C.Clean(2), motion)
    assert [C.iou(kept[t], disks[t]) for t in range(5)] == [1.0] * 5
    assert not any(kept[t][blob].any() for t in range(1, 5))
    assert np.array_equal(cleaned, np.where(kept, logits, np.where(logits >= 0, np.float32(-100.0), logits)))
    # across groups: the same chain in pieces of 2, 2 and 1 frames
    pieces, before = [], (None, None)
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        _, k = B.gate_sequence(images[lo:hi], logits[lo:hi], disks[0] if lo == 0 else None, C.Clean(2), motion, *before)
        before = (B.luma(images[hi - 1]), k[-1])
        pieces.append(k)
    assert np.array_equal(np.concatenate(pieces), kept)
    # ... and frame by frame: the stream's definition
    _, tracked = B.track(list(zip(images, logits)), disks[0], C.Clean(2), motion)
    assert np.array_equal(tracked, kept)
    # a hand-set seed is used unwarped, and the motion starts again there
    _, again = B.track(list(zip(images, logits)), None, C.Clean(2), motion, reseed={2: disks[2]})
    assert again[0].sum() == (logits[0] >= 0).sum() and np.array_equal(again[2:], kept[2:])


def test_gate_sequence_refusals():
    images, logits, disks, _ = C.prototype()
    for bad in (lambda: B.gate_sequence(images, logits, None, C.Clean(None)),
                lambda: B.gate_sequence(images[:2], logits, None, C.Clean(2)),
                lambda: B.gate_sequence(images, logits, None, C.Clean(2), None, B.luma(images[0]), None),
                lambda: B.gate_sequence(images, logits, disks[0], C.Clean(2), None, B.luma(images[0]), disks[0]),
                lambda: B.gate_sequence(images, logits.astype(np.float64), None, C.Clean(2))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ options and limits
def test_motion_options():
    from fosvos_hip import limits
    from fosvos_hip.options import MotionOptions
    o = MotionOptions()
    assert (o.block, o.search, o.zero_bias) == (16, 8, 8) == tuple(B.Params()) and o.as_dict() == {"block": 16, "search": 8, "zero_bias": 8}
    assert B.check_options(o) == B.Params() and B.check_options(MotionOptions(8, 16, 255)) == B.Params(8, 16, 255)
    assert (limits.MOTION_BLOCKS, limits.MOTION_MAX_SEARCH, limits.MOTION_MAX_ZERO_BIAS) == (B.BLOCKS, B.MAX_SEARCH, B.MAX_ZERO_BIAS)
    with pytest.raises(Exception):
        o.block = 8                          # frozen
    for kw in ({"block": 12}, {"block": 4}, {"block": True}, {"block": 16.0}, {"search": 0}, {"search": 17}, {"search": 2.0},
               {"zero_bias": -1}, {"zero_bias": 256}, {"zero_bias": None}):
        with pytest.raises(ValueError, match="MotionOptions: " + next(iter(kw))):
            MotionOptions(**kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            B.check_options(types.SimpleNamespace(**{**B.Params()._asdict(), **kw}))
    assert "os.environ" not in inspect.getsource(MotionOptions) and "getenv" not in inspect.getsource(MotionOptions)


# ------------------------------------------------------------------------------------------ refusals of the Python faces
def test_ops_refuse_before_they_launch():
    from fosvos_hip import ops
    from fosvos_hip.options import MotionOptions
    image, plane = torch.zeros((1, 3, 8, 8)), torch.zeros((1, 8, 8), dtype=torch.uint8)
    field = torch.zeros((1, 1, 1, 2), dtype=torch.int8)
    for call in (lambda: ops.motion_luma(image), lambda: ops.motion_estimate(plane, plane), lambda: ops.motion_warp(plane, field, 16)):
        with pytest.raises(RuntimeError) as err:
            call()
        assert NO_CPU in str(err.value)
    with pytest.raises(ValueError, match="MotionOptions"):
        ops.motion_estimate(plane, plane, options=B.Params())
    assert ops.MOTION_BLOCKS == B.BLOCKS and ops.MOTION_MAX_SEARCH == B.MAX_SEARCH
    assert MotionOptions().as_dict() == B.Params()._asdict()


def test_fast_refuses_motion_without_a_temporal_gate(tmp_path):
    from fosvos_hip.options import CleanOptions, MotionOptions
    for kw, reason in (({"motion": MotionOptions()}, "temporal_radius"),
                       ({"motion": MotionOptions(), "clean": CleanOptions(largest=True)}, "temporal_radius"),
                       ({"motion": B.Params(), "clean": CleanOptions(temporal_radius=2)}, "MotionOptions")):
        with pytest.raises(ValueError, match=reason) as err:
            experiment_helper.test_fast(None, None, tmp_path, **kw)
        assert str(err.value).startswith("test_fast: motion")


def test_segmenters_refuse_motion_with_the_reason():
    from fosvos_hip.options import CleanOptions, MotionOptions
    from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
    for kw, reason in (({"motion": MotionOptions()}, "temporal_radius"),
                       ({"motion": MotionOptions(), "clean": CleanOptions(min_area=3)}, "temporal_radius"),
                       ({"motion": {"block": 16}, "clean": CleanOptions(temporal_radius=2)}, "MotionOptions")):
        with pytest.raises(ValueError, match=reason) as err:
            FrameSegmenter(None, 32, 48, **kw)
        assert str(err.value).startswith("FrameSegmenter: motion")
    with pytest.raises(ValueError, match="ONE object") as err:
        ObjectSegmenter([None], 32, 48, motion=MotionOptions())
    assert str(err.value).startswith("ObjectSegmenter: motion=")


def test_command_lines(capsys):
    import run_webcam
    online = ["--fast-test", "--synthetic"]
    args = args_helper.parse_args(True, online + ["--clean-temporal", "3", "--clean-motion"])
    assert args.motion.as_dict() == {"block": 16, "search": 8, "zero_bias": 8}
    args = args_helper.parse_args(True, online + ["--clean-temporal", "3", "--clean-motion", "--motion-block", "8", "--motion-search", "16",
                                                  "--motion-zero-bias", "0", "--crf", "--ensemble-flip", "--clean-largest"])
    assert args.motion.as_dict() == {"block": 8, "search": 16, "zero_bias": 0} and args.crf_options is not None
    assert args_helper.parse_args(True, online + ["--clean-temporal", "3"]).motion is None
    refused = [(online + ["--clean-temporal", "3", "--motion-block", "8"], "--motion-block set(s) an option of the motion-compensated gate"),
               (online + ["--motion-search", "3", "--motion-zero-bias", "1"], "--motion-search / --motion-zero-bias set(s)"),
               (online + ["--clean-motion"], "--clean-motion carries the seed of the temporal gate"),
               (online + ["--clean-largest", "--clean-motion"], "it needs --clean-temporal R"),
               (online + ["--clean-temporal", "3", "--clean-motion", "--motion-block", "12"], "--motion-*: block must be one of (8, 16)"),
               (online + ["--clean-temporal", "3", "--clean-motion", "--motion-search", "17"], "--motion-*: search must be an integer in 1..16"),
               (["--synthetic", "--clean-temporal", "3", "--clean-motion"], "they need --fast-test"),
               (online + ["--multi-object", "--clean-temporal", "3", "--clean-motion"], "--multi-object is not built")]
    for argv, reason in refused:
        with pytest.raises(SystemExit):
            args_helper.parse_args(True, argv)
        assert reason in capsys.readouterr().err, argv
    for argv, reason in ((["--clean-motion"], "it needs --clean-temporal R"),
                         (["--clean-temporal", "2", "--motion-search", "4"], "it needs --clean-motion"),
                         (["--clean-temporal", "2", "--clean-motion", "--motion-zero-bias", "300"], "zero_bias must be an integer in 0..255")):
        with pytest.raises(SystemExit):
            run_webcam.main(argv)
        assert reason in capsys.readouterr().err, argv
    parsed = run_webcam.build_parser().parse_args(["--clean-temporal", "2", "--clean-motion", "--motion-block", "8"])
    assert args_helper.motion_of(run_webcam.build_parser(), parsed).block == 8


# ------------------------------------------------------------------------------------------ the order of the device calls
class DefinitionOps:
    """A stand-in for ``fosvos_hip.ops`` on CPU tensors: every call is logged as (name, the buffers it was handed) and computed
    by the numpy definitions."""
    BUFFERS = ("out", "field", "cost", "kept")

    def __init__(self):
        self.log = []

    def _add(self, name, **buffers):
        self.log.append((name, tuple(b for b in self.BUFFERS if buffers.get(b) is not None)))

    def motion_luma(self, image, out=None):
        self._add("motion_luma", out=out)
        out.copy_(torch.from_numpy(B.luma(image.numpy())).view(out.shape))
        return out

    def motion_estimate(self, prev_y, cur_y, options=None, field=None, cost=None):
        self._add("motion_estimate", field=field, cost=cost)
        f, c = B.estimate(prev_y.numpy().reshape((-1,) + tuple(prev_y.shape[-2:])), cur_y.numpy().reshape((-1,) + tuple(cur_y.shape[-2:])),
                          options=options)
        field.copy_(torch.from_numpy(f))
        cost.copy_(torch.from_numpy(c))
        return field, cost

    def motion_warp(self, mask, field, block, out=None):
        self._add("motion_warp", out=out)
        assert out.data_ptr() != mask.data_ptr()
        out.copy_(torch.from_numpy(np.stack([B.warp(m, f, block) for m, f in zip(mask.numpy(), field.numpy())])))
        return out

    def clean_components(self, logits, seed=None, radius=0, min_area=0, largest=False, chain=False, fill=-100.0, out=None, kept=None):
        self._add("clean_components", out=out, kept=kept)
        assert chain and logits.shape[0] == 1
        x, k = mask_components.clean_sequence(logits[:, 0].numpy().copy(), None if seed is None else seed[0].numpy().copy(), radius,
                                              min_area, largest, chain=True, fill=fill)
        out.copy_(torch.from_numpy(x)[:, None])
        if kept is not None:
            kept.copy_(torch.from_numpy(k.astype(np.uint8)))
        return out

    # the stream's other calls: logged, nothing computed
    def frame_prep(self, frame, mirror, out=None, net_size=None):
        self._add("frame_prep", out=out)

    def overlay(self, frame, logits, *args, out=None, net_size=None):
        self._add("overlay", out=out)


def test_a_groups_calls_and_their_result():
    """Two groups of 3 and 2 frames of the pan through ``_motion_clean``: per group ONE luma and ONE estimate - the second
    group's over the pair across the boundary too -, per frame a warp (not for the sequence's first frame) and a clean call;
    and the chain is ``gate_sequence``'s."""
    from fosvos_hip.options import CleanOptions, MotionOptions
    images, logits, disks, _ = C.prototype()
    clean, motion = CleanOptions(temporal_radius=2), MotionOptions(search=16)
    ops = DefinitionOps()
    buffers = experiment_helper._MotionBuffers(3, 97, 161, motion.block, torch.device("cpu"))
    seed = torch.from_numpy(disks[0].astype(np.uint8))[None].clone()
    got, kept_all = [], []
    for lo, hi, continued in ((0, 3, False), (3, 5, True)):
        x = torch.from_numpy(logits[lo:hi].copy())[:, None]
        kept = torch.zeros((hi - lo, 97, 161), dtype=torch.uint8)
        experiment_helper._motion_clean(ops, torch.from_numpy(images[lo:hi].copy()), x, seed, kept, buffers, continued, clean, motion)
        seed.copy_(kept[hi - lo - 1:hi - lo])
        got.append(x[:, 0].numpy())
        kept_all.append(kept.numpy())
    want, want_kept = B.gate_sequence(images, logits, disks[0], clean, motion)
    assert np.array_equal(np.concatenate(got), want) and np.array_equal(np.concatenate(kept_all), want_kept.astype(np.uint8))
    frame = [("motion_warp", ("out",)), ("clean_components", ("out", "kept"))]
    head = [("motion_luma", ("out",)), ("motion_estimate", ("field", "cost"))]
    assert ops.log == head + frame[1:] + 2 * frame + head + 2 * frame
    # one frame, nothing before it: no pair, no estimate
    ops = DefinitionOps()
    x = torch.from_numpy(logits[:1].copy())[:, None]
    experiment_helper._motion_clean(ops, torch.from_numpy(images[:1].copy()), x, None, torch.zeros((1, 97, 161), dtype=torch.uint8), buffers,
                                    False, clean, motion)
    assert ops.log == [("motion_luma", ("out",)), ("clean_components", ("out", "kept"))]


class Net:
    def __init__(self, answers):
        self.answers = iter(answers)

    def forward(self, image):
        return [torch.from_numpy(next(self.answers).copy())[None, None]]


def stream_frames(motion, monkeypatch):
    """The pan through ``FrameSegmenter._compute`` on a segmenter put together by hand (no stream, no slot buffers but the
    image): (the log, the cleaned logits, the kept masks)."""
    from fosvos_hip import stream
    from fosvos_hip.options import CleanOptions
    images, logits, disks, _ = C.prototype()
    ops = DefinitionOps()
    monkeypatch.setattr(stream, "ops", ops)
    seg = stream.FrameSegmenter.__new__(stream.FrameSegmenter)
    seg.net, seg.clean, seg.motion, seg.mirror, seg.overlay, seg.boolean_mask = Net(logits), CleanOptions(temporal_radius=2), motion, False, True, True
    seg.color, seg.alpha, seg.encode, seg.net_size = "r", 1.0, None, None
    seg._seed = torch.from_numpy(disks[0].astype(np.uint8))[None].clone()
    if motion is not None:
        seg._luma = torch.zeros((2, 1, 97, 161), dtype=torch.uint8)
        seg._field, seg._cost = torch.zeros((1, 7, 11, 2), dtype=torch.int8), torch.zeros((1, 7, 11), dtype=torch.int32)
        seg._warped = torch.zeros((1, 97, 161), dtype=torch.uint8)
    cleaned, kept = [], []
    real = ops.overlay

    def overlay(frame, x, *args, **kwargs):
        cleaned.append(x[0, 0].numpy().copy())
        return real(frame, x, *args, **kwargs)
    ops.overlay = overlay
    for t in range(5):
        seg._compute(types.SimpleNamespace(frame=None, image=torch.from_numpy(images[t:t + 1].copy()), out=torch.zeros(1)))
        kept.append(seg._seed[0].numpy().copy())
    return ops.log, np.stack(cleaned), np.stack(kept)


def test_a_stream_frames_calls_and_their_result(monkeypatch):
    from fosvos_hip.options import MotionOptions
    images, logits, disks, _ = C.prototype()
    motion = MotionOptions(search=16)
    log, cleaned, kept = stream_frames(motion, monkeypatch)
    first = [("frame_prep", ("out",)), ("motion_luma", ("out",)), ("clean_components", ("out", "kept")), ("overlay", ("out",))]
    later = first[:2] + [("motion_estimate", ("field", "cost")), ("motion_warp", ("out",))] + first[2:]
    assert log == first + 4 * later
    want, want_kept = B.track(list(zip(images, logits)), disks[0], C.Clean(2), motion)
    assert np.array_equal(cleaned, want) and np.array_equal(kept, want_kept.astype(np.uint8))


def test_without_motion_the_calls_are_what_they_were(monkeypatch):
    images, logits, disks, _ = C.prototype()
    log, cleaned, kept = stream_frames(None, monkeypatch)
    assert log == 5 * [("frame_prep", ("out",)), ("clean_components", ("out", "kept")), ("overlay", ("out",))]
    want, want_kept = C.chain_without_motion(logits, disks[0], 2)
    assert np.array_equal(cleaned, want) and np.array_equal(kept, want_kept.astype(np.uint8))
    # the test pass: the arguments of the unchanged call carry no motion, and its source asks for no motion op without one
    assert inspect.signature(experiment_helper.test_fast).parameters["motion"].default is None
