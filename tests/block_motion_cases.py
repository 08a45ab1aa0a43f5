"""Shapes, contents and the definition's answers for the block-matching tests (tests/test_block_motion_cpu.py and
tests/test_gpu_block_motion.py), each reference computed once and handed out read-only.  A plain module: nothing here is a
fixture or a pytest setting.  Every comparison made with these is exact equality."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders.davis_2016 import MEANVAL  # noqa: E402
from util import block_motion as B, mask_components  # noqa: E402

# csrc/motion.hip: a workgroup of k_motion_estimate owns a tile of TILE rows x columns; the tile is a multiple of both blocks
TILE = (16, 64)
# two whole tiles and a ragged third in both axes; ragged for blocks of 8 and of 16 as well (43 = 5 * 8 + 3, 165 = 20 * 8 + 5)
TWO_TILES = (2 * TILE[0] + 11, 2 * TILE[1] + 37)
SHAPES = [(5, 7),        # smaller than a block
          (19, 70),      # with search 16 the window is taller than the frame
          (37, 150),
          TWO_TILES]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
BATCHES = (1, 3)
BLOCKS = (8, 16)
SEARCHES = (1, 7, 16)
SHIFT = (5, 14)
# content -> zero_bias.  The tie cases run without a bias so that the order (dy^2 + dx^2, dy, dx) alone decides
CONTENTS = {"random": 8,        # unique minima
            "planted": 8,       # the shift is recovered
            "flat": 0,          # all ties
            "stripes": 0,       # directed ties
            "checker": 8,       # 0 / 255 checkerboard against its inverse: SAD 0 at odd steps, the maximum at even ones
            "opposite": 255}    # all 0 against all 255 with the largest bias: the largest score there is, in every candidate


def planes(content, n, h, w, seed=0):
    """(prev, cur) uint8 [n,h,w] of a content."""
    rng = np.random.default_rng([seed, n, h, w, sorted(CONTENTS).index(content)])
    yy, xx = np.mgrid[:h, :w]
    if content == "random":
        prev, cur = rng.integers(0, 256, (2, n, h, w), dtype=np.uint8)
    elif content == "planted":
        prev, cur = planted(n, h, w, SHIFT, rng)
    elif content == "flat":
        prev = cur = np.broadcast_to(rng.integers(0, 256, (n, 1, 1), dtype=np.uint8), (n, h, w))
    elif content == "stripes":
        # vertical stripes of period 4, the current frame one column on: dx = 1, -3, 5, ... match exactly, at every dy
        prev = np.broadcast_to((((xx % 4) < 2) * 200 + 20).astype(np.uint8), (n, h, w))
        cur = np.broadcast_to(((((xx + 1) % 4) < 2) * 200 + 20).astype(np.uint8), (n, h, w))
    elif content == "checker":
        prev = np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8), (n, h, w))
        cur = 255 - prev
    else:
        assert content == "opposite"
        prev, cur = np.zeros((n, h, w), np.uint8), np.full((n, h, w), 255, np.uint8)
    return np.ascontiguousarray(prev), np.ascontiguousarray(cur)


def planted(n, h, w, shift, rng):
    """Random bytes with ``cur[p] = prev[p + shift]`` wherever ``p + shift`` lies in the frame."""
    dy, dx = shift
    big = rng.integers(0, 256, (n, h + 2 * abs(dy), w + 2 * abs(dx)), dtype=np.uint8)
    prev = big[:, abs(dy):abs(dy) + h, abs(dx):abs(dx) + w]
    cur = big[:, abs(dy) + dy:abs(dy) + dy + h, abs(dx) + dx:abs(dx) + dx + w]
    return prev, cur


def inside_blocks(h, w, block, shift):
    """bool [Hb,Wb]: the blocks whose square, moved by ``shift``, lies wholly in the frame."""
    hb, wb = B.grid(h, w, block)
    ys, xs = np.arange(hb) * block, np.arange(wb) * block
    ye, xe = np.minimum(ys + block, h), np.minimum(xs + block, w)
    ok_y = (ys + shift[0] >= 0) & (ye + shift[0] <= h)
    ok_x = (xs + shift[1] >= 0) & (xe + shift[1] <= w)
    return ok_y[:, None] & ok_x[None, :]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(content, n, shape, block, search):
    """(prev, cur, field, cost) of a case: the vectorised definition's answer, read-only."""
    prev, cur = planes(content, n, shape[0], shape[1])
    field, cost = B.estimate(prev, cur, block, search, CONTENTS[content])
    return frozen(prev, cur, field, cost)


def prepared(frames):
    """uint8 [N,H,W,3] BGR frames -> the net's input float32 [N,3,H,W]."""
    mean = np.array(MEANVAL, dtype=np.float32)
    return np.ascontiguousarray(frames.astype(np.float32).transpose(0, 3, 1, 2) - mean[None, :, None, None])


def random_field(n, h, w, block, seed=0):
    """int8 [n,Hb,Wb,2] of every magnitude, the extremes planted."""
    rng = np.random.default_rng([seed, n, h, w, block])
    hb, wb = B.grid(h, w, block)
    field = rng.integers(-128, 128, (n, hb, wb, 2)).astype(np.int8)
    small = rng.random((n, hb, wb)) < 0.6          # most vectors land in the frame
    field[small] = rng.integers(-4, 5, (int(small.sum()), 2)).astype(np.int8)
    flat = field.reshape(-1, 2)
    for k, v in enumerate(((127, 127), (-128, -128), (127, -128), (-128, 127), (0, 0))[:len(flat)]):
        flat[k] = v
    return field


# ------------------------------------------------------------------------------------------ the prototype case
class Clean:
    """What ``gate_sequence`` reads of a CleanOptions."""
    min_area, largest, fill = 0, False, -100.0

    def __init__(self, temporal_radius):
        self.temporal_radius = temporal_radius


@functools.lru_cache(maxsize=None)
def pan(t_n, scale=1):
    """A pan over random bytes: (frames uint8 [t_n, 97 scale, 161 scale, 3], logits float32 [t_n,97,161], disks bool
    [t_n,97,161], blob slice).  On the 97 x 161 map the scene pans by SHIFT a frame (``scale`` times that in the frames, whose
    ``scale x scale`` averages are the map's pixels); a disk of radius 6 is fixed in the scene, from (60, 110); a 5 x 6 blob is
    fixed in the map; the logits are +1 on both and -1 elsewhere."""
    h, w = 97, 161
    rng = np.random.default_rng(2016 + scale)
    big = rng.integers(0, 256, (scale * (h + SHIFT[0] * t_n), scale * (w + SHIFT[1] * t_n)), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    blob = (slice(10, 15), slice(10, 16))
    frames, logits, disks = [], [], []
    for t in range(t_n):
        y0, x0 = scale * SHIFT[0] * t, scale * SHIFT[1] * t                          # frame t [p] = frame t-1 [p + shift]
        frames.append(np.repeat(big[y0:y0 + scale * h, x0:x0 + scale * w, None], 3, axis=2))
        disk = (yy - (60 - SHIFT[0] * t)) ** 2 + (xx - (110 - SHIFT[1] * t)) ** 2 <= 36
        mask = disk.copy()
        mask[blob] = True
        disks.append(disk)
        logits.append(np.where(mask, 1.0, -1.0).astype(np.float32))
    return frozen(np.stack(frames), np.stack(logits), np.stack(disks)) + (blob,)


def prototype():
    """The pan of five frames as (images float32 [5,3,97,161] - the net's input -, logits, disks, blob slice)."""
    frames, logits, disks, blob = pan(5)
    return frozen(prepared(frames))[0], logits, disks, blob


def iou(a, b):
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    return float((a & b).sum()) / float(max(1, (a | b).sum()))


def chain_without_motion(logits, seed, radius):
    return mask_components.clean_sequence(logits, seed, radius=radius, chain=True)
