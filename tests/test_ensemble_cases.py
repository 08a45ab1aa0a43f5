"""The cases the test-time ensemble's CPU and GPU tests share (tests/test_test_ensemble_cpu.py, tests/test_gpu_test_ensemble.py):
shapes, view sets, seeded operands, the comparison of bits and the stand-in nets.  A plain module of data and helpers: it
holds no test of its own.

Comparing bits.  ``same_bits`` asks for equal bit patterns wherever the expected value is no NaN, and for a NaN wherever it
is one.  IEEE 754 leaves the sign and the payload of a NaN that an operation GENERATES (inf x 0, inf - inf) to the
implementation: x86 makes 0xFFC00000 of it, gfx950 0x7FC00000, so a generated NaN of the numpy definition and of the kernel
are both NaN and differ in the sign bit.  Every other value - infinities and signed zeros included - must agree to the last
bit."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from util import test_ensemble as TE  # noqa: E402

F, T = False, True
SHAPES = [(1, 1), (2, 5), (5, 7), (13, 37), (33, 67), (48, 80)]
SCALES = [0.25, 0.5, 0.75, 1.25, 2.0, 4.0]
VIEW_SIZES = [((480, 854), 0.5, (240, 427)), ((480, 854), 0.75, (360, 641)), ((480, 854), 1.25, (600, 1068)),
              ((2, 5), 0.5, (1, 3)), ((5, 7), 0.75, (4, 5)), ((5, 7), 1.25, (6, 9)), ((1, 1), 0.25, (1, 1))]
EIGHT = [(1.0, F), (1.0, T), (0.75, F), (0.75, T), (1.25, F), (1.25, T), (0.5, F), (2.0, T)]
VIEW_SETS = {"flip": TE.views(True, (1.0,)), "scales": TE.views(True, (0.75, 1.25)), "eight": EIGHT}
GPU_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 13, 37), (3, 33, 67), (1, 48, 80)]


def image(n, h, w, seed=0, channels=3):
    """float32 [n,channels,h,w]: seeded, mean-free, of a frame's magnitude."""
    return (np.random.default_rng(seed).standard_normal((n, channels, h, w)) * 60.0).astype(np.float32)


def logit_maps(n, h, w, views, seed=0):
    """One float32 [n,1,hs,ws] per view."""
    rng = np.random.default_rng(seed + 1000)
    return [(rng.standard_normal((n, 1) + TE.view_sizes(h, w, s)) * 4.0).astype(np.float32) for s, _ in views]


def with_specials(maps, seed=0):
    """Copies of the maps with a positive quiet NaN, +inf, -inf and -0.0 written into seeded places of every map."""
    rng = np.random.default_rng(seed + 2000)
    out = []
    for a in maps:
        a = a.copy()
        flat = a.reshape(-1)
        for value in (np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-0.0)):
            flat[int(rng.integers(0, flat.size))] = value
        out.append(a)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """None, or one line that says how the two float32 arrays differ (see the module's docstring for the rule on NaNs)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return "shapes / dtypes differ: %s %s and %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    if not bad.any():
        return None
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    return "%d of %d values differ; first at %s: got %r (bits %#x), expected %r (bits %#x)" % (
        int(bad.sum()), bad.size, at, float(got[at]), int(bits(got)[at]), float(want[at]), int(bits(want)[at]))


def nan_bits_that_differ(got, want):
    """How many NaNs of the two arrays differ in their bits (a figure the GPU tests print; ``same_bits`` does not ask)."""
    nan = np.isnan(want) & np.isnan(got)
    return int((bits(got)[nan] != bits(want)[nan]).sum())


def ramp(h, w):
    """``x + 3 y`` as float32 [1,3,h,w] (every channel the same)."""
    a = (np.arange(w, dtype=np.float32)[None, :] + 3.0 * np.arange(h, dtype=np.float32)[:, None]).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(a, (1, 3, h, w)))


# ------------------------------------------------------------------------------------------ stand-in nets
class Provider:
    def __init__(self, network):
        self.network = network


class StubNet:
    """A CPU stand-in that records its calls: channel ``channel`` of its input, each frame centred on its median and scaled
    (about half of the pixels are object).  Every frame is computed alone, whatever batch it comes in."""

    def __init__(self, channel=0, scale=0.125):
        self.channel, self.scale, self.calls = channel, scale, []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        x = x.cpu()
        c = x[:, self.channel:self.channel + 1]
        return [((c - c.flatten(1).median(dim=1).values.view(-1, 1, 1, 1)) * self.scale).contiguous()]


class EnsembleByDefinition:
    """A net whose ``forward`` applies the numpy definition around ``net``: the views are made with
    ``test_ensemble.make_views`` on the host, each is forwarded through ``net`` on ``device`` (None: the host) and the answers
    are merged with ``test_ensemble.merge``.  A pass WITHOUT ``ensemble`` over this net is what a pass with it must equal."""

    def __init__(self, net, views, device=None):
        self.net, self.views, self.device = net, list(views), device

    def forward(self, x):
        h, w = int(x.shape[2]), int(x.shape[3])
        maps = []
        for view in TE.make_views(x.detach().cpu().numpy(), self.views):
            t = torch.from_numpy(view)
            out = self.net.forward(t if self.device is None else t.to(self.device))[-1]
            maps.append(out.detach().float().cpu().contiguous().numpy())
        merged = torch.from_numpy(TE.merge(maps, self.views, h, w))
        return [merged if self.device is None else merged.to(self.device)]


def files_of(root):
    """name -> bytes of every file below ``root``."""
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}
