"""The cases the CRF's CPU and GPU tests share (tests/test_mask_crf_cpu.py, tests/test_gpu_mask_crf.py): shapes, guides, logits,
the numpy definition's answers computed once, the prototype case and the stand-in nets.  A plain module of data and helpers: it
holds no test of its own."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guided_cases as G  # noqa: E402
from util import mask_crf as M  # noqa: E402

# (N, H, W, r).  The kernel's tile is 16 x 64.
GPU_CASES = [
    (1, 1, 1, 5),      # a 1 x 1 map: no neighbour at all
    (1, 3, 5, 5),      # every window clipped on all sides
    (1, 16, 64, 1),    # exactly one tile
    (1, 17, 65, 5),    # one pixel over in both axes
    (2, 19, 70, 3),    # two frames
    (1, 1, 150, 2),    # one row
    (1, 33, 17, 5),    # tall, with the largest halo
    (1, 23, 67, 4),
]
IDS = ["%dx%dx%d_r%d" % c for c in GPU_CASES]
ITERATIONS = (1, 2, 5)   # two is the least that reads a halo another workgroup wrote
GUIDES = ("random", "constant", "step", "salt", "nonfinite")
SALT_STEP = 6            # above the largest radius: no salt pixel sees another


def options(r=5, iterations=5, guide="random", **kw):
    from fosvos_hip.options import CrfOptions
    if guide == "salt":
        kw.setdefault("theta_rgb", 1.0)   # RGB[255] underflows to 0: a salt pixel's every neighbour weighs nothing
    return CrfOptions(iterations=iterations, radius=r, **kw)


def prepared(frames_u8):
    """uint8 [N,H,W,3] -> float32 [N,3,H,W]: what the prep and the loaders make of frames."""
    from util import frame_overlay as F
    return np.ascontiguousarray(np.concatenate([F.prepare_frame(f) for f in frames_u8]))


def salt_frames(n, h, w):
    """uint8 [N,H,W,3]: isolated pixels of 255 on 0, ``SALT_STEP`` apart."""
    f = np.zeros((n, h, w, 3), dtype=np.uint8)
    f[:, min(2, h - 1)::SALT_STEP, min(3, w - 1)::SALT_STEP] = 255
    return f


def image(n, h, w, guide):
    """float32 [N,3,H,W]: the net's input of a guide kind."""
    if guide in G.KINDS:
        return prepared(G.frames(n, h, w, guide))
    if guide == "salt":
        return prepared(salt_frames(n, h, w))
    assert guide == "nonfinite"
    x = prepared(G.frames(n, h, w, "random"))
    flat = x.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30)):
        flat[(5 + 3 * k) % flat.size::max(flat.size // 4, 1) + 7] = np.float32(v)
    return x


def logits(n, h, w):
    """float32 [N,1,H,W]: sigma 3 with ``guided_cases.SPECIALS`` planted."""
    return G.logits(n, h, w, special=True)


@functools.lru_cache(maxsize=None)
def reference(case, guide, iterations, weights=None):
    """(image, logits, options, tables, refined float32 [N,1,H,W]) of a case: the numpy definition, computed once and shared.
    Read-only arrays."""
    n, h, w, r = case
    kw = {} if weights is None else {"weight_appearance": weights[0], "weight_smooth": weights[1]}
    o = options(r, iterations, guide, **kw)
    im, x, tab = image(n, h, w, guide), logits(n, h, w), M.tables(o)
    want = M.refine_batch(im, x, o, tab)
    for a in (im, x, tab, want):
        a.setflags(write=False)
    return im, x, o, tab, want


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """None, or one line that says how the two float32 arrays differ.  The CRF's output is finite for every input, so every
    value must agree to the last bit."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return "shapes / dtypes differ: %s %s and %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    if not bad.any():
        return None
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    return "%d of %d values differ; first at %s: got %r (bits %#x), expected %r (bits %#x)" % (
        int(bad.sum()), bad.size, at, float(got[at]), int(bits(got)[at]), float(want[at]), int(bits(want)[at]))


# ------------------------------------------------------------------------------------------ the prototype case
def _nearest_distance(mask):
    """float64 [H,W]: the Euclidean distance of every pixel to the nearest True pixel of ``mask`` (exact, two passes)."""
    h, w = mask.shape
    rows = np.arange(h, dtype=np.float64)
    gap = np.abs(rows[:, None, None] - rows[None, :, None])                 # [y, y', 1]
    col = np.where(mask[None, :, :], gap, np.inf).min(axis=1)               # [y, x]: the nearest True in column x
    cols = np.arange(w, dtype=np.float64)
    side = (cols[:, None] - cols[None, :]) ** 2                             # [x, x']
    return np.sqrt((side[None, :, :] + (col ** 2)[:, None, :]).min(axis=2))


def signed_distance(mask):
    """float64 [H,W]: positive inside ``mask`` (the distance to the nearest pixel outside), negative outside."""
    return _nearest_distance(~mask) - _nearest_distance(mask)


BLOB = (slice(8, 12), slice(20, 25))   # the stray 4 x 5 blob, far from the ellipse


@functools.lru_cache(maxsize=None)
def prototype_case():
    """(frame uint8 [97,161,3], truth bool [97,161], logits float32 [97,161]): a contrasting ellipse with +-12 of noise (the
    frame of ``guided_cases.ellipse_case``); the net's mask is the true one shifted by three pixels, its logits are ``6 tanh(signed
    distance / 6)`` plus noise of sigma 0.5, and one stray 4 x 5 blob of object far from the ellipse."""
    frame, truth, _ = G.ellipse_case()
    net_mask = np.roll(truth, 3, axis=1)
    rng = np.random.default_rng(1)
    lg = 6.0 * np.tanh(signed_distance(net_mask) / 6.0) + 0.5 * rng.standard_normal(truth.shape)
    assert not truth[BLOB].any() and not net_mask[BLOB].any()
    lg[BLOB] = 3.0
    lg = np.ascontiguousarray(lg.astype(np.float32))
    for a in (frame, truth, lg):
        a.setflags(write=False)
    return frame, truth, lg


iou = G.iou


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


class CrfByDefinition:
    """A net whose ``forward`` applies the numpy definition behind ``net``: the frames go through ``net`` (on ``device``; None:
    the host), and ``mask_crf.refine`` refines every frame's answer on the host with the frame as the guide.  A pass WITHOUT
    ``crf`` over this net is what a pass with it must equal."""

    def __init__(self, net, crf, device=None):
        self.net, self.crf, self.device = net, crf, device

    def forward(self, x):
        out = self.net.forward(x)[-1].detach().float().cpu().contiguous().numpy()
        refined = torch.from_numpy(M.refine_batch(x.detach().float().cpu().contiguous().numpy(), out, self.crf))
        return [refined if self.device is None else refined.to(self.device)]


def files_of(root):
    """name -> bytes of every file below ``root``."""
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}
