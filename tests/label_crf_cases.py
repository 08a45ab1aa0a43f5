"""The cases the joint CRF's CPU and GPU tests share (tests/test_label_crf_cpu.py, tests/test_gpu_crf_labels.py): shapes, logit
maps, the numpy definition's answers computed once, the two-object prototype case and the stand-in nets.  A plain module of data
and helpers: it holds no test of its own.  Guides, options and the bit comparison are tests/mask_crf_cases.py's."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guided_cases as G  # noqa: E402
import mask_crf_cases as C  # noqa: E402
from util import label_crf as LC  # noqa: E402

CHUNK = 4   # the labels a workgroup holds at a time (csrc/crf.hip: kLabelChunk)
# (N, H, W, r, K).  The kernel's tile is 16 x 64; K + 1 labels are walked in chunks of CHUNK.
GPU_CASES = [
    (1, 1, 1, 5, 1),       # a 1 x 1 map: no neighbour at all
    (1, 3, 5, 5, 2),       # every window clipped on all sides
    (1, 16, 64, 1, 3),     # exactly one tile, exactly one chunk
    (1, 17, 65, 5, 2),     # one pixel over in both axes
    (2, 19, 70, 3, 3),     # two frames
    (1, 1, 150, 2, 16),    # one row, the most labels: five chunks, the last of one label
    (1, 33, 17, 5, 5),     # tall, with the largest halo; a chunk and half a chunk
    (1, 23, 67, 4, CHUNK - 1),   # K + 1 is exactly one chunk
    (1, 23, 67, 4, CHUNK),       # ... and one label more
]
IDS = ["%dx%dx%d_r%d_k%d" % c for c in GPU_CASES]
ITERATIONS = C.ITERATIONS
GUIDES = ("random", "constant", "salt", "nonfinite")


def logit_maps(n, h, w, k):
    """K arrays float32 [N,1,H,W]: sigma 3, every map with ``guided_cases.SPECIALS`` planted at places of its own, and EQUAL
    values planted across the nets: all nets equal (positive, negative, +inf, NaN) and pairs of nets equal above the rest."""
    rng = np.random.default_rng(G.seed_of(n, h, w) + 17 * k)
    maps = []
    for j in range(k):
        x = (3.0 * rng.standard_normal((n, 1, h, w))).astype(np.float32)
        flat = x.reshape(-1)
        for s, v in enumerate(G.SPECIALS):
            flat[(3 + 7 * s + 5 * j) % flat.size::max(flat.size // 3, 1) + 11] = np.float32(v)
        maps.append(x)
    size = maps[0].size
    for s, v in enumerate((2.5, -1.25, np.inf, np.nan, 0.0, 7.0)):   # every net the same value
        for x in maps:
            x.reshape(-1)[(1 + 13 * s) % size::max(size // 2, 1) + 5] = np.float32(v)
    if k >= 2:                                                         # the last two nets equal and above everything finite
        for x in maps[-2:]:
            x.reshape(-1)[31 % size::max(size // 5, 1) + 3] = np.float32(5.5)
    return maps


@functools.lru_cache(maxsize=None)
def reference(case, guide, iterations, weights=None, clip=None):
    """(image, K logit maps, options, tables, labels uint8 [N,H,W], scores float32 [N,K+1,H,W]) of a case: the numpy definition,
    computed once and shared.  Read-only arrays."""
    n, h, w, r, k = case
    kw = {} if weights is None else {"weight_appearance": weights[0], "weight_smooth": weights[1]}
    if clip is not None:
        kw["clip"] = clip
    o = C.options(r, iterations, guide, **kw)
    im, maps, tab = C.image(n, h, w, guide), logit_maps(n, h, w, k), LC.tables(o)
    labels, scores = LC.refine_labels_batch(im, maps, o, tab)
    for a in [im, tab, labels, scores] + maps:
        a.setflags(write=False)
    return im, tuple(maps), o, tab, labels, scores


# ------------------------------------------------------------------------------------------ the two-object prototype case
PROTO_SIZE = (97, 161)
PROTO_OWN, PROTO_OTHER, PROTO_BACKGROUND, PROTO_SIGMA = 3.0, 1.5, -3.0, 1.5


@functools.lru_cache(maxsize=None)
def two_object_case():
    """(frame uint8 [97,161,3], truth uint8 [97,161] in 0..2, logits: two float32 [97,161]): two touching ellipses of nearly the
    same colour on a dark ground, +-12 of noise on the frame.  Each net answers on BOTH instances - ``PROTO_OWN`` on its own,
    1.5 lower on the other one, ``PROTO_BACKGROUND`` elsewhere - with logit noise of sigma 1.5: the hard case of two instances
    that look alike."""
    h, w = PROTO_SIZE
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    one = ((yy - 48.0) / 30.0) ** 2 + ((xx - 55.0) / 28.0) ** 2 <= 1.0
    two = (((yy - 48.0) / 30.0) ** 2 + ((xx - 108.0) / 26.0) ** 2 <= 1.0) & ~one
    truth = np.where(one, 1, np.where(two, 2, 0)).astype(np.uint8)
    assert (one[:, 1:] & two[:, :-1]).any() or (one[:, :-1] & two[:, 1:]).any()     # they touch
    colours = np.array([[40, 50, 45], [200, 120, 80], [192, 126, 88]], dtype=np.float64)
    rng = np.random.default_rng(7)
    frame = colours[truth] + rng.integers(-12, 13, (h, w, 3))
    frame = np.ascontiguousarray(np.clip(frame, 0, 255).astype(np.uint8))
    logits = []
    for k in (1, 2):
        clean = np.where(truth == k, PROTO_OWN, np.where(truth == 0, PROTO_BACKGROUND, PROTO_OTHER))
        noise = PROTO_SIGMA * np.random.default_rng(10 + k).standard_normal((h, w))
        logits.append(np.ascontiguousarray((clean + noise).astype(np.float32)))
    for a in [frame, truth] + logits:
        a.setflags(write=False)
    return frame, truth, tuple(logits)


def object_ious(labels, truth):
    return [C.iou(labels == k, truth == k) for k in (1, 2)]


# ------------------------------------------------------------------------------------------ stand-in nets
class JointByDefinition:
    """Net ``index`` of K whose ``forward`` applies the numpy definition behind ALL of ``nets``: the frames go through every
    net, ``label_crf.refine_labels_batch`` labels them on the host with the frames as the guide, and the answer is +1 where the
    label is ``index + 1`` and -1 elsewhere.  A pass WITHOUT ``crf`` over K of these merges to the definition's label maps: what a
    pass with ``crf_joint`` must equal."""

    def __init__(self, nets, index, crf, device=None):
        self.nets, self.index, self.crf, self.device = nets, index, crf, device

    def forward(self, x):
        outs = [net.forward(x)[-1].detach().float().cpu().contiguous().numpy() for net in self.nets]
        labels, _ = LC.refine_labels_batch(x.detach().float().cpu().contiguous().numpy(), outs, self.crf)
        answer = torch.from_numpy(np.where(labels == self.index + 1, np.float32(1.0), np.float32(-1.0))[:, None].copy())
        return [answer if self.device is None else answer.to(self.device)]
