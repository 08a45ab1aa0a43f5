"""Shapes, inputs and references shared by tests/test_guided_upsample_cpu.py and tests/test_gpu_guided_upsample.py (not a test
module).  The band of the soft modes is the one of tests/frame_overlay_cases.py."""
import functools

import numpy as np

from frame_overlay_cases import ALPHAS, BAND, BAND_SHARE, SOFT_ALPHAS  # noqa: F401

# (N, Hf, Wf, Hn, Wn, r): frames of [Hf,Wf], the net at [Hn,Wn], windows of radius r.  The fit kernel's tile is 16 x 64.
CASES = [
    (1, 7, 9, 3, 5, 8),         # the map is smaller than the radius in both axes: every window is clipped on both sides
    (2, 37, 131, 19, 70, 3),    # two frames, a non-integer ratio, the map crosses a 16 x 64 tile in both axes
    (1, 40, 96, 20, 48, 1),     # exactly 2x
    (1, 23, 67, 23, 67, 4),     # equal sizes; a row length that is no multiple of 16: the stores' heads and tails
    (1, 5, 300, 1, 150, 2),     # one net row, several 16-pixel groups a row
    (1, 64, 33, 33, 17, 8),     # tall, with the largest halo
]
IDS = ["%dx%dx%d_to_%dx%d_r%d" % c for c in CASES]
KINDS = ("random", "constant", "step")
EPS = (1e-3, 400.0)
CLIP = 6.0


def seed_of(n, h, w):
    return 100000 * n + 1000 * h + w


def frames(n, hf, wf, kind="random"):
    """uint8 [N,Hf,Wf,3]: random bytes, one grey level, or a 0 / 255 vertical step."""
    if kind == "random":
        return np.random.default_rng(seed_of(n, hf, wf)).integers(0, 256, (n, hf, wf, 3), dtype=np.uint8)
    if kind == "constant":
        return np.full((n, hf, wf, 3), 93, dtype=np.uint8)
    assert kind == "step"
    f = np.zeros((n, hf, wf, 3), dtype=np.uint8)
    f[:, :, wf // 2:] = 255
    return f


SPECIALS = (0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30, -100.0)


def logits(n, hn, wn, special=True):
    """float32 [N,1,Hn,Wn]: mean 0 and sigma 3; with ``special`` a few +-0.0, +-inf, NaN, +-1e30 and -100 entries."""
    x = (3.0 * np.random.default_rng(seed_of(n, hn, wn) + 1).standard_normal((n, 1, hn, wn))).astype(np.float32)
    if special:
        flat = x.reshape(-1)
        for k, v in enumerate(SPECIALS):
            flat[(3 + 7 * k) % flat.size::max(flat.size // 3, 1) + 11] = np.float32(v)
    return x


def images(f, hn, wn, mirror=False):
    """float32 [N,3,Hn,Wn]: what the prep makes of the frames for a net of [Hn,Wn]."""
    from util import frame_overlay as F
    from util import frame_resample as R
    if f.shape[1:3] == (hn, wn):
        return np.concatenate([F.prepare_frame(f[k], mirror) for k in range(f.shape[0])])
    return np.concatenate([R.prepare_frame_scaled(f[k], hn, wn, mirror) for k in range(f.shape[0])])


@functools.lru_cache(maxsize=None)
def reference(case, kind, eps, mirror=False):
    """(frames, image, logits, coeff) of a case: the numpy definition, computed once and shared.  Read-only arrays."""
    from util import guided_upsample as G
    n, hf, wf, hn, wn, r = case
    f, x = frames(n, hf, wf, kind), logits(n, hn, wn)
    im = images(f, hn, wn, mirror)
    coeff = np.stack([G.coefficients(im[k], x[k, 0], r, eps, CLIP) for k in range(n)])
    for a in (f, im, x, coeff):
        a.setflags(write=False)
    return f, im, x, coeff


def soft_band_guided(img, coeff, mirror, overlay, color, alpha):
    """bool [Hf,Wf]: ``frame_overlay_cases.soft_band`` with the refined logits - the pixels of one frame where an ulp of exp()
    may decide the soft byte."""
    from util import frame_overlay as F
    from util import guided_upsample as G
    p = G.prediction_guided(coeff, img, mirror, False)
    if overlay:
        c = F.COLOR_CHANNEL[color]
        v = F.mirrored(img, mirror)[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
        return (np.abs(v - np.rint(v)) <= BAND) & (v < 255.0 + BAND)
    v = 255 * p + 0.5
    return np.abs(v - np.rint(v)) <= BAND


# the edge-snap case of the prototype
def ellipse_case():
    """(frame uint8 [97,161,3], truth bool [97,161], logits float32 [31,50]): a contrasting ellipse with +-12 of noise; the net
    runs at 31 x 50 and its mask is the true one, by area coverage >= 0.5, shifted by one net pixel."""
    from util import frame_resample as R
    hf, wf, hn, wn = 97, 161, 31, 50
    yy, xx = np.mgrid[0:hf, 0:wf]
    truth = ((yy - 0.47 * hf) / (0.29 * hf)) ** 2 + ((xx - 0.52 * wf) / (0.31 * wf)) ** 2 <= 1.0
    noise = np.random.default_rng(0).integers(-12, 13, (hf, wf, 3))
    frame = np.clip(np.where(truth, 170, 60)[:, :, None] + noise, 0, 255).astype(np.uint8)
    cover = (R.box_weights(hf, hn) @ truth.astype(np.int64) @ R.box_weights(wf, wn).T) / float(hf * wf)
    lg = np.where(cover >= 0.5, 6.0, -6.0).astype(np.float32)
    return frame, truth, np.ascontiguousarray(np.roll(lg, 1, axis=1))


def iou(a, b):
    return float((a & b).sum()) / float((a | b).sum())
