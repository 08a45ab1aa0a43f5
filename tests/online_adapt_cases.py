"""The cases the CPU and the GPU tests of online adaptation share (util/online_adapt.py, csrc/adapt.hip, the void form of
csrc/loss.hip): shapes that cross a boundary of the kernels, distances, masks, and the net-like labelling input."""
import numpy as np

# (1,1) and (3,5): H W no multiple of 4; (40,52): three loss blocks; (49,83), (70,131): W no multiple of 64, and more than
# one wave a row
SHAPES = [(1, 1), (3, 5), (40, 52), (49, 83), (70, 131)]
BRUTE_SHAPES = [s for s in SHAPES if s[0] * s[1] <= 40 * 52]
DISTANCES = [0, 1, 5, 12, 30, 1000]  # 1000: larger than every frame
ERODES = [0, 2]


def ellipse(h, w, cy=0.45, cx=0.5, ry=0.2, rx=0.16):
    y, x = np.mgrid[0:h, 0:w]
    return ((((y - cy * h) / (ry * h + 0.5)) ** 2 + ((x - cx * w) / (rx * w + 0.5)) ** 2) <= 1.0).astype(np.uint8)


def pair_offset(h, w, d):
    """(dy, dx) with dy^2 + dx^2 == d^2 that fits the frame: a 3-4-5 multiple where d is one, else along the longer axis;
    None where the frame is too small."""
    if d % 5 == 0 and 3 * d // 5 < h and 4 * d // 5 < w:
        return 3 * d // 5, 4 * d // 5
    if d < w:
        return 0, d
    if d < h:
        return d, 0
    return None


def masks(h, w, d):
    """name -> uint8 [H,W]; values other than 1 are used on purpose (a non-zero byte is a set pixel)."""
    out = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}
    corner = np.zeros((h, w), np.uint8)
    corner[h - 1, w - 1] = 1
    out["corner"] = corner
    blob = ellipse(h, w) * 7
    blob[0, w - 1] = 1  # the stray pixel
    out["ellipse_stray"] = blob.astype(np.uint8)
    col0 = np.zeros((h, w), np.uint8)
    col0[:, 0] = 1
    out["column_first"] = col0
    col1 = np.zeros((h, w), np.uint8)
    col1[:, w - 1] = 2
    out["column_last"] = col1
    off = pair_offset(h, w, d)
    if off is not None:  # two pixels at distance exactly d: every pixel at exactly d from one of them must come out 0
        pair = np.zeros((h, w), np.uint8)
        pair[0, 0] = 1
        pair[off[0], off[1]] = 1
        out["pair_at_d"] = pair
    return out


def gate_cases():
    """(id, mask, distance) over every shape, distance and mask."""
    for h, w in SHAPES:
        for d in DISTANCES:
            for name, m in masks(h, w, d).items():
                yield "%dx%d_d%d_%s" % (h, w, d, name), m, d


def stacks():
    """(id, masks uint8 [3,H,W], distance): N = 3 with three different masks."""
    for h, w in SHAPES:
        for d in (1, 12):
            ms = masks(h, w, d)
            yield "%dx%d_d%d" % (h, w, d), np.stack([ms["ellipse_stray"], ms["empty"], ms["column_last"]]), d


def brute_far_from(mask, d, invert=False):
    """The definition itself, O(n^2): 1 at p iff every set q has |p - q|^2 > d^2."""
    h, w = mask.shape
    s = (mask != 0) != invert
    y, x = np.mgrid[0:h, 0:w]
    py, px = y.reshape(-1, 1).astype(np.int64), x.reshape(-1, 1).astype(np.int64)
    qy, qx = y[s].reshape(1, -1).astype(np.int64), x[s].reshape(1, -1).astype(np.int64)
    if qy.size == 0:
        return np.ones((h, w), np.uint8)
    d2 = (py - qy) ** 2 + (px - qx) ** 2
    return (d2.min(axis=1) > d * d).reshape(h, w).astype(np.uint8)


def logits_for(h, w, seed=0):
    """Net-like logits around an ellipse: +-6 plus N(0, 3), rolled 3 pixels against the mask."""
    rng = np.random.default_rng(1000 * h + w + seed)
    m = ellipse(h, w)
    x = np.where(m != 0, 6.0, -6.0) + rng.normal(0.0, 3.0, (h, w))
    return np.roll(x, 3, axis=1).astype(np.float32), m


# the net-like case of the issue: every class must hold at least 5 % of the pixels (a condition on the input)
NET_LIKE = dict(shape=(49, 83), pos_prob=0.97, neg_distance=12, erode=2)


def pos_logit(p):
    import math
    return float(np.float32(math.log(p / (1.0 - p))))


def label_cases():
    """(id, logits f32 [H,W], last_mask u8 [H,W], pos_logit, neg_distance, erode)."""
    for h, w in SHAPES:
        x, m = logits_for(h, w)
        ms = masks(h, w, 5)
        for e in ERODES:
            for d in (0, 5, 12, 1000):
                yield "%dx%d_D%d_E%d_ellipse" % (h, w, d, e), x, m, pos_logit(0.97), d, e
            yield "%dx%d_E%d_empty" % (h, w, e), x, ms["empty"], pos_logit(0.97), 5, e
            yield "%dx%d_E%d_full" % (h, w, e), x, ms["full"], pos_logit(0.9), 1, e
            yield "%dx%d_E%d_corner" % (h, w, e), x, ms["corner"], pos_logit(0.6), 12, e
    # special logit values against the threshold, on a frame with a far zone
    h, w = 3, 5
    t = np.float32(pos_logit(0.97))
    x = np.array([[np.nan, np.inf, -np.inf, -0.0, 0.0],
                  [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)), 100.0, -100.0],
                  [np.nan, np.inf, t, t, 7.0]], dtype=np.float32)
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = 1
    yield "specials_near", x, m, float(t), 1000, 0
    yield "specials_far", x, m, float(t), 2, 0


def loss_inputs(n, h, w, seed=0, void_share=0.4):
    """(logits, label, void) float32 / float32 / uint8 [N,1,H,W]."""
    rng = np.random.default_rng(seed + 31 * n + 7 * h + w)
    x = rng.normal(0.0, 3.0, (n, 1, h, w)).astype(np.float32)
    y = (rng.random((n, 1, h, w)) < 0.3).astype(np.float32)
    v = (rng.random((n, 1, h, w)) < void_share).astype(np.uint8) * rng.integers(1, 256, (n, 1, h, w)).astype(np.uint8)
    return x, y, v
