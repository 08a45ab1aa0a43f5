"""Shared tables and seeded generators of the several-objects overlay tests (test_object_overlay_cpu.py,
test_gpu_object_overlay.py).  The shapes are the smallest at which the kernels' partition can go wrong, not the workload's."""
import numpy as np

# (N,H,W): head only; one full group; group + tail; head + groups + tail; and, under mirror, rows shorter than a group
SHAPES = [(1, 1, 1), (1, 5, 7), (1, 3, 15), (1, 2, 16), (1, 2, 17), (2, 3, 33), (1, 4, 47), (2, 5, 64)]
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]
KS = (1, 2, 3, 16)
ALPHAS = (0.0, 0.3, 0.5, 1.0)
# (Hf,Wf,Hn,Wn)
SCALED = [(2, 33, 1, 1), (5, 37, 3, 17), (7, 50, 7, 25), (9, 48, 4, 48), (6, 16, 5, 16), (4, 70, 2, 9)]
SCALED_IDS = ["%dx%d_from_%dx%d" % s for s in SCALED]
SCALED_N = 2


def frames(n, h, w, seed=1):
    return np.random.default_rng([seed, n, h, w]).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def random_palette(seed=17):
    """uint8 [256,3] whose three channels differ in every entry: a swapped RGB / BGR order cannot pass."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 256, 256)
    d1, d2 = rng.integers(1, 101, 256), rng.integers(1, 101, 256)
    pal = np.stack([r, (r + d1) % 256, (r + d1 + d2) % 256], axis=1).astype(np.uint8)
    assert (pal[:, 0] != pal[:, 1]).all() and (pal[:, 1] != pal[:, 2]).all() and (pal[:, 0] != pal[:, 2]).all()
    return pal


def palettes():
    """name -> palette (None: the DAVIS one, the default)."""
    return {"davis": None, "random": random_palette()}


def _quarters(rng, shape):
    return (rng.integers(-16, 17, shape) * 0.25).astype(np.float32)  # multiples of 0.25 in [-4, 4]


def logits(k, n, h, w, seed=2):
    """K maps float32 [N,1,H,W] for the unscaled cases: seeded multiples of 0.25, so exact ties and exact zeros occur, then
    up to five planted pixels spread over frame 0 (as many as it has): -0.0 alone (valid), +0.0 alone in the last map, a NaN
    (never valid), +inf in two maps (the lower id wins), and all maps negative (background)."""
    rng = np.random.default_rng([seed, k, n, h, w])
    maps = [_quarters(rng, (n, 1, h, w)) for _ in range(k)]
    p = h * w
    spots = [(i * (p - 1)) // 4 for i in range(5)] if p >= 5 else list(range(p))

    def put(spot, values):
        y, x = divmod(spot, w)
        for m, v in zip(maps, values):
            m[0, 0, y, x] = v

    plants = [[-0.0] + [-1.0] * (k - 1),
              [-2.0] * (k - 1) + [0.0],
              [np.nan] + [-0.5] * (k - 2) + ([1.25] if k > 1 else []),
              [np.inf, np.inf] + [3.0] * (k - 2) if k > 1 else [np.inf],
              [-0.25] * k]
    for spot, values in zip(spots, plants):
        put(spot, values)
    return maps


def logits_scaled(k, n, hn, wn, seed=3):
    """K maps float32 [N,1,Hn,Wn] for the scaled cases: finite (inf x 0 in the taps is NaN on both sides and proves nothing).
    The last map's top-left 2x2 block is zero, so the output's corner pixels interpolate to exactly 0; map 1's first column
    repeats map 0's, so the output's left border holds exact ties."""
    rng = np.random.default_rng([seed, k, n, hn, wn])
    maps = [_quarters(rng, (n, 1, hn, wn)) for _ in range(k)]
    if k > 1:
        maps[1][:, :, :, 0] = maps[0][:, :, :, 0]
    maps[-1][:, :, :2, :2] = 0.0
    return maps


def frame_maps(maps, n):
    """The K [H,W] maps of frame n."""
    return [m[n, 0] for m in maps]
