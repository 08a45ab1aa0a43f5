"""Seeded inputs shared by tests/test_frame_overlay_cpu.py and tests/test_gpu_frame_overlay.py (not a test module)."""
import numpy as np

# (N, H, W): mirrored 5x7 is scalar only; 16x16 is one aligned group a row; 33x47 and 61x107 have ragged rows whose bases are
# on no 16-byte boundary; 48x86 and 33x47 hold several frames; 64x128 is all groups
SHAPES = [(1, 5, 7), (1, 16, 16), (2, 33, 47), (1, 61, 107), (3, 48, 86), (1, 64, 128)]
COLORS = ('b', 'g', 'r')
ALPHAS = (0.0, 0.5, 1.0, 2.0)
SOFT_ALPHAS = (0.5, 1.0, 2.0)   # (alpha 0 leaves every byte as it is, exactly: tested without an exclusion)
BAND = 1e-9
BAND_SHARE = 1e-4


def seed_of(n, h, w):
    return 100000 * n + 1000 * h + w


def frames(n, h, w):
    """uint8 [N,H,W,3] with planted 0 and 255 bytes."""
    f = np.random.default_rng(seed_of(n, h, w)).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    flat = f.reshape(-1)
    flat[::7] = 0
    flat[3::11] = 255
    return f


def logits(n, h, w, zeros=True):
    """float32 [N,1,H,W], both signs, no value with 0 < |x| < 1e-6; with ``zeros`` planted +0.0 and -0.0."""
    x = (3.0 * np.random.default_rng(seed_of(n, h, w) + 1).standard_normal((n, 1, h, w))).astype(np.float32)
    small = np.abs(x) < 1e-6
    x[small] = np.where(np.signbit(x[small]), np.float32(-2e-6), np.float32(2e-6))
    if zeros:
        flat = x.reshape(-1)
        flat[::5] = 0.0
        flat[2::13] = -0.0
    return x


def soft_band(img, lg, mirror, overlay, color, alpha):
    """bool [H,W]: the pixels of one frame where an ulp of exp() may decide the soft byte - the float64 value within 1e-9
    of an integer (the overlay truncates there) or, for the mask bytes, 255 p within 1e-9 of a half (it rounds there)."""
    from util import frame_overlay as F
    p = F.prediction(lg, False)
    if overlay:
        c = F.COLOR_CHANNEL[color]
        v = F.mirrored(img, mirror)[:, :, c].astype(np.float64) + (np.float64(alpha) * 255.0) * p
        return (np.abs(v - np.rint(v)) <= BAND) & (v < 255.0 + BAND)
    v = 255 * p + 0.5
    return np.abs(v - np.rint(v)) <= BAND
