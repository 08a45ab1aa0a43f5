"""Seeded inputs of the 4:2:0 JPEG tests, shared by the CPU test of the layout (tests/test_jpeg420_layout_cpu.py) and the GPU
test of the kernels (tests/test_gpu_jpeg420.py), so that both look at the same frames.  Frames are uint8 [H,W,3] BGR."""
import io

import numpy as np
from PIL import Image

RI_420 = 16
QUALITIES = (1, 50, 90, 100)
# (H, W): what the shape is there to catch
SIZES = ((16, 16),    # one MCU, no padding
         (8, 8),      # dummy Y blocks right and bottom, one real block
         (1, 1),      # everything replicated
         (9, 17),     # W mod 16 = 1: a chroma column from replicated pixels, a dummy right column in the second MCU
         (24, 40),    # H mod 16 = 8 and W mod 16 = 8: a dummy row and a dummy column together
         (17, 33),    # one real pixel row / column in the last block row / column, no dummies there
         (16, 272),   # 17 MCUs: two intervals, RST0 and the DC reset
         (32, 136))   # 2 rows of 9 MCUs, right-edge dummies, an interval that crosses an MCU row
BATCH = (3, 48, 80)   # per-frame lengths and offsets
WORKLOAD = (480, 854)  # once, at quality 90: 854 mod 16 = 6 (right-edge dummies), 1620 MCUs = 102 intervals, the last one short
CONTENTS = ("noise", "flat", "ramp", "checker")


def noise(h, w, seed=0):
    rng = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def flat(h, w, value=(200, 90, 30)):
    """One colour: every block is a DC (not 0 after the level shift) and an EOB."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.uint8), (h, w, 3)))


def ramp(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(3 * x + y) % 256, (2 * y + 40) % 256, (255 - x - 2 * y) % 256], -1).astype(np.uint8)


def checker(h, w):
    """A saturated checkerboard of single pixels: blue against yellow, the largest AC coefficients there are."""
    y, x = np.mgrid[0:h, 0:w]
    on = ((y + x) & 1).astype(bool)
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[on], img[~on] = (255, 0, 0), (0, 255, 255)
    return img


def workload_frame():
    """Smooth content with an edge and some noise at the workload's size."""
    h, w = WORKLOAD
    img = ramp(h, w).astype(np.int32)
    img[h // 3:, w // 2:] = 255 - img[h // 3:, w // 2:]
    img += np.random.default_rng(7).integers(-6, 7, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def make(content, h, w):
    return {"noise": noise, "flat": flat, "ramp": ramp, "checker": checker}[content](h, w)


def batch():
    n, h, w = BATCH
    return np.stack([noise(h, w, seed=1), ramp(h, w), checker(h, w)][:n])


def pil_encode_420(img, quality):
    """PIL's own 4:2:0 file of the same BGR frame with the layout's parameters."""
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(b, "JPEG", quality=quality, subsampling=2, optimize=False,
                                                               restart_marker_blocks=RI_420)
    return b.getvalue()


def small_inputs():
    """[(id, frame, quality)]: every size of SIZES with every content at every quality, and the frames of the batch."""
    out = []
    for h, w in SIZES:
        for content in CONTENTS:
            for q in QUALITIES:
                out.append(("%s_%dx%d_q%d" % (content, h, w, q), make(content, h, w), q))
    for k, frame in enumerate(batch()):
        for q in QUALITIES:
            out.append(("batch%d_%dx%d_q%d" % ((k,) + BATCH[1:] + (q,)), frame, q))
    return out
