"""Seeded inputs of the JPEG tests, shared by the CPU test of the layout (tests/test_jpeg_layout_cpu.py) and the GPU test of
the kernels (tests/test_gpu_jpeg.py), so that both look at the same frames.  Frames are uint8 [H,W,3] BGR or [H,W] grey."""
import io

import numpy as np
from PIL import Image

QUALITIES = (1, 50, 90, 100)
# 1x1; one whole block; both edges ragged; two block rows, whole columns; one restart interval; a short last interval
SIZES = ((1, 1), (8, 8), (7, 9), (17, 16), (33, 47), (61, 107))
MANY = (120, 214)  # 15 x 27 MCUs: 13 restart intervals, the markers go round RST0..RST7 and on


def noise(h, w, grey=False, seed=0):
    rng = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    return rng.integers(0, 256, (h, w) if grey else (h, w, 3), dtype=np.uint8)


def smooth(h, w, grey=False):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 100 * np.sin(x / 9.0 + y / 23.0), 128 + 90 * np.cos(y / 7.0 + x / 13.0), 40 + 1.5 * x + 0.8 * y]
    img = np.stack([np.clip(p, 0, 255) for p in planes], -1).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0]) if grey else img


def picture(h, w, grey=False):
    """Smooth content with an edge and some noise: every size of SIZES gets DC and AC symbols."""
    img = smooth(h, w, grey).astype(np.int32)
    img[h // 3:, w // 2:] = 255 - img[h // 3:, w // 2:]
    img += np.random.default_rng(h * 131 + w).integers(-6, 7, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def constant(h, w, grey=False, value=128):
    return np.full((h, w) if grey else (h, w, 3), value, dtype=np.uint8)


def checker(h, w, grey=False):
    """8x8 blocks alternating 0 / 255: the DC difference of neighbours is 2040, size category 11, at quality 100."""
    y, x = np.mgrid[0:h, 0:w]
    g = (((y // 8 + x // 8) % 2) * 255).astype(np.uint8)
    return g if grey else np.ascontiguousarray(np.stack([g] * 3, -1))


def corner_cosine(h, w, grey=False, amplitude=20.0):
    """The (7,7) basis function at a low amplitude on mid grey: only coefficient 63 of a block survives quantisation at
    quality 50 - a run of 62 zeros (three ZRLs) and no EOB."""
    y, x = np.mgrid[0:h, 0:w]
    g = 128 + amplitude * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
    g = np.round(g).astype(np.uint8)
    return g if grey else np.ascontiguousarray(np.stack([g] * 3, -1))


# (name, maker, quality) of the coverage inputs (item 4), each at 24x40: 15 MCUs
COVERAGE = (("constant", constant, 90), ("checker", checker, 100), ("corner_cosine", corner_cosine, 50), ("noise", noise, 100))
COVERAGE_SIZE = (24, 40)


def pil_encode(img, quality, ri):
    """PIL's own file of the same frame with the layout's parameters."""
    b = io.BytesIO()
    im = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[..., ::-1]))
    im.save(b, "JPEG", quality=quality, subsampling=0, optimize=False, restart_marker_blocks=ri)
    return b.getvalue()


def decode(data):
    """PIL's decode of a file: (mode, array) with a colour picture back in BGR."""
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    return im.mode, (a if a.ndim == 2 else a[..., ::-1])


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def all_inputs():
    """[(id, frame, quality)]: every input of items 1, 3 and 4, colour and grey, at every quality they are run at."""
    out = []
    for grey in (False, True):
        tag = "grey" if grey else "bgr"
        for h, w in SIZES:
            for q in QUALITIES:
                out.append(("picture_%dx%d_%s_q%d" % (h, w, tag, q), picture(h, w, grey), q))
        for q in QUALITIES:
            out.append(("picture_%dx%d_%s_q%d" % (MANY + (tag, q)), picture(*MANY, grey), q))
        out.append(("noise_%dx%d_%s_q100" % (MANY + (tag,)), noise(*MANY, grey), 100))
        out.append(("noise_61x107_%s_q100" % tag, noise(61, 107, grey), 100))
        for name, make, q in COVERAGE:
            for qq in QUALITIES if name != "noise" else (q,):
                out.append(("%s_%s_q%d" % (name, tag, qq), make(*COVERAGE_SIZE, grey), qq))
    return out
