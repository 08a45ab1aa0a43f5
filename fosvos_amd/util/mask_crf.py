"""Refining the test pass's logits with a conditional random field on the frame's colours, on the host in numpy: the locally
connected form of the dense CRF (Kraehenbuehl & Koltun 2011; ConvCRF, Teichmann & Cipolla 2018).  Mean-field inference over a
``(2r+1) x (2r+1)`` window with an appearance kernel (near AND alike in colour) and a smoothness kernel (near), a few
iterations.  The net's coarse, blurred edge moves onto the colour edge of the picture, and small islands the picture does not
support go away.

These functions are the project's statement of that arithmetic.  The HIP kernel (csrc/crf.hip: fosvos_crf_refine) is compared
with ``refine`` bit for bit.  So that a kernel can match there is no transcendental in the per-frame arithmetic: every ``exp``
and ``tanh`` is a TABLE the host computes once (``tables``) and hands to the kernel and to ``refine`` alike; every float64
operation below is ONE correctly rounded IEEE operation, the order of every addition is fixed, and nothing is contracted into
a fused multiply-add.

Options (``fosvos_hip.options.CrfOptions``, or anything with these attributes; ``Params`` here holds the defaults):
``iterations`` T in 1..10, ``radius`` r in 1..5, ``theta_pos`` in [0.25, 1e3], ``theta_rgb`` in [1, 1e3], ``theta_smooth`` in
[0.25, 1e3], ``weight_appearance`` and ``weight_smooth`` in [0, 100], ``clip`` in (0, 1e4].

Tables, one float64 vector ``[256 | (2r+1)^2 | (2r+1)^2 | 2049]``:
* ``RGB[d] = exp(-d^2 / (2 theta_rgb^2))``, d = 0..255
* ``A[dy+r, dx+r] = exp(-(dy^2 + dx^2) / (2 theta_pos^2))``
* ``B[dy+r, dx+r] = exp(-(dy^2 + dx^2) / (2 theta_smooth^2))``
* ``D[i] = tanh((i/64 - 16) / 2)``, i = 0..2048

Per frame.  Guide levels, from the net's input ``image`` float32 [3,H,W] (the frame minus MEANVAL): ``t = (f64(v) +
f64(f32(MEANVAL[c]))) + 0.5``; ``g = t >= 0 ? (t < 256 ? floor(t) : 255) : 0`` - a NaN compares false and gives 0.  For
anything the prep or the loaders made, ``g`` is the frame's byte.  A frame uint8 [H,W,3] is its own guide.

Unary: ``u = f64(logit)`` clipped to ``[-clip, clip]`` as util/guided_upsample.py clips, so a NaN becomes ``-clip``.  ``z^0 = u``.

Belief of a value z: ``zc = min(max(z, -16), 16)``; ``p = (zc + 16.0) * 64.0``; ``i = min(int(floor(p)), 2047)``; ``f = p - i``;
``s = D[i] + f * (D[i+1] - D[i])`` - that is ``2 sigmoid(z) - 1``, piecewise linear, to about 1e-5.

Iteration t = 1..T.  Every pixel has four running sums ``Na, Da, Ns, Ds`` that start from 0.0 and run over the offsets
``(dy, dx)`` in raster order, ``dy`` ascending outside and ``dx`` ascending inside.  The centre is skipped; a neighbour outside
the map is skipped, not added as zero.  For each neighbour j, with ``s_j`` the belief of ``z^{t-1}_j``:
``a = A[dy,dx] * ((RGB[|d0|] * RGB[|d1|]) * RGB[|d2|])`` (``d_c`` the difference of the guide levels of channel c, in the
image's channel order), ``b = B[dy,dx]``; ``Na = Na + a * s_j``; ``Da = Da + a``; ``Ns = Ns + b * s_j``; ``Ds = Ds + b``.  Then
``ma = Da > 0 ? Na / Da : 0.0`` (``RGB`` underflows to 0 at small ``theta_rgb``: a pixel whose every neighbour is far in
colour has ``Da == 0``), ``ms = Ds > 0 ? Ns / Ds : 0.0`` (a 1 x 1 map has no neighbour), and
``z^t = (u + weight_appearance * ma) + weight_smooth * ms``.

Output: ``float32(z^T)``, round to nearest even.  Finite for every input; ``|z| <= clip + weight_appearance + weight_smooth``.
With both weights 0, and on a 1 x 1 map, it is ``float32(u)`` as a number; the sign of a zero is that of ``(u + 0.0) + 0.0``.
"""
import math
from typing import NamedTuple

import numpy as np

from dataloaders.davis_2016 import MEANVAL

MAX_RADIUS = 5
MAX_ITERATIONS = 10
THETA_POS_RANGE = (0.25, 1e3)
THETA_RGB_RANGE = (1.0, 1e3)
THETA_SMOOTH_RANGE = (0.25, 1e3)
MAX_WEIGHT = 100.0
MAX_CLIP = 1e4
BELIEF_LIMIT = 16.0     # the belief table spans [-16, 16] ...
BELIEF_PER_UNIT = 64.0  # ... in steps of 1/64
BELIEF_STEPS = 2048


class Params(NamedTuple):
    """The defaults (DenseCRF-like, unmeasured on trained nets); ``fosvos_hip.options.CrfOptions`` has the same fields."""
    iterations: int = 5
    radius: int = 5
    theta_pos: float = 8.0
    theta_rgb: float = 13.0
    theta_smooth: float = 3.0
    weight_appearance: float = 4.0
    weight_smooth: float = 3.0
    clip: float = 6.0


def check_options(options=None) -> Params:
    """The options as ``Params`` of an int and float64 values, or ValueError with the range."""
    o = Params() if options is None else options
    ints = (("iterations", 1, MAX_ITERATIONS), ("radius", 1, MAX_RADIUS))
    reals = (("theta_pos",) + THETA_POS_RANGE, ("theta_rgb",) + THETA_RGB_RANGE, ("theta_smooth",) + THETA_SMOOTH_RANGE,
             ("weight_appearance", 0.0, MAX_WEIGHT), ("weight_smooth", 0.0, MAX_WEIGHT), ("clip", 0.0, MAX_CLIP))
    got = {}
    for name, lo, hi in ints:
        v = getattr(o, name)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
        got[name] = int(v)
    for name, lo, hi in reals:
        v = getattr(o, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v):
            raise ValueError("%s must be a finite number, got %r" % (name, v))
        if not (lo < v if name == "clip" else lo <= v) or not v <= hi:
            raise ValueError("%s must be in %s%g, %g], got %r" % (name, "(" if name == "clip" else "[", lo, hi, v))
        got[name] = np.float64(v)
    return Params(**got)


def table_sizes(radius: int):
    """(offset of A, offset of B, offset of D, length) of the table vector of a radius."""
    k = (2 * int(radius) + 1) ** 2
    return 256, 256 + k, 256 + 2 * k, 256 + 2 * k + BELIEF_STEPS + 1


def tables(options=None) -> np.ndarray:
    """float64 ``[256 | (2r+1)^2 | (2r+1)^2 | 2049]`` = ``[RGB | A | B | D]``.  The one place with an ``exp`` or a ``tanh``: what
    it returns is DATA to the kernel and to ``refine``, so how this host rounds them does not enter the comparison."""
    o = check_options(options)
    r = o.radius
    d = np.arange(256, dtype=np.float64)
    rgb = np.exp(-(d * d) / (2.0 * o.theta_rgb * o.theta_rgb))
    off = np.arange(-r, r + 1, dtype=np.float64)
    d2 = off[:, None] * off[:, None] + off[None, :] * off[None, :]
    a = np.exp(-d2 / (2.0 * o.theta_pos * o.theta_pos))
    b = np.exp(-d2 / (2.0 * o.theta_smooth * o.theta_smooth))
    i = np.arange(BELIEF_STEPS + 1, dtype=np.float64)
    dd = np.tanh((i / BELIEF_PER_UNIT - BELIEF_LIMIT) / 2.0)
    out = np.ascontiguousarray(np.concatenate([rgb, a.reshape(-1), b.reshape(-1), dd]))
    assert out.dtype == np.float64 and out.size == table_sizes(r)[3]
    return out


def _split_tables(tab, o: Params):
    tab = np.asarray(tab)
    oa, ob, od, total = table_sizes(o.radius)
    if tab.dtype != np.float64 or tab.shape != (total,):
        raise ValueError("the tables of radius %d are a float64 [%d] vector, got %s %s" % (o.radius, total, tab.dtype, tab.shape))
    k = 2 * o.radius + 1
    return tab[:oa], tab[oa:ob].reshape(k, k), tab[ob:od].reshape(k, k), tab[od:]


def guide_levels(image: np.ndarray) -> np.ndarray:
    """float32 [3,H,W] (the net's input) -> uint8 [3,H,W]: the frame's bytes again."""
    image = np.asarray(image)
    if image.dtype != np.float32 or image.ndim != 3 or image.shape[0] != 3 or image.size == 0:
        raise ValueError("image must be a non-empty float32 [3,H,W], got %s %s" % (image.dtype, image.shape))
    mean = np.array(MEANVAL, dtype=np.float32).astype(np.float64)
    t = (image.astype(np.float64) + mean[:, None, None]) + 0.5
    with np.errstate(invalid="ignore"):
        inside = np.where(t < 256.0, np.floor(t), 255.0)
        g = np.where(t >= 0.0, inside, 0.0)   # a NaN compares false: 0
    return np.ascontiguousarray(g.astype(np.uint8))


def _guide(image) -> np.ndarray:
    """The guide uint8 [3,H,W] of either input form: the net's input float32 [3,H,W] or the frame uint8 [H,W,3]."""
    image = np.asarray(image)
    if image.dtype == np.uint8:
        if image.ndim != 3 or image.shape[2] != 3 or image.size == 0:
            raise ValueError("a frame must be a non-empty uint8 [H,W,3], got %s" % (image.shape,))
        return np.ascontiguousarray(image.transpose(2, 0, 1))
    return guide_levels(image)


def unary(logits: np.ndarray, clip) -> np.ndarray:
    """float32 [H,W] -> float64 [H,W]: the clipped logit; a NaN is ``-clip``."""
    logits = np.asarray(logits)
    if logits.dtype != np.float32 or logits.ndim != 2 or logits.size == 0:
        raise ValueError("logits must be a non-empty float32 [H,W], got %s %s" % (logits.dtype, logits.shape))
    clip = np.float64(clip)
    x = logits.astype(np.float64)
    with np.errstate(invalid="ignore"):
        u = np.where(x >= -clip, x, -clip)   # a NaN compares false: -clip
        u = np.where(u <= clip, u, clip)
    return u


def belief(z, dd: np.ndarray):
    """``2 sigmoid(z) - 1`` of finite float64 values, piecewise linear on the table ``dd`` = D."""
    z = np.asarray(z, dtype=np.float64)
    zc = np.minimum(np.maximum(z, -BELIEF_LIMIT), BELIEF_LIMIT)
    p = (zc + BELIEF_LIMIT) * BELIEF_PER_UNIT
    i = np.minimum(np.floor(p).astype(np.int64), BELIEF_STEPS - 1)
    f = p - i.astype(np.float64)
    return dd[i] + f * (dd[i + 1] - dd[i])


def _operands(image, logits, options, tab):
    o = check_options(options)
    g = _guide(image).astype(np.int64)
    u = unary(logits, o.clip)
    if g.shape[1:] != u.shape:
        raise ValueError("the guide is %s, the logits are %s" % (g.shape[1:], u.shape))
    rgb, a, b, dd = _split_tables(tables(o) if tab is None else tab, o)
    return o, g, u, rgb, a, b, dd


def messages(image, logits, options=None, tables=None):
    """(z^T float64 [H,W], Da float64 [H,W]) - ``refine`` before its rounding, and the appearance kernel's mass at every pixel."""
    o, g, u, rgb, ta, tb, dd = _operands(image, logits, options, tables)
    h, w = u.shape
    r = o.radius
    z = u
    da = np.zeros((h, w), dtype=np.float64)
    for _ in range(o.iterations):
        s = belief(z, dd)
        na, da, ns, ds = (np.zeros((h, w), dtype=np.float64) for _ in range(4))
        for dy in range(-r, r + 1):
            ylo, yhi = max(0, -dy), min(h, h - dy)
            for dx in range(-r, r + 1):
                xlo, xhi = max(0, -dx), min(w, w - dx)
                if (dy == 0 and dx == 0) or ylo >= yhi or xlo >= xhi:
                    continue
                here = (slice(ylo, yhi), slice(xlo, xhi))
                there = (slice(ylo + dy, yhi + dy), slice(xlo + dx, xhi + dx))
                d0, d1, d2 = (np.abs(g[c][here] - g[c][there]) for c in range(3))
                a = ta[dy + r, dx + r] * ((rgb[d0] * rgb[d1]) * rgb[d2])
                b = tb[dy + r, dx + r]
                sj = s[there]
                na[here] = na[here] + a * sj
                da[here] = da[here] + a
                ns[here] = ns[here] + b * sj
                ds[here] = ds[here] + b
        with np.errstate(invalid="ignore", divide="ignore"):
            ma = np.where(da > 0.0, na / da, 0.0)
            ms = np.where(ds > 0.0, ns / ds, 0.0)
        z = (u + o.weight_appearance * ma) + o.weight_smooth * ms
    return z, da


def refine(image, logits, options=None, tables=None) -> np.ndarray:
    """The refined logits float32 [H,W] of one frame.  ``image``: the net's input float32 [3,H,W], or the frame uint8 [H,W,3];
    ``logits`` float32 [H,W]; ``tables``: what ``tables(options)`` returned (None: made here).  Vectorised over the pixels,
    sequential over the offsets."""
    return np.ascontiguousarray(messages(image, logits, options, tables)[0].astype(np.float32))


def refine_loop(image, logits, options=None, tables=None) -> np.ndarray:
    """``refine`` as a plain double loop over the pixels, the module's text line by line (Python floats are IEEE float64)."""
    o, g, u, rgb, ta, tb, dd = _operands(image, logits, options, tables)
    h, w = u.shape
    r = o.radius
    g, rgb, ta, tb, dd = g.tolist(), rgb.tolist(), ta.tolist(), tb.tolist(), dd.tolist()
    wa, ws = float(o.weight_appearance), float(o.weight_smooth)
    u = [[float(v) for v in row] for row in u]

    def belief_of(zv):
        zc = min(max(zv, -BELIEF_LIMIT), BELIEF_LIMIT)
        p = (zc + BELIEF_LIMIT) * BELIEF_PER_UNIT
        i = min(int(math.floor(p)), BELIEF_STEPS - 1)
        f = p - i
        return dd[i] + f * (dd[i + 1] - dd[i])

    z = u
    for _ in range(o.iterations):
        s = [[belief_of(v) for v in row] for row in z]
        nxt = [[0.0] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                na = da = ns = ds = 0.0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        yy, xx = y + dy, x + dx
                        if (dy == 0 and dx == 0) or yy < 0 or yy >= h or xx < 0 or xx >= w:
                            continue
                        a = ta[dy + r][dx + r] * ((rgb[abs(g[0][y][x] - g[0][yy][xx])] * rgb[abs(g[1][y][x] - g[1][yy][xx])])
                                                  * rgb[abs(g[2][y][x] - g[2][yy][xx])])
                        b = tb[dy + r][dx + r]
                        na = na + a * s[yy][xx]
                        da = da + a
                        ns = ns + b * s[yy][xx]
                        ds = ds + b
                ma = na / da if da > 0.0 else 0.0
                ms = ns / ds if ds > 0.0 else 0.0
                nxt[y][x] = (u[y][x] + wa * ma) + ws * ms
        z = nxt
    return np.ascontiguousarray(np.array(z, dtype=np.float64).reshape(h, w).astype(np.float32))


def refine_batch(images, logits, options=None, tables=None) -> np.ndarray:
    """``refine`` frame by frame: images float32 [N,3,H,W] and logits float32 [N,1,H,W] -> float32 [N,1,H,W]."""
    images, logits = np.asarray(images), np.asarray(logits)
    if images.ndim != 4 or logits.ndim != 4 or logits.shape[1] != 1 or logits.shape[0] != images.shape[0]:
        raise ValueError("images [N,3,H,W] and logits [N,1,H,W], got %s and %s" % (images.shape, logits.shape))
    o = check_options(options)
    tab = _tables(o) if tables is None else tables
    return np.ascontiguousarray(np.stack([refine(images[k], logits[k, 0], o, tab) for k in range(images.shape[0])])[:, None])


_tables = tables  # under a name the ``tables=`` arguments above do not hide
