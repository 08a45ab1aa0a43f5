"""A joint CRF over the objects of a frame, on the host in numpy: ONE mean-field CRF over the labels ``0..K`` (0 = background,
k = object k) in place of K binary ones (util/mask_crf.py) and the label merge behind them (util/object_merge.merge_labels).
The K per-object nets' logits are the unaries, the labels compete at every pixel through a soft-max, and the two pairwise
kernels of util/mask_crf.py - appearance and smoothness over a ``(2r+1) x (2r+1)`` window - carry every label's belief.  Where
two nets both answer "object" a per-net CRF adds the same message to both logits and the merge orders them by the raw logits'
noise as before; here the neighbours' beliefs decide.

These functions are the project's statement of that arithmetic; the HIP kernel (csrc/crf.hip: fosvos_crf_labels) is compared
with ``refine_labels_batch`` bit for bit.  The rules are util/mask_crf.py's: every float64 operation below is ONE correctly
rounded IEEE operation, the order of every addition is fixed, nothing is contracted, and every ``exp`` comes from a table the
host makes once.  ``check_options``, the guide (``_guide`` / ``guide_levels``), ``unary`` and the tables ``RGB``, ``A``, ``B``
are that module's own.

Inputs: ``image`` float32 [3,H,W] (the net's input) or a frame uint8 [H,W,3]; K logit maps float32 [H,W], 1 <= K <=
``object_merge.MAX_OBJECTS``; options as for ``mask_crf`` (``fosvos_hip.options.CrfOptions``, same fields and ranges).

Tables, one float64 vector ``[RGB 256 | A (2r+1)^2 | B (2r+1)^2 | E 2049]``, as long as ``mask_crf.tables``' vector: ``RGB``,
``A`` and ``B`` are ``mask_crf.tables(options)``' own and ``E[i] = exp(-(i / 64))``, i = 0..2048.

Unary: ``U_0 = 0.0``, ``U_k = mask_crf.unary(logit_k, clip)`` (a NaN becomes ``-clip``).  ``z^0 = U``.

Belief of a pixel's ``z_0..z_K`` (a soft-max, piecewise linear on ``E``): ``m = z_0``, then ``m = z_l > m ? z_l : m`` for l
ascending.  For each l: ``d = min(m - z_l, 32.0)``; ``p = d * 64.0``; ``i = min(int(floor(p)), 2047)``; ``f = p - i``;
``e_l = E[i] + f * (E[i+1] - E[i])``.  ``S = 0.0``, then ``S = S + e_l`` for l ascending; ``q_l = e_l / S``.  ``S >= 1``: the
largest label has ``e = E[0] = 1``.

Iteration t = 1..T.  The offsets in ``mask_crf``'s order (``dy`` ascending outside, ``dx`` ascending inside, the centre
skipped; a neighbour outside the map is skipped, not added as zero).  A pixel keeps ``Da``, ``Ds`` and per label ``Na_l``,
``Ns_l``, all from 0.0.  Per neighbour j: ``a = A[dy,dx] * ((RGB[|d0|] * RGB[|d1|]) * RGB[|d2|])``, ``b = B[dy,dx]``;
``Da = Da + a``; ``Ds = Ds + b``; for each l ``Na_l = Na_l + a * q_j(l)`` and ``Ns_l = Ns_l + b * q_j(l)``.  Then
``ma_l = Da > 0 ? Na_l / Da : 0.0``, ``ms_l = Ds > 0 ? Ns_l / Ds : 0.0`` and
``z^t_l = (U_l + weight_appearance * ma_l) + weight_smooth * ms_l``.

Output: ``scores`` float32 [K+1,H,W] = ``float32(z^T_l)``, finite for every input; ``labels`` uint8 [H,W]: start with
``label = 0, val = z^T_0``; for k = 1..K in order take k (``label = k, val = z^T_k``) if ``label == 0 ? z^T_k >= val :
z^T_k > val`` - an object beats the background on a tie and the lowest object wins among equal objects, ``merge_labels``' rule.
With both weights 0 and logits within ``[-clip, clip]`` the labels ARE ``merge_labels``'.
"""
import math

import numpy as np

from util import mask_crf
from util.mask_crf import check_options
from util.object_merge import MAX_OBJECTS

EXP_LIMIT = 32.0      # the exp table spans gaps of [0, 32] ...
EXP_PER_UNIT = 64.0   # ... in steps of 1/64
EXP_STEPS = 2048
assert EXP_STEPS == mask_crf.BELIEF_STEPS  # the vector is as long as ``mask_crf.tables``'


def tables(options=None) -> np.ndarray:
    """float64 ``[RGB | A | B | E]``: ``mask_crf.tables(options)`` with ``E[i] = exp(-(i / 64))`` in the place of ``D``."""
    o = check_options(options)
    tab = mask_crf.tables(o).copy()
    od = mask_crf.table_sizes(o.radius)[2]
    tab[od:] = np.exp(-(np.arange(EXP_STEPS + 1, dtype=np.float64) / EXP_PER_UNIT))
    return np.ascontiguousarray(tab)


def beliefs(z, ee: np.ndarray):
    """z float64 [L,...] (finite) -> (q float64 [L,...], S float64 [...]): the soft-max over the first axis, piecewise linear
    on the table ``ee`` = E."""
    z = np.asarray(z, dtype=np.float64)
    m = z[0]
    for l in range(1, z.shape[0]):
        m = np.where(z[l] > m, z[l], m)
    e = []
    for l in range(z.shape[0]):
        d = np.minimum(m - z[l], EXP_LIMIT)
        p = d * EXP_PER_UNIT
        i = np.minimum(np.floor(p).astype(np.int64), EXP_STEPS - 1)
        f = p - i.astype(np.float64)
        e.append(ee[i] + f * (ee[i + 1] - ee[i]))
    s = np.zeros(z.shape[1:], dtype=np.float64)
    for l in range(z.shape[0]):
        s = s + e[l]
    return np.stack([e[l] / s for l in range(z.shape[0])]), s


def _logit_list(logits):
    maps = [np.asarray(x) for x in logits]
    if not 1 <= len(maps) <= MAX_OBJECTS:
        raise ValueError("%d logit maps, outside [1, %d]" % (len(maps), MAX_OBJECTS))
    return maps


def _operands(image, logits, options, tab):
    o = check_options(options)
    g = mask_crf._guide(image).astype(np.int64)
    maps = _logit_list(logits)
    u = [mask_crf.unary(x, o.clip) for x in maps]
    for x in u:
        if x.shape != g.shape[1:]:
            raise ValueError("the guide is %s, a logit map is %s" % (g.shape[1:], x.shape))
    u = np.stack([np.zeros(g.shape[1:], dtype=np.float64)] + u)
    rgb, a, b, ee = mask_crf._split_tables(tables(o) if tab is None else tab, o)
    return o, g, u, rgb, a, b, ee


def messages(image, logits, options=None, tables=None):
    """(z^T float64 [K+1,H,W], Da float64 [H,W]): ``refine_labels`` before its rounding and its choice, and the appearance
    kernel's mass at every pixel."""
    o, g, u, rgb, ta, tb, ee = _operands(image, logits, options, tables)
    n_labels, h, w = u.shape
    r = o.radius
    z = u
    da = np.zeros((h, w), dtype=np.float64)
    for _ in range(o.iterations):
        q, _ = beliefs(z, ee)
        na, ns = (np.zeros((n_labels, h, w), dtype=np.float64) for _ in range(2))
        da, ds = (np.zeros((h, w), dtype=np.float64) for _ in range(2))
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
                da[here] = da[here] + a
                ds[here] = ds[here] + b
                for l in range(n_labels):
                    qj = q[l][there]
                    na[l][here] = na[l][here] + a * qj
                    ns[l][here] = ns[l][here] + b * qj
        with np.errstate(invalid="ignore", divide="ignore"):
            ma = np.where(da > 0.0, na / da, 0.0)
            ms = np.where(ds > 0.0, ns / ds, 0.0)
        z = (u + o.weight_appearance * ma) + o.weight_smooth * ms
    return z, da


def choose(z) -> np.ndarray:
    """z float64 [K+1,...] -> uint8 [...]: the label rule of the module's text."""
    z = np.asarray(z, dtype=np.float64)
    label = np.zeros(z.shape[1:], dtype=np.uint8)
    val = z[0]
    for k in range(1, z.shape[0]):
        take = np.where(label == 0, z[k] >= val, z[k] > val)
        label = np.where(take, np.uint8(k), label)
        val = np.where(take, z[k], val)
    return np.ascontiguousarray(label.astype(np.uint8))


def refine_labels(image, logits, options=None, tables=None):
    """(labels uint8 [H,W], scores float32 [K+1,H,W]) of one frame.  ``image``: the net's input float32 [3,H,W], or the frame
    uint8 [H,W,3]; ``logits``: K maps float32 [H,W]; ``tables``: what ``tables(options)`` returned (None: made here).
    Vectorised over the pixels, sequential over the offsets and the labels."""
    z, _ = messages(image, logits, options, tables)
    return choose(z), np.ascontiguousarray(z.astype(np.float32))


def refine_labels_loop(image, logits, options=None, tables=None):
    """``refine_labels`` as a plain loop over the pixels, the module's text line by line (Python floats are IEEE float64)."""
    o, g, u, rgb, ta, tb, ee = _operands(image, logits, options, tables)
    n_labels, h, w = u.shape
    r = o.radius
    g, rgb, ta, tb, ee = g.tolist(), rgb.tolist(), ta.tolist(), tb.tolist(), ee.tolist()
    wa, ws = float(o.weight_appearance), float(o.weight_smooth)
    u = [[[float(v) for v in row] for row in plane] for plane in u]

    def beliefs_of(zs):
        m = zs[0]
        for v in zs[1:]:
            m = v if v > m else m
        e = []
        for v in zs:
            d = min(m - v, EXP_LIMIT)
            p = d * EXP_PER_UNIT
            i = min(int(math.floor(p)), EXP_STEPS - 1)
            f = p - i
            e.append(ee[i] + f * (ee[i + 1] - ee[i]))
        s = 0.0
        for v in e:
            s = s + v
        return [v / s for v in e]

    z = u
    labels = range(n_labels)
    for _ in range(o.iterations):
        q = [[beliefs_of([z[l][y][x] for l in labels]) for x in range(w)] for y in range(h)]
        nxt = [[[0.0] * w for _ in range(h)] for _ in labels]
        for y in range(h):
            for x in range(w):
                da = ds = 0.0
                na, ns = [0.0] * n_labels, [0.0] * n_labels
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        yy, xx = y + dy, x + dx
                        if (dy == 0 and dx == 0) or yy < 0 or yy >= h or xx < 0 or xx >= w:
                            continue
                        a = ta[dy + r][dx + r] * ((rgb[abs(g[0][y][x] - g[0][yy][xx])] * rgb[abs(g[1][y][x] - g[1][yy][xx])])
                                                  * rgb[abs(g[2][y][x] - g[2][yy][xx])])
                        b = tb[dy + r][dx + r]
                        da = da + a
                        ds = ds + b
                        qj = q[yy][xx]
                        for l in labels:
                            na[l] = na[l] + a * qj[l]
                            ns[l] = ns[l] + b * qj[l]
                for l in labels:
                    ma = na[l] / da if da > 0.0 else 0.0
                    ms = ns[l] / ds if ds > 0.0 else 0.0
                    nxt[l][y][x] = (u[l][y][x] + wa * ma) + ws * ms
        z = nxt
    out = np.zeros((h, w), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            label, val = 0, z[0][y][x]
            for k in range(1, n_labels):
                v = z[k][y][x]
                if (v >= val) if label == 0 else (v > val):
                    label, val = k, v
            out[y, x] = label
    return out, np.ascontiguousarray(np.array(z, dtype=np.float64).reshape(n_labels, h, w).astype(np.float32))


def refine_labels_batch(images, logits, options=None, tables=None):
    """``refine_labels`` frame by frame: images float32 [N,3,H,W] and K logit maps float32 [N,1,H,W] -> (labels uint8 [N,H,W],
    scores float32 [N,K+1,H,W])."""
    images = np.asarray(images)
    maps = _logit_list(logits)
    if images.ndim != 4:
        raise ValueError("images [N,3,H,W], got %s" % (images.shape,))
    for x in maps:
        if x.ndim != 4 or x.shape[1] != 1 or x.shape[0] != images.shape[0]:
            raise ValueError("images [N,3,H,W] and every logit map [N,1,H,W], got %s and %s" % (images.shape, x.shape))
    o = check_options(options)
    tab = _tables(o) if tables is None else tables
    both = [refine_labels(images[k], [x[k, 0] for x in maps], o, tab) for k in range(images.shape[0])]
    return np.ascontiguousarray(np.stack([b[0] for b in both])), np.ascontiguousarray(np.stack([b[1] for b in both]))


_tables = tables  # under a name the ``tables=`` arguments above do not hide
