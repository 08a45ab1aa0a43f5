"""Input makers shared by test_mask_components_cpu.py and test_gpu_mask_components.py: logit maps whose masks are hard for a
connected-component labelling, and the geometry cases of the temporal gate.  numpy only; everything is deterministic."""
import numpy as np

FG, BG = np.float32(1.5), np.float32(-2.5)


def mask_logits(mask):
    """float32 logits whose mask (``>= 0``) is ``mask``."""
    return np.where(np.asarray(mask, dtype=bool), FG, BG).astype(np.float32)


def planted_logits(h, w, density, seed=0):
    """A random map with the given foreground density and NaN, +-0.0 and +-inf planted in it (as far as it has room)."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    x = rng.standard_normal((h, w)).astype(np.float32)
    x = np.where(rng.random((h, w)) < density, np.abs(x) + np.float32(0.01), -np.abs(x) - np.float32(0.01)).astype(np.float32)
    specials = [np.float32(np.nan), np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)]
    flat = x.ravel()
    if flat.size >= 2 * len(specials):
        at = rng.choice(flat.size, size=2 * len(specials), replace=False)
        for k, p in enumerate(at):
            flat[p] = specials[k % len(specials)]
        # a NaN with a payload and the sign bit set: it must pass bit for bit
        flat[at[0]:at[0] + 1].view(np.uint32)[0] = 0xffc12345
    return x


def serpentine(h, w):
    """One pixel wide, through the whole frame: full rows 0, 2, 4, ... joined at alternating ends."""
    m = np.zeros((h, w), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(h, w):
    """A one-pixel path from a corner inwards that turns right whenever going on would leave the frame or come within a pixel
    of an earlier arm."""
    m = np.zeros((h, w), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True

    def can_step(dy, dx):
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < h and 0 <= nx < w) or m[ny, nx]:
            return False
        return not (0 <= fy < h and 0 <= fx < w and m[fy, fx])

    for _ in range(h * w):
        if not can_step(dy, dx):
            dy, dx = dx, -dy
            if not can_step(dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = True
    return m


def checkerboard(h, w):
    """(x + y) even: one 8-connected component (all unions are diagonal), none 4-connected."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx) % 2 == 0


def diagonal_join(h, w, oy, ox, centre=None):
    """Two 3x3 blobs that touch only by the diagonal step (cy - 1, cx - 1) - (cy, cx), with (cy, cx) the centre (the
    frame's unless given) moved by (oy, ox)."""
    m = np.zeros((h, w), dtype=bool)
    cy, cx = centre if centre is not None else (h // 2, w // 2)
    cy, cx = cy + oy, cx + ox
    m[max(cy - 3, 0):cy, max(cx - 3, 0):cx] = True
    m[cy:cy + 3, cx:cx + 3] = True
    return m


def equal_blobs(h, w):
    """Two blobs of equal area (2x3 and 3x2) and a smaller one: ``largest`` must keep the first in raster order."""
    m = np.zeros((h, w), dtype=bool)
    if h < 9 or w < 12:
        return None
    m[h - 4:h - 2, 1:4] = True        # 6 pixels, later root
    m[1:4, w - 3:w - 1] = True        # 6 pixels, earlier root
    m[h // 2, w // 2] = True          # 1 pixel
    return m


def area_blobs(h, w, min_area):
    """A row blob of exactly ``min_area`` pixels and one of ``min_area - 1``."""
    if min_area < 2 or w < min_area + 2 or h < 4:
        return None
    m = np.zeros((h, w), dtype=bool)
    m[0, 1:1 + min_area] = True
    m[h - 1, 1:min_area] = True
    return m


def diagonal_offsets():
    """Every position relative to a 16-pixel grid."""
    return [(oy, ox) for oy in range(16) for ox in range(16)]


def mask_cases(h, w):
    """[(name, logits float32 [H,W])] of every case that fits a frame of this size."""
    cases = [('planted{:.2f}'.format(d), planted_logits(h, w, d)) for d in (0.2, 0.41, 0.7)]
    cases += [('serpentine', mask_logits(serpentine(h, w))), ('spiral', mask_logits(spiral(h, w))),
              ('checkerboard', mask_logits(checkerboard(h, w))),
              ('all_foreground', mask_logits(np.ones((h, w), bool))), ('all_background', mask_logits(np.zeros((h, w), bool)))]
    if h >= 8 and w >= 8:
        cases.append(('diagonal_centre', mask_logits(diagonal_join(h, w, 0, 0))))
        cases.append(('anti_diagonal_centre', mask_logits(diagonal_join(h, w, 0, 0)[:, ::-1])))
    for name, m in (('equal_blobs', equal_blobs(h, w)), ('area_blobs7', area_blobs(h, w, 7))):
        if m is not None:
            cases.append((name, mask_logits(m)))
    return cases


def diagonal_cases(h, w, centre=None):
    """[(name, logits)]: the diagonal step at every position relative to a 16-pixel grid around the frame centre (or
    ``centre``), both diagonals, so some placement straddles a corner of every tile whose sides divide 16; ``centre`` lets a
    test aim at the corner of a wider tile."""
    cy, cx = centre if centre is not None else (h // 2, w // 2)
    out = []
    for oy, ox in diagonal_offsets():
        out.append(('diag{:+d}{:+d}'.format(oy - 8, ox - 8), mask_logits(diagonal_join(h, w, oy - 8, ox - 8, (cy, cx)))))
        # mirrored about the centre column: the step (y - 1, x) - (y, x - 1)
        out.append(('anti{:+d}{:+d}'.format(oy - 8, ox - 8),
                    mask_logits(diagonal_join(h, w, oy - 8, ox - 8, (cy, w - cx))[:, ::-1])))
    return out


def half_width(r, dy):
    half = 0
    while (half + 1) ** 2 <= r * r - dy * dy:
        half += 1
    return half


def gate_cases(h=150, w=300):
    """The geometry of the gate: [(name, logits [H,W], seed uint8 [H,W], radius, near)] with one single-pixel blob, one far
    blob that never touches, and one seed pixel; ``near`` says whether the single-pixel blob lies inside the dilated seed.
    The blob sits in column 63 or 62 so that seed and blob are in different 64-pixel words, and the diagonal cases put them
    in different tile rows."""
    out = []
    for r in (0, 1, 5, 63):
        dy_diag = {0: 0, 1: 1, 5: 3, 63: 38}[r]
        for name, dy in (('horizontal', 0), ('diagonal', dy_diag)):
            dx_in = half_width(r, dy)
            for inside, dx in ((True, dx_in), (False, dx_in + 1)):
                for direction in (1, -1):  # the seed right and below of the blob, and left and above
                    by, bx = (20, 63) if direction == 1 else (20 + dy, 63 + dx)
                    sy, sx = by + direction * dy, bx + direction * dx
                    m = np.zeros((h, w), dtype=bool)
                    m[by, bx] = True
                    m[h - 6:h - 2, w - 9:w - 3] = True   # far from every seed used here
                    seed = np.zeros((h, w), dtype=np.uint8)
                    seed[sy, sx] = 255 if inside else 1
                    out.append(('r{}_{}_{}_{}'.format(r, name, 'in' if inside else 'out', 'fwd' if direction == 1 else 'back'),
                                mask_logits(m), seed, r, inside))
    return out


def seed_for(logits):
    """A seed for a general map: the top-left quarter of its mask (so some components touch it and some do not)."""
    with np.errstate(invalid='ignore'):
        m = logits >= 0
    seed = np.zeros(m.shape, dtype=np.uint8)
    h, w = m.shape
    seed[:(h + 1) // 2, :(w + 1) // 2] = m[:(h + 1) // 2, :(w + 1) // 2] * 7
    return seed
