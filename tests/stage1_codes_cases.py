"""Host reference of the pool's WINNER CODES (fosvos_conv3x3_fwd_pool_codes, include/fosvos_hip.h) and the cases the
stage-1 tests share.

Definition.  MaxPool2d(2, 2, ceil_mode=True) windows of a post-ReLU map y[N, H, W, C]; the window's pixels are numbered
k = 2 dy + dx in scan order (0,0), (0,1), (1,0), (1,1).  The code of a window and channel is a one-hot nibble: bit k is set
iff pixel k is the FIRST maximum in scan order (a later pixel wins only with a strictly larger value; pixels outside the image
never win; pixel 0 is always inside) AND that maximum is > 0.  A zero nibble: the whole window is 0.

``codes`` is written from that text alone, on plain torch ops, and works on any device.  ``pack_words`` is the library's
memory layout: one int32 per pooled pixel and 8 channels, channel 8 g + 2 i + h at bit 4 i + 16 h (i = 0..3, h = 0, 1).
"""
import torch


def codes(y: torch.Tensor) -> torch.Tensor:
    """y: [N, H, W, C] (any float dtype, finite).  Returns the nibbles as uint8 [N, ceil(H/2), ceil(W/2), C]."""
    n, h, w, c = y.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    v = torch.full((n, 2 * oh, 2 * ow, c), float("-inf"), dtype=torch.float32, device=y.device)
    v[:, :h, :w] = y.float()
    px = [v[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]  # pixel k = 2 dy + dx of every window
    best, win = px[0].clone(), torch.zeros_like(px[0], dtype=torch.int64)
    for k in (1, 2, 3):
        later = px[k] > best  # strictly larger only
        best = torch.where(later, px[k], best)
        win = torch.where(later, torch.full_like(win, k), win)
    nib = torch.where(best > 0, torch.ones_like(win) << win, torch.zeros_like(win))
    return nib.to(torch.uint8)


def pack_words(nib: torch.Tensor) -> torch.Tensor:
    """uint8 nibbles [N, OH, OW, C] -> int32 words [N, OH, OW, C / 8] in the library's layout."""
    n, oh, ow, c = nib.shape
    assert c % 8 == 0
    v = nib.to(torch.int64).reshape(n, oh, ow, c // 8, 4, 2)  # [.., i, h]
    word = torch.zeros((n, oh, ow, c // 8), dtype=torch.int64, device=nib.device)
    for i in range(4):
        for hh in range(2):
            word |= v[..., i, hh] << (4 * i + 16 * hh)
    word = torch.where(word >= 1 << 31, word - (1 << 32), word)  # as the int32 bit pattern
    return word.to(torch.int32)


def unpack_words(words: torch.Tensor) -> torch.Tensor:
    """The inverse of pack_words."""
    n, oh, ow, g = words.shape
    u = words.to(torch.int64) & 0xFFFFFFFF
    out = torch.empty((n, oh, ow, g, 4, 2), dtype=torch.uint8, device=words.device)
    for i in range(4):
        for hh in range(2):
            out[..., i, hh] = ((u >> (4 * i + 16 * hh)) & 15).to(torch.uint8)
    return out.reshape(n, oh, ow, g * 8)


def route(nib: torch.Tensor, dy: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """The pool backward the codes stand for: dx[N, h, w, C] holds dy's own values where the pixel's bit is set, +0 elsewhere."""
    n, oh, ow, c = nib.shape
    full = torch.zeros((n, 2 * oh, 2 * ow, c), dtype=dy.dtype, device=dy.device)
    for k in range(4):
        full[:, (k >> 1)::2, (k & 1)::2] = torch.where(((nib >> k) & 1).bool(), dy, torch.zeros_like(dy))
    return full[:, :h, :w].contiguous()


def few_valued(shape, seed: int, levels: int = 4, zero_share: float = 0.4) -> torch.Tensor:
    """A non-negative bf16 map with few distinct values and many zeros: ties in most windows."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, levels, shape, generator=g).float() * 0.25
    v = torch.where(torch.rand(shape, generator=g) < zero_share, torch.zeros_like(v), v)
    return v.to(torch.bfloat16)


# forward op cases of the issue: (N, H, W).  (2,128,512): exactly 512 tiles of 8 x 32, all windows whole; (6,121,213): odd in
# both directions; (3,125,427): ragged tiles at the right and bottom
FWD_SHAPES = [(2, 128, 512), (6, 121, 213), (3, 125, 427)]
# backward op cases: (N, H, W, C)
BWD_SHAPES = [(3, 121, 213, 64), (1, 8, 32, 64), (2, 1, 1, 64)]
# the pass tests' frame: both forward chains of five frames get at least 512 tiles, H and W odd
PASS_SHAPE = (5, 125, 499)
