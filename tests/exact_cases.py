"""Exactly summable operands for the contraction kernels of the VGG path: case tables, operand generators, the bound that
makes each case exact, and the references in torch on the CPU.  Shared by tests/test_exact_cases_cpu.py (the reference alone)
and tests/test_gpu_exact.py (the kernels against it, by equality).  Nothing here touches the device.

The argument.  Every operand is an integer (or a dyadic rational with a common unit ``lsb``) that the kernel's input format
holds exactly.  A product of two such values is a multiple of lsb, and so is every partial sum, in any order and any
grouping; its magnitude is at most  terms x max|a| x max|b| (+ max|bias|).  While that is below 2^24 lsb every partial sum
is an fp32 number, so an fp32 accumulation is exact whatever its order: the tile, the K split, the persistent or the igemm
kernel, a fold or a slab reduction cannot change the result, and the result is the integer the CPU computes (fp32 and fp64
agree bit for bit).  A bf16 output is then the round-to-nearest-even image of that integer, and every comparison is
``torch.equal``.  The bound is computed from the DECLARED operand ranges, never from drawn values.

Class names follow tests/test_gpu_layer_parity.py: "pp<=64" / "pp-reload" for the persistent forward kernel by K-chunk
regime, else "<tile_h>x<tile_w>x<tile_co>/k<K splits>" of the igemm."""
import torch
import torch.nn.functional as F

LIMIT = 2 ** 24


# ------------------------------------------------------------------------------------------ number formats
def bf(t):
    """Round to bf16 (nearest, ties to even), fp32 container."""
    return t.to(torch.bfloat16).float()


def _bits(t):
    return t.contiguous().view(torch.int32)


def bf16_trunc(t):
    """What a truncating fp32 -> bf16 convert gives (fp32 container)."""
    return (_bits(t) & -65536).view(torch.float32)


def bf16_half_away(t):
    """What round-half-away-from-zero gives (the bias 0x8000 added to the magnitude, then truncated)."""
    b = _bits(t)
    mag = ((b & 0x7FFFFFFF) + 0x8000) & -65536
    return (mag | (b & -2147483648)).view(torch.float32)


def is_tie(t):
    """Exactly half way between two bf16 numbers."""
    return (_bits(t) & 0xFFFF) == 0x8000


def rounding_shares(pre):
    """Shares of the fp32 values ``pre`` that: need rounding to bf16, are exact ties, round differently under truncation,
    round differently under half-away."""
    r = bf(pre)
    n = float(pre.numel())
    return {"rounded": float((r != pre).sum()) / n, "ties": float(is_tie(pre).sum()) / n,
            "trunc": float((r != bf16_trunc(pre)).sum()) / n, "away": float((r != bf16_half_away(pre)).sum()) / n}


def compare_bits(got, want, pre=None):
    """None if ``got`` equals ``want`` bit for bit (shape, dtype, every element; +0 and -0 are told apart), else one line:
    how many elements differ, the first differing index, the two values, and - where ``pre``, the exact fp32 value in front
    of the final bf16 rounding, is given - whether the kernel's values are the truncated or the half-away image of it."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape/dtype {tuple(got.shape)} {got.dtype} != {tuple(want.shape)} {want.dtype}"
    g, w = got.float().contiguous(), want.float().contiguous()
    bad = _bits(g) != _bits(w)
    n_bad = int(bad.sum())
    if n_bad == 0:
        return None
    idx = tuple(int(i) for i in bad.nonzero()[0])
    msg = f"{n_bad} / {bad.numel()} elements differ; first at {idx}: kernel {g[idx].item()!r}, reference {w[idx].item()!r}"
    if pre is not None:
        p = pre.float().contiguous()
        tr, aw = bf16_trunc(p), bf16_half_away(p)
        msg += (f" (exact value {p[idx].item()!r}; kernel == truncation there: {bool(g[idx] == tr[idx])}, == half-away: "
                f"{bool(g[idx] == aw[idx])}; of the differing elements {int((g[bad] == tr[bad]).sum())} equal the truncated and "
                f"{int((g[bad] == aw[bad]).sum())} the half-away rounding)")
    return msg


# ------------------------------------------------------------------------------------------ operand generators
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, amax):
    """Uniform integers in [-amax, amax] as fp32."""
    return torch.randint(-amax, amax + 1, shape, generator=g).float()


def survives_bf16(t):
    return torch.equal(bf(t), t)


class Case:
    """One row of a table: ``id``, ``shape``, the launch class ``cls`` it is listed for, and the declared operand ranges."""

    def __init__(self, id, shape, cls, seed, **ranges):
        self.id, self.shape, self.cls, self.seed = id, shape, cls, seed
        self.__dict__.update(ranges)

    def __repr__(self):
        return self.id


def cls_name(plan, contraction):
    if plan["persistent"]:
        return "pp<=64" if contraction <= 64 else "pp-reload"
    return "%dx%dx%d/k%d" % (*plan["tile"], plan["k_splits"])


# ------------------------------------------------------------------------------------------ forward
# shape = n, h, w, ci, co.  x in [-xmax, xmax], w in [-wmax, wmax], bias in [-bmax, bmax], all integers.  Every map has ragged
# right and bottom edges for its tile.  co == 16: the fp32-output side form.
FWD_CASES = [
    Case("mid_k1", (1, 61, 107, 64, 512), "8x16x64/k1", 1001, xmax=8, wmax=4, bmax=64),
    Case("mid_k3", (1, 15, 27, 96, 64), "8x16x64/k3", 1002, xmax=8, wmax=4, bmax=64),
    Case("mid_k16", (1, 15, 27, 512, 64), "8x16x64/k16", 1003, xmax=8, wmax=4, bmax=64),
    Case("big_k1", (1, 47, 250, 64, 512), "8x32x64/k1", 1004, xmax=8, wmax=4, bmax=64),
    Case("square_k1", (1, 47, 240, 64, 512), "16x16x64/k1", 1005, xmax=8, wmax=4, bmax=64),
    Case("pp_resident", (1, 61, 250, 64, 512), "pp<=64", 1006, xmax=8, wmax=4, bmax=64),
    Case("pp_reload3", (1, 61, 250, 96, 512), "pp-reload", 1007, xmax=8, wmax=4, bmax=64),
    Case("side_small_k8", (1, 15, 27, 256, 16), "4x16x16/k8", 1008, xmax=8, wmax=4, bmax=64),
    Case("side_large", (1, 240, 274, 128, 16), "8x32x16/k1", 1009, xmax=8, wmax=4, bmax=64),
]
FWD_CLASSES = {"8x16x64/k1", "8x16x64/k3", "8x16x64/k16", "8x32x64/k1", "16x16x64/k1", "pp<=64", "pp-reload",
               "4x16x16/k8", "8x32x16/k1"}


def fwd_bound(c):
    n, h, w, ci, co = c.shape
    return 9 * ci * c.xmax * c.wmax + c.bmax


def fwd_class(ops, c):
    n, h, w, ci, co = c.shape
    plan = ops.conv3x3_plan(n, h, w, ci, co) if co == 16 else ops.conv3x3_fwd_plan(n, h, w, ci, co)
    return cls_name(plan, ci)


def fwd_operands(c):
    n, h, w, ci, co = c.shape
    g = _gen(c.seed)
    return ints(g, (n, ci, h, w), c.xmax), ints(g, (co, ci, 3, 3), c.wmax), ints(g, (co,), c.bmax)


def fwd_reference(x, w, b, dtype=torch.float32):
    """The exact fp32 values in front of the output conversion: {"linear": conv(x, w), "bias": conv + b, "relu": relu(conv +
    b)} (NCHW).  The bf16 outputs are bf() of these, the pooled maps ``pool()`` of the bf16 outputs."""
    s = F.conv2d(x.to(dtype), w.to(dtype), None, padding=1)
    sb = s + b.to(dtype).view(1, -1, 1, 1)
    return {"linear": s, "bias": sb, "relu": torch.relu(sb)}


def pool(y):
    return F.max_pool2d(y, 2, 2, ceil_mode=True)


# ------------------------------------------------------------------------------------------ data gradient
# shape = n, h, w, ci, co of the forward op: dx has ci channels, the contraction runs over co (the plan is queried with the
# channel roles swapped).  dy in [-ymax, ymax], w in [-wmax, wmax], the addend (or the pooled gradient) in [-amax, amax],
# the ReLU source relu(integers in [-smin, smax]).  kind: "plain" (conv3x3_dgrad: plain, relu_src, relu_bits, addend aliased
# to out, mask and addend together; co == 16: the side form, 16 real channels in a 32-wide gradient image), "unpool"
# (conv3x3_dgrad_unpool).  bits_cls: the class fosvos_conv3x3_dgrad_bits takes without an addend, where it is another.
DGRAD_CASES = [
    Case("mid_k1_fused", (1, 61, 107, 512, 64), "8x16x64/k1", 2001, kind="plain", ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("mid_k3", (1, 15, 27, 64, 96), "8x16x64/k3", 2002, kind="plain", ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("mid_k16_splitk", (1, 15, 27, 64, 512), "8x16x64/k16", 2003, kind="plain", ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("big_k1", (1, 47, 250, 512, 64), "8x32x64/k1", 2004, kind="plain", ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("square_k1", (1, 47, 240, 512, 64), "16x16x64/k1", 2005, kind="plain", ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("bits_pp_resident", (1, 61, 250, 512, 64), "8x32x64/k1", 2006, kind="plain", bits_cls="pp<=64",
         ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("bits_pp_reload3", (1, 61, 250, 512, 96), "8x32x64/k1", 2007, kind="plain", bits_cls="pp-reload",
         ymax=8, wmax=4, amax=255, smin=2, smax=4),
    Case("side", (1, 30, 54, 128, 16), "8x16x64/k1", 2008, kind="plain", ymax=8, wmax=16, amax=255, smin=2, smax=4),
    Case("unpool_big", (1, 47, 250, 512, 16), "8x32x64/k1", 2009, kind="unpool", ymax=8, wmax=16, amax=255, smin=2, smax=4),
    Case("unpool_square", (1, 47, 240, 512, 16), "16x16x64/k1", 2010, kind="unpool", ymax=8, wmax=16, amax=255, smin=2, smax=4),
    Case("unpool_mid", (2, 61, 107, 64, 16), "8x16x64/k1", 2011, kind="unpool", ymax=8, wmax=16, amax=255, smin=2, smax=4),
    Case("unpool_two_pass_32ch", (2, 61, 107, 32, 16), "4x16x32/k1", 2012, kind="unpool", ymax=8, wmax=16, amax=255, smin=2, smax=4),
]
DGRAD_CLASSES = {"8x16x64/k1", "8x16x64/k3", "8x16x64/k16", "8x32x64/k1", "16x16x64/k1", "pp<=64", "pp-reload"}
UNPOOL_CLASSES = {"8x32x64/k1", "16x16x64/k1", "8x16x64/k1", "4x16x32/k1"}


def dgrad_bound(c):
    n, h, w, ci, co = c.shape
    return 9 * co * c.ymax * c.wmax + c.amax


def dgrad_class(ops, c):
    n, h, w, ci, co = c.shape
    return cls_name(ops.conv3x3_plan(n, h, w, co, ci), co)


def dgrad_bits_class(ops, c):
    """What fosvos_conv3x3_dgrad_bits launches without an addend: the persistent kernel where a forward conv of the swapped
    shape would take it, else the igemm class."""
    n, h, w, ci, co = c.shape
    pp = ops.conv3x3_fwd_plan(n, h, w, co, ci, relu=False)
    return cls_name(pp, co) if pp["persistent"] else dgrad_class(ops, c)


def dgrad_operands(c):
    """dy [n,co,h,w], w [co,ci,3,3], src [n,ci,h,w] >= 0 (the producer's post-ReLU output: mask and pool input), addend
    [n,ci,h,w] ("plain") or the pooled gradient [n,ci,ceil(h/2),ceil(w/2)] ("unpool")."""
    n, h, w, ci, co = c.shape
    g = _gen(c.seed)
    dy, wt = ints(g, (n, co, h, w), c.ymax), ints(g, (co, ci, 3, 3), c.wmax)
    src = torch.relu(torch.randint(-c.smin, c.smax + 1, (n, ci, h, w), generator=g).float())
    a_shape = (n, ci, h, w) if c.kind == "plain" else (n, ci, (h + 1) // 2, (w + 1) // 2)
    return dy, wt, src, ints(g, a_shape, c.amax)


def dgrad_sum(dy, w, dtype=torch.float32):
    """The exact data gradient dx[n,ci,y,x] = sum_{co,ky,kx} dy[n,co,y+1-ky,x+1-kx] w[co,ci,ky,kx]."""
    return F.conv_transpose2d(dy.to(dtype), w.to(dtype), None, padding=1)


def dgrad_epilogue(s, mask=None, addend=None):
    """The documented sequence (k_splitk_epilogue, the fused epilogue): t = bf16(s); t = mask ? t : 0; t = t + addend in
    fp32; y = bf16(t).  Returns (y, the exact fp32 value in front of the LAST rounding)."""
    if mask is None and addend is None:
        return bf(s), s
    t = bf(s)
    if mask is not None:
        t = torch.where(mask, t, torch.zeros_like(t))
    if addend is not None:
        t = t + addend
    return bf(t), t


def pool_windows(x):
    """[n,c,oh,ow,4] windows of the 2x2 ceil-mode pool in scan order (missing pixels of a ragged window: -inf)."""
    n, c, h, w = x.shape
    xp = F.pad(x, [0, w % 2, 0, h % 2], value=float("-inf"))
    return xp.reshape(n, c, (h + 1) // 2, 2, (w + 1) // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, (h + 1) // 2, (w + 1) // 2, 4)


def pool_backward(x, d_pooled, relu_mask=True):
    """Exactly routed pool gradient: each window's gradient goes to its FIRST maximum in scan order, and (relu_mask) only
    where that maximum is > 0 (the ReLU mask of the producer)."""
    n, c, h, w = x.shape
    win = pool_windows(x)
    is_max = win == win.max(-1, keepdim=True).values
    first = is_max & (is_max.int().cumsum(-1) == 1)
    if relu_mask:
        first = first & (win > 0)
    r = torch.where(first, d_pooled.unsqueeze(-1).expand_as(win), torch.zeros_like(win))  # (+0 elsewhere, not -0)
    oh, ow = (h + 1) // 2, (w + 1) // 2
    r = r.reshape(n, c, oh, ow, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * oh, 2 * ow)
    return r[:, :, :h, :w].contiguous()


def tied_window_share(x):
    """Share of the pooling windows whose (positive) maximum is attained more than once."""
    win = pool_windows(x)
    m = win.max(-1, keepdim=True).values
    tied = ((win == m).sum(-1) > 1) & (m.squeeze(-1) > 0)
    return float(tied.sum()) / tied.numel()


def relu_bits(src_nhwc):
    """[N,H,W,C] -> uint8 [N,H,W,C/8]: bit e of byte g = (src[..., 8 g + e] > 0)."""
    n, h, w, c = src_nhwc.shape
    pos = (src_nhwc.float() > 0).reshape(n, h, w, c // 8, 8).to(torch.int32)
    return (pos << torch.arange(8, dtype=torch.int32, device=src_nhwc.device)).sum(-1).to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------------ weight and bias gradient
# shape = n, h, w, ci, co.  x and dy in [-8, 8]; the prefill of the accumulate form in [-pmax, pmax].  terms = n h w.
WGRAD_CASES = [
    Case("fold_two_co_blocks", (1, 61, 107, 64, 128), "56 splits, fold stage, two co blocks", 3001, xmax=8, ymax=8, pmax=1000),
    Case("reduce_loop_105", (1, 120, 214, 64, 64), "105 splits: more than 8 folded slabs", 3002, xmax=8, ymax=8, pmax=1000),
    Case("split_crosses_image", (2, 30, 54, 512, 512), "3 splits of 11 tiles across the image boundary", 3003,
         xmax=8, ymax=8, pmax=1000),
    Case("side_form", (2, 33, 47, 128, 16), "side form, 30 splits", 3004, xmax=8, ymax=8, pmax=1000),
    Case("one_small_tile", (1, 7, 5, 64, 64), "one tile, smaller than the tile", 3005, xmax=8, ymax=8, pmax=1000),
]


def wgrad_bound(c):
    n, h, w, ci, co = c.shape
    return n * h * w * c.xmax * c.ymax + c.pmax


def wgrad_operands(c):
    n, h, w, ci, co = c.shape
    g = _gen(c.seed)
    return (ints(g, (n, ci, h, w), c.xmax), ints(g, (n, co, h, w), c.ymax), ints(g, (co, ci, 3, 3), c.pmax),
            ints(g, (co,), c.pmax))


def wgrad_reference(x, dy, dtype=torch.float32):
    """(dw [co,ci,3,3], db [co]): the exact integers, dw[co,ci,ky,kx] = sum_{n,y,x} dy[n,co,y,x] x[n,ci,y+ky-1,x+kx-1]."""
    co, ci = dy.shape[1], x.shape[1]
    wt = torch.zeros(co, ci, 3, 3, dtype=dtype, requires_grad=True)
    b = torch.zeros(co, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), wt, b, padding=1).backward(dy.to(dtype))
    return wt.grad, b.grad


# ------------------------------------------------------------------------------------------ conv1_1
# Forward, two operand sets per shape; frame = xk / xdiv with integer |xk| <= xkmax, weights = k / wdiv with |k| <= kmax, integer
# bias, lsb = 1 / (xdiv wdiv):
#   "split": half-integers in [-255, 255] (up to 9 significant bits) and weights k / 256 with |k| <= 1023.  Both operands have
#            a non-zero low bf16 term (an INTEGER up to 255 would have none: it has 8 significant bits), so all four term
#            products of the kernel's hi/lo split contribute, and each is exact.  Nearly every output needs rounding and half
#            of them differ under truncation, but with 27 terms of unit 2^-9 an exact tie is rare.
#   "ties":  small integers, sums of a few hundred: the ties that tell round-to-nearest-even from half-away.
FIRST_FWD_CASES = [
    Case("first_2x61x107_split", (2, 61, 107), "conv1_1 forward", 4001, kind="split", xkmax=510, xdiv=2, kmax=1023, wdiv=256, bmax=8),
    Case("first_2x61x107_ties", (2, 61, 107), "conv1_1 forward", 4005, kind="ties", xkmax=32, xdiv=1, kmax=4, wdiv=1, bmax=8),
    Case("first_1x9x130_split", (1, 9, 130), "conv1_1 forward", 4002, kind="split", xkmax=510, xdiv=2, kmax=1023, wdiv=256, bmax=8),
    Case("first_1x9x130_ties", (1, 9, 130), "conv1_1 forward", 4006, kind="ties", xkmax=32, xdiv=1, kmax=4, wdiv=1, bmax=8),
]
# Weight gradient: the kernel rounds the fp32 frame to bf16 itself.  "rounded_frame": integers up to 1023, most of them with
# more than 8 significant bits, ties among them; "many_tiles": more than 512 tiles of 8 x 16 (tiles_per_split = 2, and with
# chunks of 4 tiles half of the workgroups own none), a bf16-exact frame and dy in {-1, 0, 1}.
FIRST_WGRAD_CASES = [
    Case("first_wgrad_rounded_frame", (2, 33, 47), "in-kernel rounding, partial last chunk", 4003, xmax=1023, ymax=4),
    Case("first_wgrad_many_tiles", (3, 121, 213), "tiles_per_split 2, idle workgroups", 4004, xmax=128, ymax=1),
]


def first_fwd_bound(c):
    """In units of lsb = 1 / (xdiv wdiv): 27 products of |xk| <= xkmax and |k| <= kmax, the bias in whole units."""
    return 27 * c.xkmax * c.kmax + c.bmax * c.xdiv * c.wdiv


def first_fwd_operands(c):
    n, h, w = c.shape
    g = _gen(c.seed)
    return ints(g, (n, 3, h, w), c.xkmax) / c.xdiv, ints(g, (64, 3, 3, 3), c.kmax) / c.wdiv, ints(g, (64,), c.bmax)


def first_fwd_reference(frame, w, b, dtype=torch.float32):
    """relu(conv(frame, w) + b) on the fp32 operands, exact; the kernel's output is bf() of it, its bits (that > 0)."""
    return torch.relu(F.conv2d(frame.to(dtype), w.to(dtype), b.to(dtype), padding=1))


def first_wgrad_bound(c):
    n, h, w = c.shape
    x_bf = int(bf(torch.tensor(float(c.xmax))))  # rounding is monotone: |bf16(x)| <= bf16(xmax) (1024 for xmax = 1023)
    return n * h * w * x_bf * c.ymax


def first_wgrad_operands(c):
    n, h, w = c.shape
    g = _gen(c.seed)
    return ints(g, (n, 3, h, w), c.xmax), ints(g, (n, 64, h, w), c.ymax)


def first_wgrad_reference(frame, dy, dtype=torch.float32):
    """Exact weight and bias gradient on bf16(frame)."""
    return wgrad_reference(bf(frame), dy, dtype)


def significant_bits_over_8_share(frame):
    return float((bf(frame) != frame).sum()) / frame.numel()
