"""The VGG head kernels (csrc/head.hip: k_head_fwd<WITH_SIDE_OUT>, k_head_bwd_scale<S, WITH_SIDE_OUT, UNIFORM>, k_head_finish)
at the frame sizes where their tiles split, for all 18 instances: every (side outputs, uniform filters) combination of the
two forward and sixteen backward kernels, against ``_head_ref`` in float64 on the CPU (autograd for the backward).

The op tests of tests/test_gpu_ops.py run W <= 107 and N <= 3: no third forward column tile, no second scale-3 column block,
no last block of one row or column and never more than 16 slabs per scale.  SHAPES below are chosen by tile arithmetic for
those features, and test_tile_table_and_shape_features (no GPU) restates the tile table and asserts that each shape still
has the features it is listed for, and that the library's workspace size agrees with the restated slab counts: whoever
changes a tile is told there to derive the shapes again.

Bounds, all from tests/test_gpu_ops.py and tests/test_gpu_layer_parity.py (none is set from what these kernels give):
  * fused and side outputs against the reference: rel-to-max 1e-5
  * d_fuse_w, d_fuse_b, d_dsn_w[s], d_dsn_b[s] against the reference: rel-to-max 2e-5
  * d_side[..., :16]: assert_bf16_close;  d_side[..., 16:]: exactly zero
  * uniform kernels against the general ones on the same inputs: forward 2e-6, d_side 4e-3, parameter gradients 1e-5
Every case prints one line: the worst error of each family of checks in units of its bound (1.0 = on the bar).
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import osvos_ref as O
from test_gpu_layer_parity import Margins
from test_gpu_ops import _head_inputs, _head_ref, assert_bf16_close, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

DEV = "cuda:0"

# ------------------------------------------------------------------------------------------ the tile table, restated
TI = (8, 4, 4, 2)        # HeadTile<S>::TI: low-res rows of a backward workgroup
TJ = (32, 16, 4, 8)      # HeadTile<S>::TJ: low-res columns
HF_TY, HF_TX = 16, 64    # output pixels of a forward workgroup
GROUPS, IN_FLIGHT = 16, 8  # k_head_finish: row groups, slabs in flight per thread (one b0 iteration takes GROUPS * IN_FLIGHT)
BIAS_FLOATS = 512        # kBiasBlocks

# id -> (N, H, W, side map sizing).  "ceil": what four ceil-mode pools give; "floor": H >> (s + 1), the smallest maps
# make_geom takes here ((hs + 1) * f >= H), with crop offsets top[0] = left[0] = 0.
SHAPES = {
    "1x33x129": (1, 33, 129, "ceil"),
    "2x32x128": (2, 32, 128, "ceil"),
    "15x40x129": (15, 40, 129, "ceil"),
    "1x1x1": (1, 1, 1, "ceil"),
    "2x1x70": (2, 1, 70, "ceil"),
    "1x5x3": (1, 5, 3, "ceil"),
    "1x33x129-floor": (1, 33, 129, "floor"),
}
# seeds of the inputs; chosen on the CPU so that no bias sum of the reference is a cancellation (see `reference`)
SEEDS = {"1x33x129": 810, "2x32x128": 811, "15x40x129": 812, "1x1x1": 813, "2x1x70": 814, "1x5x3": 815, "1x33x129-floor": 816}

MASKS = (0b0000, 0b1111)
MIXED_MASKS = (0b0110, 0b1001)


def cdiv(a, b):
    return -(-a // b)


def side_sizes(H, W, sizing):
    if sizing == "floor":
        return [(H >> (s + 1), W >> (s + 1)) for s in range(4)]
    out, h, w = [], H, W
    for _ in range(4):
        h, w = (h + 1) // 2, (w + 1) // 2
        out.append((h, w))
    return out


def bwd_blocks(H, W, sizing):
    """(row blocks, column blocks) of k_head_bwd_scale per scale."""
    return [(cdiv(h, TI[s]), cdiv(w, TJ[s])) for s, (h, w) in enumerate(side_sizes(H, W, sizing))]


def slabs(N, H, W, sizing):
    return [N * r * c for r, c in bwd_blocks(H, W, sizing)]


def crop_offsets(H, W, sizing):
    return [(((h + 1) * (2 << s) - H) // 2, ((w + 1) * (2 << s) - W) // 2) for s, (h, w) in enumerate(side_sizes(H, W, sizing))]


def test_tile_table_and_shape_features():
    """No GPU.  The features SHAPES is there for, from the restated tile table; and the library's own slab arithmetic
    (fosvos_head_bwd_workspace_bytes) against the restatement.  If this fails after a tile change, derive the shapes of this
    file again from the new tiles: the GPU cases below no longer sit on the boundaries they claim."""
    from fosvos_hip import lib
    L = lib()
    for n, H, W, _ in SHAPES.values():  # the workspace is sized for the ceil-pooled maps, whatever the caller's are
        assert L.fosvos_head_bwd_workspace_bytes(n, H, W) == 4 * (48 * sum(slabs(n, H, W, "ceil")) + BIAS_FLOATS), (n, H, W)

    # 1x33x129: >= 2 blocks each way at every scale, each last block (and the last forward tile) one row and one column
    n, H, W, sizing = SHAPES["1x33x129"]
    assert bwd_blocks(H, W, sizing) == [(3, 3), (3, 3), (2, 5), (2, 2)]
    for s, (h, w) in enumerate(side_sizes(H, W, sizing)):
        assert h % TI[s] == 1 and w % TJ[s] == 1, s
    assert (cdiv(H, HF_TY), cdiv(W, HF_TX)) == (3, 3) and H % HF_TY == 1 and W % HF_TX == 1
    assert slabs(n, H, W, sizing) == [9, 9, 10, 4] and slabs(n, H, W, sizing)[3] < GROUPS

    # 2x32x128: everything divides
    n, H, W, sizing = SHAPES["2x32x128"]
    assert side_sizes(H, W, sizing) == [(16, 64), (8, 32), (4, 16), (2, 8)]
    for s, (h, w) in enumerate(side_sizes(H, W, sizing)):
        assert h % TI[s] == 0 and w % TJ[s] == 0, s
    assert H % HF_TY == 0 and W % HF_TX == 0 and n == 2

    # 15x40x129: a second b0 iteration (> 128 slabs), several slabs per group (> 16), a partial last group of eight
    n, H, W, sizing = SHAPES["15x40x129"]
    got = slabs(n, H, W, sizing)
    assert got == [135, 135, 150, 60]
    assert [g > GROUPS * IN_FLIGHT for g in got] == [True, True, True, False] and all(g > GROUPS for g in got)
    assert all(cdiv(g, GROUPS) % IN_FLIGHT != 0 for g in got)
    assert all(t != l for t, l in crop_offsets(H, W, sizing)[1:])

    # degenerate maps
    n, H, W, sizing = SHAPES["1x1x1"]
    assert side_sizes(H, W, sizing) == [(1, 1)] * 4
    n, H, W, sizing = SHAPES["2x1x70"]
    assert H == 1 and cdiv(W, HF_TX) == 2 and all(h == 1 for h, _ in side_sizes(H, W, sizing))
    n, H, W, sizing = SHAPES["1x5x3"]
    assert all(W < (2 << s) for s in (1, 2, 3)) and slabs(n, H, W, sizing) == [1, 1, 1, 1]

    # 1x33x129 with floor-sized maps: each still covers the frame, with nothing cropped before the first row and column
    n, H, W, sizing = SHAPES["1x33x129-floor"]
    assert side_sizes(H, W, sizing) == [(16, 64), (8, 32), (4, 16), (2, 8)]
    for s, (h, w) in enumerate(side_sizes(H, W, sizing)):
        assert (h + 1) * (2 << s) >= H and (w + 1) * (2 << s) >= W
        assert h < side_sizes(H, W, "ceil")[s][0] and w < side_sizes(H, W, "ceil")[s][1]
    assert crop_offsets(H, W, sizing)[0] == (0, 0)


# ------------------------------------------------------------------------------------------ inputs and the fp64 reference
def _not_a_cancellation(what, terms, total):
    """A bias gradient is one long sum.  Where its terms cancel, rel-to-max of the SUM measures the summation order of
    whoever computes it: the inputs are drawn (upstream gradients randn + 0.5) so that they do not."""
    assert abs(float(terms.sum()) - float(total)) <= 1e-9 * float(terms.abs().sum()), what
    assert abs(float(total)) >= 0.25 * float(terms.abs().sum()), f"{what}: the sum cancels; pick another seed"


@functools.lru_cache(maxsize=None)
def reference(shape_id, mask):
    """Inputs (fp32, host) of one shape and filter mask, and the float64 reference: the five outputs and the gradients for
    all five upstream gradients ("all"), the fused one only ("fused") and the four side outputs only ("side").  Computed
    once per (shape, mask) and shared; nobody writes to it."""
    n, H, W, sizing = SHAPES[shape_id]
    side, up, up1, dsn_w, dsn_b, fuse_w, fuse_b = _head_inputs(n, H, W, seed=SEEDS[shape_id])
    side = [s[:, :, :h, :w].contiguous() for s, (h, w) in zip(side, side_sizes(H, W, sizing))]
    for i in range(4):
        if (mask >> i) & 1:  # channel 3's filter (noise and all) on the whole diagonal, as test_head_channel_uniform_filters
            same = up[i][3, 3].clone()
            for c in range(16):
                up[i][c, c] = same
    gen = torch.Generator().manual_seed(SEEDS[shape_id] + 1000)
    g = [torch.randn(n, 1, H, W, generator=gen) + 0.5 for _ in range(5)]

    leaves = [s.double().requires_grad_(True) for s in side]
    dw_l, db_l = dsn_w.double().requires_grad_(True), dsn_b.double().requires_grad_(True)
    fw_l, fb_l = fuse_w.double().requires_grad_(True), fuse_b.double().requires_grad_(True)
    up64, up164, g64 = [u.double() for u in up], [u.double() for u in up1], [t.double() for t in g]
    ref = _head_ref(leaves, up64, up164, dw_l, db_l, fw_l, fb_l, H, W)
    ga = torch.autograd.grad(ref, leaves + [fw_l, fb_l, dw_l, db_l], g64, retain_graph=True)
    gf = torch.autograd.grad([ref[4]], leaves + [fw_l, fb_l], [g64[4]], retain_graph=True)
    gs = torch.autograd.grad(ref[:4], leaves + [dw_l, db_l], g64[:4])

    _not_a_cancellation("d_fuse_b", g64[4], ga[5])
    for i in range(4):  # d_dsn_b[i] is the sum of the score map's gradient: the upstream gradient through upscale_[i] and crop
        z = torch.zeros(n, 1, *side[i].shape[2:], dtype=torch.float64, requires_grad=True)
        O.center_crop(F.conv_transpose2d(z, up164[i], stride=2 << i), H, W).backward(g64[i])
        _not_a_cancellation(f"d_dsn_b[{i}]", z.grad, ga[7][i])
    grads = {"all": dict(side=ga[:4], fw=ga[4], fb=ga[5], dw=ga[6], db=ga[7]),
             "fused": dict(side=gf[:4], fw=gf[4], fb=gf[5]),
             "side": dict(side=gs[:4], dw=gs[4], db=gs[5])}
    return dict(n=n, H=H, W=W, side=side, up=up, up1=up1, dsn_w=dsn_w, dsn_b=dsn_b, fuse_w=fuse_w, fuse_b=fuse_b, g=g,
                out=[r.detach() for r in ref], grads=grads)


def test_reference_bias_sums_do_not_cancel():
    """No GPU: the condition on the inputs (asserted inside ``reference``) holds for every case the GPU tests run."""
    for shape_id in SHAPES:
        for mask in MASKS + (MIXED_MASKS if shape_id == "1x33x129" else ()):
            reference(shape_id, mask)


# ------------------------------------------------------------------------------------------ device side
@pytest.fixture(scope="module")
def ops():
    from fosvos_hip import ops as _ops
    return _ops


def device_inputs(c):
    dev = lambda t: t.contiguous().to(DEV)
    idx = torch.arange(16)
    return dict(side=[dev(s.permute(0, 2, 3, 1)) for s in c["side"]],             # fp32 NHWC
                filt=[dev(u[idx, idx].permute(1, 2, 0)) for u in c["up"]],       # [k,k,16], channel fastest
                filt1=[dev(u[0, 0]) for u in c["up1"]], dsn_w=dev(c["dsn_w"]), dsn_b=dev(c["dsn_b"]),
                fuse_w=dev(c["fuse_w"]), fuse_b=dev(c["fuse_b"]), g=[dev(t) for t in c["g"]])


def run_fwd(ops, c, d, with_so, mask):
    if with_so:
        return ops.head_fwd(d["side"], d["filt"], d["filt1"], d["dsn_w"], d["dsn_b"], d["fuse_w"], d["fuse_b"], c["H"], c["W"],
                            True, filt_uniform=mask)
    return ops.head_fwd(d["side"], d["filt"], None, None, None, d["fuse_w"], d["fuse_b"], c["H"], c["W"], False,
                        filt_uniform=mask)


def run_bwd(ops, c, d, which, mask):
    """which: "all" (five upstream gradients), "fused" (the fused one only) or "side" (the four side outputs only)."""
    if which == "fused":
        return ops.head_bwd(d["side"], d["filt"], None, None, d["fuse_w"], d["g"][4], None, c["H"], c["W"], filt_uniform=mask)
    return ops.head_bwd(d["side"], d["filt"], d["filt1"], d["dsn_w"], d["fuse_w"], d["g"][4] if which == "all" else None,
                        d["g"][:4], c["H"], c["W"], filt_uniform=mask)


class CaseMargins(Margins):
    """Margins, reported as ONE line: the worst margin of each family of checks (``what``), and where it was."""

    def bf16(self, layer, a, ref):
        super().bf16(layer, a, ref)
        try:
            assert_bf16_close(a, ref, layer)
        except AssertionError as e:
            self.bad.append(str(e))

    def report(self):
        worst = {}
        for layer, what, m in self.rows:
            m = m if m == m else float("inf")
            if what not in worst or m > worst[what][0]:
                worst[what] = (m, layer)
        print(f"[{self.tag}] " + "  ".join(f"{what} {m:.3f} ({layer})" for what, (m, layer) in worst.items()))
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)


def check_bwd(M, got, want, which):
    """One head_bwd result against the float64 gradients of the same upstream gradients."""
    d_side, d_fw, d_fb, d_dw, d_db = got
    for i in range(4):
        t = d_side[i].float().cpu()
        assert t.shape[:3] == want["side"][i].permute(0, 2, 3, 1).shape[:3] and t.shape[3] == 32
        M.exact(f"d_side[{i}]", "padding", t[..., 16:], torch.zeros_like(t[..., 16:]))
        M.bf16(f"d_side[{i}]", t[..., :16].permute(0, 3, 1, 2).double(), want["side"][i])
    if which == "side":  # no fused gradient: nothing reaches the fuse layer
        M.exact("d_fuse_w", "zero", d_fw.cpu(), torch.zeros(64))
        M.exact("d_fuse_b", "zero", d_fb.cpu(), torch.zeros(1))
    else:
        M.rel("d_fuse_w", "dparam", d_fw.cpu(), want["fw"], 2e-5)
        M.rel("d_fuse_b", "dparam", d_fb.cpu(), want["fb"], 2e-5)
    if which == "fused":
        assert d_dw is None and d_db is None
    else:
        for i in range(4):
            M.rel(f"d_dsn_w[{i}]", "dparam", d_dw[i].cpu(), want["dw"][i], 2e-5)
            M.rel(f"d_dsn_b[{i}]", "dparam", d_db[i:i + 1].cpu(), want["db"][i:i + 1], 2e-5)


def check_uniform_against_general(M, uni, gen_):
    """The uniform kernels against the general ones on the same (uniform) filters."""
    for i in range(4):
        M.rel(f"d_side[{i}]", "uni-dside", uni[0][i].float().cpu(), gen_[0][i].float().cpu(), 4e-3)
    for name, a, b in zip(("d_fuse_w", "d_fuse_b", "d_dsn_w", "d_dsn_b"), uni[1:], gen_[1:]):
        if a is not None:
            M.rel(name, "uni-dparam", a.cpu(), b.cpu(), 1e-5)


PARITY_CASES = [(sid, mask, so) for sid in SHAPES for mask in MASKS + (MIXED_MASKS if sid == "1x33x129" else ())
                for so in (True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape_id,mask,with_so", PARITY_CASES,
                         ids=[f"{sid}-{mask:04b}-{'so' if so else 'fused'}" for sid, mask, so in PARITY_CASES])
def test_head_tiles_parity(ops, shape_id, mask, with_so):
    """Forward and backward of one (shape, filter mask, side outputs) combination against the float64 reference, and - where
    the mask has a uniform scale - against the general kernels on the same inputs.  Masks 0b0000 and 0b1111, with and without
    side outputs, instantiate all sixteen k_head_bwd_scale kernels and both k_head_fwd kernels at every shape."""
    c = reference(shape_id, mask)
    d = device_inputs(c)
    assert ops.filters_uniform_mask(d["filt"]) == mask
    M = CaseMargins(f"parity {shape_id} mask={mask:04b} {'side-out' if with_so else 'fused-only'}")
    which = "all" if with_so else "fused"

    fused, so = run_fwd(ops, c, d, with_so, mask)
    M.rel("fused", "out", fused.cpu(), c["out"][4], 1e-5)
    if with_so:
        for i in range(4):
            M.rel(f"side_out[{i}]", "out", so[i].cpu(), c["out"][i], 1e-5)
    else:
        assert so is None
    got = run_bwd(ops, c, d, which, mask)
    check_bwd(M, got, c["grads"][which], which)

    if mask:
        fused_g, so_g = run_fwd(ops, c, d, with_so, 0)
        M.rel("fused", "uni-out", fused.cpu(), fused_g.cpu(), 2e-6)
        if with_so:
            for i in range(4):
                M.rel(f"side_out[{i}]", "uni-out", so[i].cpu(), so_g[i].cpu(), 2e-6)
        check_uniform_against_general(M, got, run_bwd(ops, c, d, which, 0))
    M.report()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS, ids=["0000", "1111"])
@pytest.mark.parametrize("shape_id", ["1x33x129", "15x40x129"])
def test_head_bwd_side_outputs_only(ops, shape_id, mask):
    """head_bwd(d_fused=None, d_side_out=[...]): a loss on the side outputs alone (engine.backward allows it).  d_side, d_dsn_w
    and d_dsn_b against autograd of the four side outputs; the fuse layer's gradients exactly zero."""
    c = reference(shape_id, mask)
    d = device_inputs(c)
    M = CaseMargins(f"side-only {shape_id} mask={mask:04b}")
    got = run_bwd(ops, c, d, "side", mask)
    check_bwd(M, got, c["grads"]["side"], "side")
    assert got[2].item() == 0.0
    if mask:
        check_uniform_against_general(M, got, run_bwd(ops, c, d, "side", 0))
    M.report()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS, ids=["0000", "1111"])
def test_head_bwd_slab_order_and_dirty_workspace(ops, mask):
    """k_head_finish adds the slabs in a fixed order and reads only the slabs of its own call: 1x33x129 on a workspace of NaN
    bytes, then 15x40x129 (which rewrites the same bytes with more slabs), then 1x33x129 again on the same inputs - every
    tensor head_bwd returns (d_side[0..3], d_fuse_w, d_fuse_b, d_dsn_w, d_dsn_b) finite, and bit for bit as the first time."""
    from fosvos_hip import lib
    small, large = reference("1x33x129", mask), reference("15x40x129", mask)
    ds, dl = device_inputs(small), device_inputs(large)
    need = lib().fosvos_head_bwd_workspace_bytes(large["n"], large["H"], large["W"])
    at = ops._WS.get(need, torch.device(DEV))[0]  # the shared workspace has its final size (and place) from here on
    next(b for b in ops._WS._buf.values() if b.data_ptr() == at).fill_(0xFF)
    first = run_bwd(ops, small, ds, "all", mask)
    run_bwd(ops, large, dl, "all", mask)
    third = run_bwd(ops, small, ds, "all", mask)
    assert ops._WS.get(1, torch.device(DEV))[0] == at, "the three runs did not share one workspace"
    flat = lambda r: list(r[0]) + list(r[1:])
    for k, (a, b) in enumerate(zip(flat(first), flat(third))):
        assert a.data_ptr() != b.data_ptr() and bool(torch.isfinite(a).all())
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)), f"tensor {k} differs"


# ------------------------------------------------------------------------------------------ the C entry points, directly
TAIL = 4096


class RawHead:
    """fosvos_head_fwd / fosvos_head_bwd through the raw binding: caller-owned outputs filled with NaN, a workspace of exactly
    the bytes the library asks for followed by TAIL bytes of 0xFF."""

    def __init__(self, c, d):
        from fosvos_hip import lib
        self.L, self.c, self.d = lib(), c, d
        n, H, W = c["n"], c["H"], c["W"]
        self.need = int(self.L.fosvos_head_bwd_workspace_bytes(n, H, W))
        nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device=DEV)
        self.d_side = [nan((n, s.shape[1], s.shape[2], 32), torch.bfloat16) for s in d["side"]]
        self.d_fw, self.d_fb = nan((64,), torch.float32), nan((1,), torch.float32)
        self.d_dw, self.d_db = nan((4, 16), torch.float32), nan((4,), torch.float32)
        self.fused = nan((n, 1, H, W), torch.float32)
        self.ws = torch.full((self.need + TAIL,), 0xFF, dtype=torch.uint8, device=DEV)
        self.stream = torch.cuda.current_stream(0).cuda_stream

    def outputs(self):
        return self.d_side + [self.d_fw, self.d_fb, self.d_dw, self.d_db]

    def bwd(self, hs=None, ws=None, workspace_bytes=None, d_fused=True, d_side_out=True):
        from fosvos_hip import int_array4, ptr_array4
        c, d = self.c, self.d
        ptrs = lambda ts: ptr_array4([t.data_ptr() for t in ts])
        none4 = ptr_array4([None] * 4)
        return self.L.fosvos_head_bwd(
            ptrs(d["side"]), int_array4(hs or [t.shape[1] for t in d["side"]]), int_array4(ws or [t.shape[2] for t in d["side"]]),
            ptrs(d["filt"]), ptrs(d["filt1"]), d["dsn_w"].data_ptr(), d["fuse_w"].data_ptr(),
            d["g"][4].data_ptr() if d_fused else None, ptrs(d["g"][:4]) if d_side_out else none4, ptrs(self.d_side),
            self.d_fw.data_ptr(), self.d_fb.data_ptr(), self.d_dw.data_ptr(), self.d_db.data_ptr(), c["n"], c["H"], c["W"], 0,
            self.ws.data_ptr(), self.need if workspace_bytes is None else workspace_bytes, 0, self.stream)

    def fwd(self, hs=None, ws=None):
        from fosvos_hip import int_array4, ptr_array4
        c, d = self.c, self.d
        ptrs = lambda ts: ptr_array4([t.data_ptr() for t in ts])
        return self.L.fosvos_head_fwd(
            ptrs(d["side"]), int_array4(hs or [t.shape[1] for t in d["side"]]), int_array4(ws or [t.shape[2] for t in d["side"]]),
            ptrs(d["filt"]), ptr_array4([None] * 4), None, None, d["fuse_w"].data_ptr(), d["fuse_b"].data_ptr(),
            self.fused.data_ptr(), ptr_array4([None] * 4), c["n"], c["H"], c["W"], 0, 0, self.stream)


@pytest.mark.gpu
@pytest.mark.parametrize("shape_id", ["1x33x129", "1x33x129-floor"])
def test_head_bwd_raw_abi_writes_every_output_and_stays_in_its_workspace(ops, shape_id):
    """After fosvos_head_bwd every element of every caller-owned output is finite (none was left at its NaN fill: each low-res
    pixel of each scale is written, padding channels included, also where the side maps are smaller than the ceil-pooled
    size), the bytes behind the workspace are untouched, and the values are those of ops.head_bwd bit for bit."""
    c = reference(shape_id, 0)
    d = device_inputs(c)
    raw = RawHead(c, d)
    assert raw.bwd() == 0
    torch.cuda.synchronize()
    for k, t in enumerate(raw.outputs()):
        assert bool(torch.isfinite(t).all()), f"output {k}: {int((~torch.isfinite(t)).sum())} elements not written"
    assert bool((raw.ws[raw.need:] == 0xFF).all()), "bytes behind the workspace were written"
    want = run_bwd(ops, c, d, "all", 0)
    for a, b in zip(raw.outputs(), list(want[0]) + list(want[1:])):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_head_raw_abi_refuses_bad_arguments_before_any_launch():
    """Each bad argument is refused with its code and without a single launch.  (Every buffer is large enough for what the
    bad call claims, so a refusal that went missing would fail this test and nothing else.)"""
    import fosvos_hip
    E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3  # include/fosvos_hip.h
    c = reference("1x33x129", 0)
    d = device_inputs(c)
    ceil_h = [s.shape[1] for s in d["side"]]
    cf = reference("1x33x129-floor", 0)
    raw, floor = RawHead(c, d), RawHead(cf, device_inputs(cf))
    cb = dict(c)  # for the too-large claim: side[0] and d_side[0] really have the claimed 17 + 1 rows
    cb["side"] = [torch.cat([c["side"][0], c["side"][0][:, :, :1]], dim=2)] + c["side"][1:]
    big = RawHead(cb, device_inputs(cb))
    short_h = [ceil_h[0], ceil_h[1], ceil_h[2], 1]                 # (1 + 1) * 16 = 32 < 33 rows; the buffers hold 3 rows
    assert (short_h[3] + 1) * 16 < c["H"]
    cases = [
        ("workspace one byte short", E_WORKSPACE, lambda: raw.bwd(workspace_bytes=raw.need - 1)),
        ("side map too small, bwd", E_SHAPE, lambda: raw.bwd(hs=short_h)),
        ("side map too small, fwd", E_SHAPE, lambda: raw.fwd(hs=short_h)),
        ("side map larger than ceil-pooled", E_SHAPE, lambda: big.bwd(hs=[ceil_h[0] + 1] + ceil_h[1:])),
        ("no upstream gradient", E_ARG, lambda: raw.bwd(d_fused=False, d_side_out=False)),
    ]
    torch.cuda.synchronize()
    with fosvos_hip.LaunchProfile(0, max_launches=16) as prof:
        for what, code, call in cases:
            assert call() == code, what
    assert prof.records == {}, prof.records
    torch.cuda.synchronize()
    for r in (raw, big):
        assert all(bool(torch.isnan(t).all()) for t in r.outputs()) and bool(torch.isnan(r.fused).all())
        assert bool((r.ws == 0xFF).all())
    # the same objects with good arguments are accepted, ceil- and floor-sized
    assert raw.bwd() == 0 and raw.fwd() == 0 and floor.bwd() == 0 and floor.fwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(raw.fused).all()) and bool(torch.isfinite(floor.fused).all())
