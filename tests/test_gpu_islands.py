"""Island tests of the VGG-step kernels (tests/islands.py): every operand of a raw C-ABI call - inputs, outputs, in-out tensors
and the workspace of exactly the reported bytes - sits alone between margins the test owns, and the call runs three times: on
zero margins, on POSITIVE quiet NaNs (outputs and workspace pre-filled with 0xFF) and on large finite values (pre-filled with
random bytes).  After each run every output holds the expected bits, every margin and every pure input is byte for byte what
it was.  A kernel that reads one pixel in front of a tensor, stores one pixel past an output or past its workspace, leaves an
output element unwritten or depends on what the workspace held fails here, deterministically, with the operand and the
distance in the message.  Run with ``pytest -m gpu``.

The conv cases, their operands, class assertions and expected bits are those of tests/exact_cases.py: exactly summable
operands, so the expected bits are unique - they do not depend on tile, split or summation order.  The pool runs on
integer-valued maps against exact_cases.pool / pool_backward.  The layout converters, the weight packers, the loss entries and
the head are compared with the bits of the matching ``ops`` call on ordinary tensors (the loss sums are fixed-order, the head's
slab sums too).  The native pass (fosvos_vgg_forward / _backward) runs once on an arena of exactly fosvos_vgg_arena_bytes: its
logits and gradients agree across the three runs.

No entry point here documents in include/fosvos_hip.h that a buffer must extend past its tensor, so no operand is extended.
The limit of the method is stated in tests/islands.py: a stray load whose value is discarded passes.  Every case prints its
launch class."""
import ctypes
import os
import sys
import zlib

import pytest
import torch

import exact_cases as E
import islands as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
RELU, OUT_F32 = 1, 2  # FOSVOS_CONV_RELU, FOSVOS_CONV_OUT_F32


@pytest.fixture(scope="module")
def ops():
    from fosvos_hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from fosvos_hip import lib
    return lib()


def _ids(cases):
    return [c.id for c in cases]


def _st():
    return torch.cuda.current_stream(0).cuda_stream


def _ck(rc, what):
    from fosvos_hip import check
    check(rc, what)


def nhwc(t, c_pad=None):
    """fp32 NCHW (cpu) -> bf16 NHWC (cpu), zero channels up to c_pad (the values are bf16-exact)."""
    t = t.permute(0, 2, 3, 1).contiguous()
    if c_pad is not None and c_pad != t.shape[3]:
        t = torch.cat([t, torch.zeros(*t.shape[:3], c_pad - t.shape[3])], 3)
    return t.to(BF)


def nhwc_f32(t):
    return t.permute(0, 2, 3, 1).contiguous()


def ptr(isl, name):
    return None if name is None else isl.ptr(name)


def run(rep, tag, operands, call, expected):
    rep.add(I.run_case(tag, operands, call, expected, device=DEV, seed=zlib.crc32(tag.encode()) & 0xFFFF))


# ------------------------------------------------------------------------------------------ forward
# N = 2: the boundary between two images and the edge of the tensor are different predicates (E.FWD_CASES are all N = 1)
FWD_TWO_IMAGES = E.Case("pp_two_images", (2, 61, 107, 64, 512), "pp<=64", 1010, xmax=8, wmax=4, bmax=64)
FWD = E.FWD_CASES + [FWD_TWO_IMAGES]


@pytest.mark.parametrize("c", FWD, ids=_ids(FWD))
def test_forward_islands(ops, L, c):
    """fosvos_conv3x3_fwd: bf16 with bias and ReLU, the linear form; the 16-channel cases with the fp32 output.
    fosvos_conv3x3_fwd_pool on the bf16 cases, both outputs islands."""
    n, h, w, ci, co = c.shape
    assert E.fwd_bound(c) < E.LIMIT and E.fwd_class(ops, c) == c.cls
    print(f"[{c.id}] {c.shape} launch class {c.cls}")
    x, wt, b = E.fwd_operands(c)
    ref = E.fwd_reference(x, wt, b)
    wf = ops.pack_conv3x3_weights(wt.to(DEV))[0].cpu()
    need = L.fosvos_conv3x3_workspace_bytes(n, h, w, ci, co)
    rep = I.Report(f"{c.id} {c.shape} {c.cls}")

    def form(tag, bias, flags, want, pooled=None):
        f32 = bool(flags & OUT_F32)
        operands = [I.inp("x", nhwc(x)), I.inp("w_packed", wf)] + ([I.inp("bias", b)] if bias else [])
        operands += [I.out("y", (n, h, w, co), F32 if f32 else BF), I.workspace("workspace", need)]
        expected = {"y": nhwc_f32(want) if f32 else nhwc(want)}
        if pooled is not None:
            operands.append(I.out("y_pool", (n, (h + 1) // 2, (w + 1) // 2, co), BF))
            expected["y_pool"] = nhwc(pooled)

        def call(isl):
            bp = isl.ptr("bias") if bias else None
            if pooled is None:
                _ck(L.fosvos_conv3x3_fwd(isl.ptr("x"), isl.ptr("w_packed"), bp, isl.ptr("y"), n, h, w, ci, co, flags,
                                         isl.ptr("workspace"), need, 0, _st()), "conv3x3_fwd")
            else:
                _ck(L.fosvos_conv3x3_fwd_pool(isl.ptr("x"), isl.ptr("w_packed"), bp, isl.ptr("y"), isl.ptr("y_pool"), n, h, w, ci,
                                              co, flags, isl.ptr("workspace"), need, 0, _st()), "conv3x3_fwd_pool")
        run(rep, f"{c.id} {tag}", operands, call, expected)

    if co == 16:
        form("fp32 conv + b", True, OUT_F32, ref["bias"])
        form("fp32 conv", False, OUT_F32, ref["linear"])
    else:
        form("relu(conv + b)", True, RELU, E.bf(ref["relu"]))
        form("linear", False, 0, E.bf(ref["linear"]))
        form("fwd_pool relu(conv + b)", True, RELU, E.bf(ref["relu"]), E.pool(E.bf(ref["relu"])))
        form("fwd_pool conv + b", True, 0, E.bf(ref["bias"]), E.pool(E.bf(ref["bias"])))
    rep.done()


# ------------------------------------------------------------------------------------------ data gradient
DGRAD_TWO_IMAGES = E.Case("mid_k1_two_images", (2, 61, 250, 64, 64), "8x16x64/k1", 2013, kind="plain",
                          ymax=8, wmax=4, amax=255, smin=2, smax=4)
PLAIN = [c for c in E.DGRAD_CASES if c.kind == "plain"] + [DGRAD_TWO_IMAGES]
UNPOOL = [c for c in E.DGRAD_CASES if c.kind == "unpool"]


def _dgrad_common(ops, L, c):
    n, h, w, ci, co = c.shape
    dy, wt, src, add = E.dgrad_operands(c)
    wd = ops.pack_conv3x3_weights(wt.to(DEV))[1].cpu()
    need = L.fosvos_conv3x3_workspace_bytes(n, h, w, co, ci)
    return dy, wt, src, add, wd, nhwc(dy, (co + 31) // 32 * 32), need


@pytest.mark.parametrize("c", PLAIN, ids=_ids(PLAIN))
def test_dgrad_islands(ops, L, c):
    """fosvos_conv3x3_dgrad plain, with relu_src, with a separate addend, with the addend aliased to out (the in-out form: the
    addend is the output's pre-fill in every run and part of the reference); fosvos_conv3x3_dgrad_bits with the mask as bits,
    alone and with a separate addend.  Mask, bit image and addend are islands of their own."""
    n, h, w, ci, co = c.shape
    bits_cls = getattr(c, "bits_cls", c.cls)
    assert E.dgrad_bound(c) < E.LIMIT and E.dgrad_class(ops, c) == c.cls and E.dgrad_bits_class(ops, c) == bits_cls
    print(f"[{c.id}] {c.shape} launch class {c.cls}, fosvos_conv3x3_dgrad_bits without an addend {bits_cls}")
    dy, wt, src, add, wd, dyd, need = _dgrad_common(ops, L, c)
    s = E.dgrad_sum(dy, wt)
    mask = src > 0
    srcd, addd = nhwc(src), nhwc(add)
    bits = E.relu_bits(srcd)
    rep = I.Report(f"{c.id} {c.shape} {c.cls}")

    def form(tag, want, mask_as=None, addend=None):
        """mask_as: None | "src" | "bits"; addend: None | "separate" | "aliased"."""
        operands = [I.inp("dy", dyd), I.inp("w_dgrad_packed", wd)]
        if mask_as == "src":
            operands.append(I.inp("relu_src", srcd))
        if mask_as == "bits":
            operands.append(I.inp("relu_bits", bits))
        if addend == "separate":
            operands.append(I.inp("addend", addd))
        operands.append(I.inout("dx", addd) if addend == "aliased" else I.out("dx", (n, h, w, ci), BF))
        operands.append(I.workspace("workspace", need))

        def call(isl):
            ap = {None: None, "separate": "addend", "aliased": "dx"}[addend]
            if mask_as == "bits":
                _ck(L.fosvos_conv3x3_dgrad_bits(isl.ptr("dy"), isl.ptr("w_dgrad_packed"), isl.ptr("relu_bits"), ptr(isl, ap),
                                                isl.ptr("dx"), n, h, w, ci, co, isl.ptr("workspace"), need, 0, _st()), "dgrad_bits")
            else:
                _ck(L.fosvos_conv3x3_dgrad(isl.ptr("dy"), isl.ptr("w_dgrad_packed"), ptr(isl, "relu_src" if mask_as else None),
                                           ptr(isl, ap), isl.ptr("dx"), n, h, w, ci, co, isl.ptr("workspace"), need, 0, _st()),
                    "dgrad")
        run(rep, f"{c.id} {tag}", operands, call, {"dx": nhwc(want)})

    form("plain", E.dgrad_epilogue(s)[0])
    form("relu_src", E.dgrad_epilogue(s, mask)[0], "src")
    form(f"relu_bits ({bits_cls})", E.dgrad_epilogue(s, mask)[0], "bits")
    form("separate addend", E.dgrad_epilogue(s, None, add)[0], None, "separate")
    form("addend aliased to out", E.dgrad_epilogue(s, None, add)[0], None, "aliased")
    form("relu_src + addend aliased to out", E.dgrad_epilogue(s, mask, add)[0], "src", "aliased")
    form("relu_bits + separate addend", E.dgrad_epilogue(s, mask, add)[0], "bits", "separate")
    rep.done()


@pytest.mark.parametrize("c", UNPOOL, ids=_ids(UNPOOL))
def test_dgrad_unpool_islands(ops, L, c):
    """fosvos_conv3x3_dgrad_unpool: x (mask and arg-max source) and d_pooled are islands of their own."""
    n, h, w, ci, co = c.shape
    assert E.dgrad_bound(c) < E.LIMIT and E.dgrad_class(ops, c) == c.cls
    print(f"[{c.id}] {c.shape} launch class {c.cls}")
    dy, wt, src, dpool, wd, dyd, need = _dgrad_common(ops, L, c)
    want = E.dgrad_epilogue(E.dgrad_sum(dy, wt), src > 0, E.pool_backward(src, dpool))[0]
    operands = [I.inp("dy", dyd), I.inp("w_dgrad_packed", wd), I.inp("x", nhwc(src)), I.inp("d_pooled", nhwc(dpool)),
                I.out("dx", (n, h, w, ci), BF), I.workspace("workspace", need)]

    def call(isl):
        _ck(L.fosvos_conv3x3_dgrad_unpool(isl.ptr("dy"), isl.ptr("w_dgrad_packed"), isl.ptr("x"), isl.ptr("d_pooled"), isl.ptr("dx"),
                                          n, h, w, ci, co, isl.ptr("workspace"), need, 0, _st()), "dgrad_unpool")
    rep = I.Report(f"{c.id} {c.shape} {c.cls}")
    run(rep, f"{c.id} dgrad_unpool", operands, call, {"dx": nhwc(want)})
    rep.done()


# ------------------------------------------------------------------------------------------ weight and bias gradient
@pytest.mark.parametrize("c", E.WGRAD_CASES, ids=_ids(E.WGRAD_CASES))
def test_wgrad_islands(L, c):
    """fosvos_conv3x3_wgrad_slabs + _reduce with and without the bias gradient and with accumulate=1 onto integer prefills (the
    in-out form), and fosvos_conv3x3_wgrad in one call.  The workspace is exactly fosvos_conv3x3_wgrad_workspace_bytes."""
    n, h, w, ci, co = c.shape
    assert E.wgrad_bound(c) < E.LIMIT
    print(f"[{c.id}] {c.shape} launch class: {c.cls}")
    x, dy, pw, pb = E.wgrad_operands(c)
    dw_ref, db_ref = E.wgrad_reference(x, dy)
    xd, dyd = nhwc(x), nhwc(dy, (co + 31) // 32 * 32)
    need = L.fosvos_conv3x3_wgrad_workspace_bytes(n, h, w, ci, co)
    rep = I.Report(f"{c.id} {c.shape}: {c.cls}")

    def form(tag, with_bias, accumulate, one_call):
        operands = [I.inp("x", xd), I.inp("dy", dyd)]
        operands.append(I.inout("dw", pw, is_map=False) if accumulate else I.out("dw", (co, ci, 3, 3), F32, is_map=False))
        expected = {"dw": dw_ref + pw if accumulate else dw_ref}
        if with_bias:
            operands.append(I.inout("db", pb) if accumulate else I.out("db", (co,), F32))
            expected["db"] = db_ref + pb if accumulate else db_ref
        operands.append(I.workspace("workspace", need))

        def call(isl):
            dbp = isl.ptr("db") if with_bias else None
            if one_call:
                _ck(L.fosvos_conv3x3_wgrad(isl.ptr("x"), isl.ptr("dy"), isl.ptr("dw"), dbp, n, h, w, ci, co, accumulate,
                                           isl.ptr("workspace"), need, 0, _st()), "wgrad")
                return
            _ck(L.fosvos_conv3x3_wgrad_slabs(isl.ptr("x"), isl.ptr("dy"), 1 if with_bias else 0, n, h, w, ci, co,
                                             isl.ptr("workspace"), need, 0, _st()), "wgrad_slabs")
            _ck(L.fosvos_conv3x3_wgrad_reduce(isl.ptr("dw"), dbp, n, h, w, ci, co, accumulate, isl.ptr("workspace"), need, 0,
                                              _st()), "wgrad_reduce")
        run(rep, f"{c.id} {tag}", operands, call, expected)

    form("slabs + reduce", True, 0, False)
    form("slabs + reduce, no bias gradient", False, 0, False)
    form("slabs + reduce, accumulate", True, 1, False)
    form("one call", True, 0, True)
    form("one call, no bias gradient", False, 0, True)
    rep.done()


# ------------------------------------------------------------------------------------------ conv1_1
@pytest.mark.parametrize("c", E.FIRST_FWD_CASES, ids=_ids(E.FIRST_FWD_CASES))
def test_first_forward_islands(ops, L, c):
    """fosvos_conv3x3_first_fwd with and without the bit output.  The frame is fp32 NCHW: a flat operand here (17 rows of one
    of its planes are far less than the 64 KiB margin)."""
    n, h, w = c.shape
    assert E.first_fwd_bound(c) < E.LIMIT
    tiles, wgs = ops.conv3x3_first_plan(n, h, w)
    print(f"[{c.id}] {c.shape} launch class: {c.cls}, {tiles} tiles on {wgs} workgroups")
    frame, wt, b = E.first_fwd_operands(c)
    pre = E.first_fwd_reference(frame, wt, b)
    rep = I.Report(f"{c.id} {c.shape}")
    for with_bits in (True, False):
        operands = [I.inp("frame", frame, is_map=False), I.inp("w_oihw", wt, is_map=False), I.inp("bias", b),
                    I.out("y", (n, h, w, 64), BF)] + ([I.out("relu_bits", (n, h, w, 8), U8)] if with_bits else [])
        expected = {"y": nhwc(E.bf(pre)), "relu_bits": E.relu_bits(nhwc_f32(pre))}

        def call(isl, with_bits=with_bits):
            _ck(L.fosvos_conv3x3_first_fwd(isl.ptr("frame"), isl.ptr("w_oihw"), isl.ptr("bias"), isl.ptr("y"),
                                           isl.ptr("relu_bits") if with_bits else None, n, h, w, 64, 0, _st()), "first_fwd")
        run(rep, f"{c.id} {'with' if with_bits else 'without'} the bit output", operands, call, expected)
    rep.done()


@pytest.mark.parametrize("c", E.FIRST_WGRAD_CASES, ids=_ids(E.FIRST_WGRAD_CASES))
def test_first_wgrad_islands(L, c):
    n, h, w = c.shape
    assert E.first_wgrad_bound(c) < E.LIMIT
    print(f"[{c.id}] {c.shape} launch class: {c.cls}")
    frame, dy = E.first_wgrad_operands(c)
    dw_ref, db_ref = E.first_wgrad_reference(frame, dy)
    need = L.fosvos_conv3x3_first_wgrad_workspace_bytes(n, h, w, 64)
    operands = [I.inp("frame", frame, is_map=False), I.inp("dy", nhwc(dy)), I.out("dw", (64, 3, 3, 3), F32, is_map=False),
                I.out("db", (64,), F32), I.workspace("workspace", need)]

    def call(isl):
        _ck(L.fosvos_conv3x3_first_wgrad(isl.ptr("frame"), isl.ptr("dy"), isl.ptr("dw"), isl.ptr("db"), n, h, w, 64,
                                         isl.ptr("workspace"), need, 0, _st()), "first_wgrad")
    rep = I.Report(f"{c.id} {c.shape}: {c.cls}")
    run(rep, f"{c.id} first_wgrad", operands, call, {"dw": dw_ref, "db": db_ref})
    rep.done()


# ------------------------------------------------------------------------------------------ pool
POOL_SHAPES = [(1, 1, 1, 64), (1, 2, 3, 128), (1, 7, 1, 64), (2, 61, 107, 64)]


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["x".join(map(str, s)) for s in POOL_SHAPES])
def test_maxpool_islands(L, shape):
    """fosvos_maxpool2x2_ceil_fwd and _bwd with and without the ReLU mask, on integer-valued maps full of ties."""
    n, h, w, ch = shape
    print(f"[pool {shape}] launch class: k_maxpool2x2_ceil_fwd / _bwd, {(h + 1) // 2} x {(w + 1) // 2} windows, ragged "
          f"{'rows ' if h % 2 else ''}{'columns' if w % 2 else ''}")
    g = torch.Generator().manual_seed(5000 + h * w)
    x = torch.randint(-3, 5, (n, ch, h, w), generator=g).float()
    d = torch.randint(-255, 256, (n, ch, (h + 1) // 2, (w + 1) // 2), generator=g).float()
    rep = I.Report(f"pool {shape}")
    operands = [I.inp("x", nhwc(x)), I.out("y", (n, (h + 1) // 2, (w + 1) // 2, ch), BF)]

    def fwd(isl):
        _ck(L.fosvos_maxpool2x2_ceil_fwd(isl.ptr("x"), isl.ptr("y"), n, h, w, ch, 0, _st()), "maxpool_fwd")
    run(rep, f"pool {shape} fwd", operands, fwd, {"y": nhwc(E.pool(x))})
    for relu_mask in (1, 0):
        operands = [I.inp("x", nhwc(x)), I.inp("dy", nhwc(d)), I.out("dx", (n, h, w, ch), BF)]

        def bwd(isl, relu_mask=relu_mask):
            _ck(L.fosvos_maxpool2x2_ceil_bwd(isl.ptr("x"), isl.ptr("dy"), isl.ptr("dx"), n, h, w, ch, relu_mask, 0, _st()),
                "maxpool_bwd")
        run(rep, f"pool {shape} bwd relu_mask={relu_mask}", operands, bwd, {"dx": nhwc(E.pool_backward(x, d, bool(relu_mask)))})
    rep.done()


# ------------------------------------------------------------------------------------------ layout, weight images
def _gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_layout_converter_islands(ops, L):
    """The four converters at the shapes of test_layout_roundtrip (channels padded 5 -> 8); expected: the ops calls."""
    print("[layout] launch class: the four layout converters, 2x5x7x9 (c_pad 8) and 2x16x5x6")
    rep = I.Report("layout")
    x = _gen(2, 5, 7, 9, seed=1)
    y = ops.nchw_to_nhwc_bf16(x.to(DEV), c_pad=8)
    s = _gen(2, 16, 5, 6, seed=2)
    s_nhwc = ops.nchw_to_nhwc_f32(s.to(DEV))
    cases = [
        ("nchw_f32_to_nhwc_bf16", x, y.cpu(), lambda i: L.fosvos_nchw_f32_to_nhwc_bf16(i.ptr("src"), i.ptr("dst"), 2, 5, 7, 9, 8, 0, _st())),
        ("nhwc_bf16_to_nchw_f32", y.cpu(), ops.nhwc_bf16_to_nchw(y, c=5).cpu(),
         lambda i: L.fosvos_nhwc_bf16_to_nchw_f32(i.ptr("src"), i.ptr("dst"), 2, 5, 7, 9, 8, 0, _st())),
        ("nchw_f32_to_nhwc_f32", s, s_nhwc.cpu(), lambda i: L.fosvos_nchw_f32_to_nhwc_f32(i.ptr("src"), i.ptr("dst"), 2, 16, 5, 6, 0, _st())),
        ("nhwc_f32_to_nchw_f32", s_nhwc.cpu(), ops.nhwc_f32_to_nchw(s_nhwc).cpu(),
         lambda i: L.fosvos_nhwc_f32_to_nchw_f32(i.ptr("src"), i.ptr("dst"), 2, 16, 5, 6, 0, _st())),
    ]
    for name, src, want, fn in cases:
        operands = [I.inp("src", src, is_map=False), I.out("dst", tuple(want.shape), want.dtype, is_map=False)]
        run(rep, name, operands, lambda isl, fn=fn, name=name: _ck(fn(isl), name), {"dst": want})
    rep.done()


PACK_SHAPES = [(64, 64), (16, 128), (128, 64), (64, 3), (16, 40)]
PACK_MULTI = [(64, 64), (128, 64), (16, 128), (256, 128), (16, 512), (96, 32)]


def test_pack_weights_islands(ops, L):
    """fosvos_pack_conv3x3_weights at the shapes of test_pack_weights (3 and 40 input channels padded to 32 and 64, 16
    output channels), and the _multi form with every master and every image of six layers an island."""
    from fosvos_hip import PackEntry
    print(f"[pack] launch class: fosvos_pack_conv3x3_weights {PACK_SHAPES}, _multi {PACK_MULTI}")
    rep = I.Report("pack")
    for co, ci in PACK_SHAPES:
        wt = _gen(co, ci, 3, 3, seed=3)
        fwd, dgr = ops.pack_conv3x3_weights(wt.to(DEV))
        operands = [I.inp("w", wt, is_map=False), I.out("w_fwd", (fwd.numel(),), BF), I.out("w_dgrad", (dgr.numel(),), BF)]

        def call(isl, co=co, ci=ci):
            _ck(L.fosvos_pack_conv3x3_weights(isl.ptr("w"), co, ci, isl.ptr("w_fwd"), isl.ptr("w_dgrad"), 0, _st()), "pack")
        run(rep, f"pack {co}x{ci}", operands, call, {"w_fwd": fwd.cpu(), "w_dgrad": dgr.cpu()})
    ws = [_gen(co, ci, 3, 3, seed=40 + i) for i, (co, ci) in enumerate(PACK_MULTI)]
    want = ops.pack_conv3x3_weights_multi([t.to(DEV) for t in ws])
    operands, expected = [], {}
    for i, (wt, (fwd, dgr)) in enumerate(zip(ws, want)):
        operands += [I.inp(f"w[{i}]", wt, is_map=False), I.out(f"w_fwd[{i}]", (fwd.numel(),), BF),
                     I.out(f"w_dgrad[{i}]", (dgr.numel(),), BF)]
        expected[f"w_fwd[{i}]"], expected[f"w_dgrad[{i}]"] = fwd.cpu(), dgr.cpu()

    def multi(isl):
        arr = (PackEntry * len(ws))()
        for i, (co, ci) in enumerate(PACK_MULTI):
            arr[i].w, arr[i].w_fwd, arr[i].w_dgrad = isl.ptr(f"w[{i}]"), isl.ptr(f"w_fwd[{i}]"), isl.ptr(f"w_dgrad[{i}]")
            arr[i].Co, arr[i].Ci = co, ci
        _ck(L.fosvos_pack_conv3x3_weights_multi(arr, len(ws), 0, _st()), "pack_multi")
    run(rep, "pack multi", operands, multi, expected)
    rep.done()


# ------------------------------------------------------------------------------------------ loss
LOSS_SHAPES = [(1, 1, 3, 5), (3, 1, 40, 52), (1, 1, 1028, 1024)]
N_MAPS = 5
SCALES = (0.75, 0.75, 0.75, 0.75, 1.0)
GRAD_SCALE = 0.2


def loss_inputs(shape):
    """Logits of five maps, a label batch and a void map whose valid pixels hold both classes in every frame
    (tests/test_islands_cpu.py asserts that, without a GPU)."""
    g = torch.Generator().manual_seed(6000 + shape[2])
    logits = [torch.randn(*shape, generator=g) * 3 for _ in range(N_MAPS)]
    label = (torch.rand(*shape, generator=g) < 0.3).float()
    void = (torch.rand(*shape, generator=g) < 0.4).to(U8)
    flat = label.reshape(shape[0], -1)
    flat[:, 0], flat[:, 1] = 1.0, 0.0  # both classes in every frame, and on pixels that are not void
    void.reshape(shape[0], -1)[:, :2] = 0
    return logits, label, void


def _loss_case(ops, L, shape, offset, rep):
    n = shape[0]
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    per = numel // n
    logits, label, void = loss_inputs(shape)
    dl, dlab, dvoid = [t.to(DEV) for t in logits], label.to(DEV), void.to(DEV)
    tag = f"loss {shape}" + (f" +{offset} B" if offset else "")
    flat = dict(is_map=False, offset=offset)

    def tensors(m=1, with_void=False):
        o = [I.inp(f"logits[{i}]", logits[i], **flat) for i in range(m)] + [I.inp("label", label, **flat)]
        if with_void:
            o.append(I.inp("void", void, is_map=False))
        return o + [I.out(f"grad[{i}]", shape, F32, **flat) for i in range(m)]

    # fosvos_cbce_loss: the whole tensor as one frame
    want_l, want_g = ops.cbce_loss(dl[0], dlab, size_average=False, grad_scale=GRAD_SCALE)
    need = L.fosvos_cbce_workspace_bytes(numel)
    operands = tensors() + [I.out("loss_out", (1,), F32), I.workspace("workspace", need)]
    run(rep, f"{tag} cbce_loss", operands,
        lambda i: _ck(L.fosvos_cbce_loss(i.ptr("logits[0]"), i.ptr("label"), numel, 0, GRAD_SCALE, i.ptr("loss_out"), i.ptr("grad[0]"),
                                         i.ptr("workspace"), need, 0, _st()), "cbce_loss"),
        {"loss_out": want_l.reshape(1).cpu(), "grad[0]": want_g.cpu()})

    # fosvos_cbce_loss_batch_counts with the counts of the tensor itself
    counts = torch.tensor([float((label >= 0.5).sum()), float(numel)], dtype=torch.float64)
    want_l, want_g = ops.cbce_loss(dl[0], dlab, size_average=True, grad_scale=GRAD_SCALE, batch_counts=counts.to(DEV))
    operands = tensors() + [I.inp("batch_counts", counts), I.out("loss_out", (1,), F32), I.workspace("workspace", need)]
    run(rep, f"{tag} cbce_loss_batch_counts", operands,
        lambda i: _ck(L.fosvos_cbce_loss_batch_counts(i.ptr("logits[0]"), i.ptr("label"), numel, 1, GRAD_SCALE, i.ptr("batch_counts"),
                                                      i.ptr("loss_out"), i.ptr("grad[0]"), i.ptr("workspace"), need, 0, _st()),
                      "cbce_loss_batch_counts"),
        {"loss_out": want_l.reshape(1).cpu(), "grad[0]": want_g.cpu()})

    # fosvos_cbce_loss_frames, and _frames_parts in its three stages (three calls that share the workspace)
    want_l, want_g = ops.cbce_loss_frames(dl[0], dlab, size_average=False, grad_scale=GRAD_SCALE)
    need = n * L.fosvos_cbce_workspace_bytes(per)
    operands = tensors() + [I.out("loss_out", (n,), F32), I.workspace("workspace", need)]
    expected = {"loss_out": want_l.cpu(), "grad[0]": want_g.cpu()}
    run(rep, f"{tag} cbce_loss_frames", operands,
        lambda i: _ck(L.fosvos_cbce_loss_frames(i.ptr("logits[0]"), i.ptr("label"), per, n, 0, GRAD_SCALE, i.ptr("loss_out"),
                                                i.ptr("grad[0]"), i.ptr("workspace"), need, 0, _st()), "cbce_loss_frames"), expected)

    def parts(i):
        for stage in (1, 2, 4):  # FOSVOS_CBCE_COUNT, _LOSS, _FINISH
            _ck(L.fosvos_cbce_loss_frames_parts(i.ptr("logits[0]"), i.ptr("label"), per, n, 0, GRAD_SCALE, i.ptr("loss_out"),
                                                i.ptr("grad[0]"), i.ptr("workspace"), need, stage, 0, _st()), f"parts({stage})")
    run(rep, f"{tag} cbce_loss_frames_parts, three stages", operands, parts, expected)

    # fosvos_cbce_loss_frames_void
    want_l, want_g = ops.cbce_loss_frames(dl[0], dlab, size_average=False, grad_scale=GRAD_SCALE, void=dvoid)
    need_v = L.fosvos_cbce_void_workspace_bytes(per, n)
    operands = tensors(with_void=True) + [I.out("loss_out", (n,), F32), I.workspace("workspace", need_v)]
    run(rep, f"{tag} cbce_loss_frames_void", operands,
        lambda i: _ck(L.fosvos_cbce_loss_frames_void(i.ptr("logits[0]"), i.ptr("label"), i.ptr("void"), per, n, 0, GRAD_SCALE,
                                                     i.ptr("loss_out"), i.ptr("grad[0]"), i.ptr("workspace"), need_v, 0, _st()),
                      "cbce_loss_frames_void"),
        {"loss_out": want_l.cpu(), "grad[0]": want_g.cpu()})

    # fosvos_cbce_loss_frames_multi: five maps that share the label batch
    want_l, want_g = ops.cbce_loss_frames_multi(dl, dlab, SCALES, size_average=False)
    need_m = L.fosvos_cbce_multi_workspace_bytes(per, n, N_MAPS)
    operands = tensors(N_MAPS) + [I.out("loss_out", (n, N_MAPS), F32), I.workspace("workspace", need_m)]
    expected = {"loss_out": want_l.cpu(), **{f"grad[{m}]": want_g[m].cpu() for m in range(N_MAPS)}}

    def multi(i):
        lp = (ctypes.c_void_p * N_MAPS)(*[i.ptr(f"logits[{m}]") for m in range(N_MAPS)])
        gp = (ctypes.c_void_p * N_MAPS)(*[i.ptr(f"grad[{m}]") for m in range(N_MAPS)])
        _ck(L.fosvos_cbce_loss_frames_multi(lp, i.ptr("label"), per, n, N_MAPS, 0, (ctypes.c_float * N_MAPS)(*SCALES),
                                            i.ptr("loss_out"), gp, i.ptr("workspace"), need_m, 7, 0, _st()), "cbce_loss_frames_multi")
    run(rep, f"{tag} cbce_loss_frames_multi, five maps", operands, multi, expected)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["x".join(map(str, s)) for s in LOSS_SHAPES])
def test_loss_islands(ops, L, shape):
    """fosvos_cbce_loss, _batch_counts, _frames, _frames_parts (three stages), _frames_void and _frames_multi (five maps):
    logits, label, void bytes, gradients, the loss_out floats and the exact workspace are islands.  Less than one vector, a
    ragged last block, and a tensor on which the stride loop runs."""
    print(f"[loss {shape}] launch class: count / loss / finish kernels, {shape[0]} frames of {shape[2] * shape[3]} pixels")
    rep = I.Report(f"loss {shape}")
    _loss_case(ops, L, shape, 0, rep)
    rep.done()


def test_loss_islands_at_the_least_alignment(ops, L):
    """Logits, label and gradient 16 bytes past the 256-byte boundary: the least alignment include/fosvos_hip.h allows."""
    print("[loss +16 B] launch class: count / loss / finish kernels, operands at 16-byte alignment")
    rep = I.Report("loss (3, 1, 40, 52) at 16-byte alignment")
    _loss_case(ops, L, (3, 1, 40, 52), 16, rep)
    rep.done()


# ------------------------------------------------------------------------------------------ head
def test_head_islands(ops, L):
    """fosvos_head_fwd / fosvos_head_bwd at 1x33x129, the smallest shape of tests/test_gpu_head_tiles.py at which every tile
    splits: side maps, filters, incoming gradients, every output and the exact workspace are islands; general filters, side
    outputs on."""
    from fosvos_hip import int_array4, ptr_array4
    import test_gpu_head_tiles as T
    c = T.reference("1x33x129", 0)
    d = T.device_inputs(c)
    n, H, W = c["n"], c["H"], c["W"]
    hs, ws_ = [t.shape[1] for t in d["side"]], [t.shape[2] for t in d["side"]]
    print(f"[head 1x33x129] launch class: k_head_fwd<side outputs>, k_head_bwd_scale<S, side outputs, general> blocks "
          f"{T.bwd_blocks(H, W, 'ceil')}, k_head_finish")
    fused, so = T.run_fwd(ops, c, d, True, 0)
    want_b = T.run_bwd(ops, c, d, "all", 0)
    rep = I.Report("head 1x33x129")
    ins = [I.inp(f"side[{s}]", d["side"][s].cpu()) for s in range(4)]
    ins += [I.inp(f"filt[{s}]", d["filt"][s].cpu(), is_map=False) for s in range(4)]
    ins += [I.inp(f"filt1[{s}]", d["filt1"][s].cpu(), is_map=False) for s in range(4)]
    ins += [I.inp(k, d[k].cpu(), is_map=False) for k in ("dsn_w", "dsn_b", "fuse_w", "fuse_b")]
    arr = lambda i, name: ptr_array4([i.ptr(f"{name}[{s}]") for s in range(4)])

    operands = ins + [I.out("fused", (n, 1, H, W), F32, is_map=False)] + [I.out(f"side_out[{s}]", (n, 1, H, W), F32, is_map=False)
                                                                        for s in range(4)]
    expected = {"fused": fused.cpu(), **{f"side_out[{s}]": so[s].cpu() for s in range(4)}}

    def fwd(i):
        _ck(L.fosvos_head_fwd(arr(i, "side"), int_array4(hs), int_array4(ws_), arr(i, "filt"), arr(i, "filt1"), i.ptr("dsn_w"),
                              i.ptr("dsn_b"), i.ptr("fuse_w"), i.ptr("fuse_b"), i.ptr("fused"), arr(i, "side_out"), n, H, W, 0, 0,
                              _st()), "head_fwd")
    run(rep, "head_fwd", operands, fwd, expected)

    need = L.fosvos_head_bwd_workspace_bytes(n, H, W)
    operands = ins + [I.inp(f"d_side_out[{s}]", d["g"][s].cpu(), is_map=False) for s in range(4)]
    operands += [I.inp("d_fused", d["g"][4].cpu(), is_map=False)]
    operands += [I.out(f"d_side[{s}]", (n, hs[s], ws_[s], 32), BF) for s in range(4)]
    operands += [I.out("d_fuse_w", (64,), F32), I.out("d_fuse_b", (1,), F32), I.out("d_dsn_w", (4, 16), F32),
                 I.out("d_dsn_b", (4,), F32), I.workspace("workspace", need)]
    expected = {f"d_side[{s}]": want_b[0][s].cpu() for s in range(4)}
    expected.update({"d_fuse_w": want_b[1].cpu(), "d_fuse_b": want_b[2].cpu(), "d_dsn_w": want_b[3].cpu(), "d_dsn_b": want_b[4].cpu()})

    def bwd(i):
        _ck(L.fosvos_head_bwd(arr(i, "side"), int_array4(hs), int_array4(ws_), arr(i, "filt"), arr(i, "filt1"), i.ptr("dsn_w"),
                              i.ptr("fuse_w"), i.ptr("d_fused"), arr(i, "d_side_out"), arr(i, "d_side"), i.ptr("d_fuse_w"),
                              i.ptr("d_fuse_b"), i.ptr("d_dsn_w"), i.ptr("d_dsn_b"), n, H, W, 0, i.ptr("workspace"), need, 0, _st()),
            "head_bwd")
    run(rep, "head_bwd", operands, bwd, expected)
    rep.done()


# ------------------------------------------------------------------------------------------ the native pass
def test_vgg_pass_islands(L):
    """fosvos_vgg_forward and fosvos_vgg_backward once, one frame of 61x107: the arena, holding exactly
    fosvos_vgg_arena_bytes, the frame, the logits and the incoming gradient are islands (weights and gradient buffers stay
    ordinary tensors).  Logits and all parameter gradients agree across the three runs; margins and inputs intact."""
    from fosvos_hip import VggGrads, engine
    import test_gpu_layer_parity as P
    n, h, w = 1, 61, 107
    print(f"[vgg 1x61x107] launch classes: {sorted(P.launch_classes(n, h, w))}")
    net = P.make_net(21)
    params = dict(zip(engine.PARAM_NAMES, net._ordered_params()))
    wts, keep = engine._weights_struct(params, net._packs)
    ctx = net._packs.arenas.ctx(0)
    need = L.fosvos_vgg_arena_bytes(n, h, w)
    frame = P.O.synthetic_frame(n, h, w, seed=361)[0]
    d_fused = torch.randn(n, 1, h, w, generator=torch.Generator().manual_seed(362)) * 1e-3
    operands = [I.inp("frame", frame, is_map=False), I.inp("d_fused", d_fused, is_map=False),
                I.out("fused", (n, 1, h, w), F32, is_map=False),
                I.workspace("arena", need, margin=I.margin_bytes((n, h, w, 64), BF, True))]
    grads = []

    def call(isl):
        G = P._grad_buffers(net, lambda _n, p: torch.full_like(p, float("nan")))
        g = VggGrads()
        for c, (wn, bn) in enumerate(engine._CONV_NAMES):
            g.conv_w[c], g.conv_b[c] = G[wn].data_ptr(), G[bn].data_ptr()
        for i in range(4):
            g.side_w[i], g.side_b[i] = G[f"side_prep.{i}.weight"].data_ptr(), G[f"side_prep.{i}.bias"].data_ptr()
        g.fuse_w, g.fuse_b = G["fuse.weight"].data_ptr(), G["fuse.bias"].data_ptr()
        g.accumulate, g.defer_join, g.bucket_events, g.last_pass_of_cycle = 0, 0, 0, 1
        _ck(L.fosvos_vgg_forward(ctypes.byref(wts), isl.ptr("frame"), n, h, w, isl.ptr("arena"), need, isl.ptr("fused"), None, 0,
                                 _st()), "vgg_forward")
        _ck(L.fosvos_vgg_backward(ctx, ctypes.byref(wts), ctypes.byref(g), isl.ptr("frame"), n, h, w, isl.ptr("arena"), need,
                                  isl.ptr("d_fused"), None, _st(), None), "vgg_backward")
        torch.cuda.synchronize()
        grads.append({k: t.cpu() for k, t in G.items()})

    res = I.run_case("vgg pass 1x61x107", operands, call, None, device=DEV, seed=21, attribute=False)
    rep = I.Report("vgg pass 1x61x107")
    rep.add(res)
    assert bool(torch.isfinite(res.outputs["Z"]["fused"]).all())
    for k, name in ((1, "N"), (2, "B")):
        for key, t in grads[0].items():
            assert bool(torch.isfinite(t).all()), key
            if not torch.equal(t.view(torch.int32), grads[k][key].view(torch.int32)):
                rep.bad.append(f"gradient {key}: run {name} differs from run Z in {int((t != grads[k][key]).sum())} elements"
                               f" ({int((~torch.isfinite(grads[k][key])).sum())} non-finite)")
    del keep
    rep.done()
