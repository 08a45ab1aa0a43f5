"""Every kernel class the full-size OSVOS_RESNET pass launches (csrc/resnet.hip, the residual / stride-2 / 16-channel forms of
csrc/conv_igemm.hip, fosvos_hip/resnet_engine.py), each against a float64 reference on the CPU:

  * B1  one GPU case per launch class, at the smallest shape that selects it; the class is asserted through the plan queries
        (ops.conv2d_plan, ops.conv3x3_plan) before the launch.  Both sides get the same bf16-rounded operands, no BatchNorm.
  * B2  test_launch_classes_of_the_full_size_nets_are_covered (CPU): every conv launch of ResNet-18 / -34 at 1080x1920 and
        480x854 (scale_down_exponent 0..3, MFMA on / off, 1 or 2 frames) is enumerated from resnet_engine.width, the channel
        tables and the plan queries, and each class must appear in a B1 case that really selects it.
  * B3  the deconv head across its 640-column blocks, B4 the pool on negative values, B5 the packed weight images.
  * B6  the shipped native pass on an arena poisoned with 0xFF (and with 0x00), guard bytes behind it.
  * B7  the layers of the 1080p pass, teacher-forced: each layer recomputed in float64 from its own bf16 input.

Tolerance forms (tests/test_gpu_ops.py, tests/test_gpu_layer_parity.py), per element, never the tensor-max form:
  * one bf16 rounding of an fp32 sum (direct conv with or without addend - it adds in fp32 -, first layer, MFMA plain and
    stride 2):                                   |err| <= 2^-8 |ref| + 1e-5 max|ref|                      (assert_bf16_close)
  * MFMA residual (the tile is rounded to bf16 before the add): 2^-7 |ref| + 1e-5 max|ref| + 2^-7 |conv + bias| (bf16_two)
  * fp32 side maps: rel-to-max 2e-5; head: 1e-4 max(1, max|ref|); pool, padded channels, repeated launches: exact.
Every case prints its plan and its worst error in units of the tolerance (1.0 = on the bar).

A class is
  ("direct", form, cob, threads, slices)   k_conv2d<KS,S,COB,OUT_F32,SLICED>; form = "3x3s1", "3x3s2", "1x1s1", "1x1s2", "3x3s1_f32"
  ("first_fp32", cob)                      k_conv7x7s2_first<COB>
  ("first_mfma", nfb) / ("first_pool_mfma", nfb)   the MFMA first layer alone / fused with the pool
  ("mfma", epilogue, tile[, K chunks])     k_conv3x3_igemm through fosvos_conv3x3_fwd_add / _s2_fwd (never split); epilogue =
                                           "res_relu", "res", "plain", "s2" or "side_f32" (16 channels, fp32: with its chunk count)
The padding rule of plan_conv2d (a block may waste at most an eighth of its lanes) keeps 72 outputs off the 64-wide block and
24 off the 16-wide one; the channel counts that do reach a block without filling it are 120 on 64, 88 on 32, 72 on 16, 40 on 8.
"""
import ctypes
import dataclasses
import functools
import os
import sys
import time

import pytest
import torch
import torch.nn.functional as F

from test_gpu_layer_parity import Margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

DEV = "cuda:0"
LAYERS = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}
BASE_CH = (64, 128, 256, 512)


def bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _out(h, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1


# ------------------------------------------------------------------------------------------ launch classes (host only)
def direct_class(form, n, h, w, ci, co):
    from fosvos_hip import ops
    p = ops.conv2d_plan(n, h, w, ci, co, int(form[0]), int(form[4]))
    return ("direct", form, p["cob"], p["threads"], p["slices"])


def first_class(kind, n, h, w, co):
    from fosvos_hip import ops
    if kind == "first_fp32":
        return (kind, ops.conv2d_plan(n, h, w, 3, co, 7, 2, fp32_math=True)["cob"])
    return (kind, ops.conv2d_plan(n, h, w, 3, co, 7, 2)["mfma_frag_blocks"])


def mfma_class(ep, n, h, w, ci, co):
    """fosvos_conv3x3_fwd_add / _s2_fwd never split K: the tile of the plan, k_splits ignored."""
    from fosvos_hip import ops
    tile = "%dx%dx%d" % ops.conv3x3_plan(n, h, w, ci, co)["tile"]
    return ("mfma", ep, tile, ci // 32) if ep == "side_f32" else ("mfma", ep, tile)


def net_launch_classes(version, e, mfma, n, H, W):
    """The class of every conv launch of one pass (resnet_engine.forward_ops / fosvos_resnet_forward): first layer, block
    convs, 1x1 downsample convs, side_prep convs."""
    from fosvos_hip.resnet_engine import width
    out = set()
    ch = [c >> e for c in BASE_CH]
    c0 = width(ch[0], mfma)
    out.add(first_class("first_fp32" if not mfma else "first_pool_mfma" if c0 <= 32 else "first_mfma", n, H, W, c0))
    h, w = _out(_out(H, 7, 2), 3, 2), _out(_out(W, 7, 2), 3, 2)
    c = ch[0]
    for s in range(4):
        for j in range(LAYERS[version][s]):
            st = 2 if s > 0 and j == 0 else 1
            cin, cout = width(c, mfma), width(ch[s], mfma)
            if st == 2 or c != ch[s]:
                out.add(direct_class("1x1s%d" % st, n, h, w, cin, cout))      # (never on the MFMA path)
            ho, wo = _out(h, 3, st), _out(w, 3, st)
            if mfma:
                out.add(mfma_class("s2" if st == 2 else "plain", n, h, w, cin, cout))
                out.add(mfma_class("res_relu", n, ho, wo, cout, cout))
            else:
                out.add(direct_class("3x3s%d" % st, n, h, w, cin, cout))
                out.add(direct_class("3x3s1", n, ho, wo, cout, cout))
            h, w, c = ho, wo, ch[s]
        if mfma:
            out.add(mfma_class("side_f32", n, h, w, width(c, mfma), 16))
        else:
            out.add(direct_class("3x3s1_f32", n, h, w, width(c, mfma), 16))
    return out


# B1 cases.  Direct conv: class -> (ci, co, (n, h, w)); n = 2, odd sizes, a pixel count that is no multiple of the thread
# count; 2, 4, 8 slices with 3, 7 and 9 input-channel chunks.
def _direct_cases():
    big = {(64, 64): (13, 115, (139, 237), (277, 471)), (32, 64): (13, 85, (115, 195), (227, 385)),
           (16, 64): (13, 72, (89, 151), (175, 297)), (16, 256): (13, 72, (125, 213), (249, 423)),
           (8, 256): (13, 37, (125, 213), (249, 423)), (8, 64): (13, 37, (63, 107), (125, 213))}
    sliced = {2: (21, 21), 4: (53, 13), 8: (72, 40)}
    cases = {}
    for form in ("3x3s1", "3x3s2", "1x1s2"):
        for (cob, thr), (ci, co, hw1, hw2) in big.items():
            if form != "3x3s1" and cob == 64:
                continue                     # (no net launches a stride-2 conv on the 64-wide block: left out, as the guard allows)
            cases[("direct", form, cob, thr, 1)] = (ci, co, (2,) + (hw1 if form == "3x3s1" else hw2))
        for sl, (ci, co) in sliced.items():
            cases[("direct", form, 8, 64, sl)] = (ci, co, (2, 19, 27))
    cases[("direct", "3x3s1_f32", 16, 64, 1)] = (13, 16, (2, 197, 335))
    cases[("direct", "3x3s1_f32", 8, 64, 1)] = (13, 16, (2, 99, 169))
    for sl, (ci, _) in sliced.items():
        cases[("direct", "3x3s1_f32", 8, 64, sl)] = (ci, 16, (2, 19, 27))
    cases[("direct", "1x1s1", 8, 64, 4)] = (40, 160, (2, 19, 27))       # Bottleneck's widening 1x1 (no full-size net here runs it)
    return cases


DIRECT_CASES = _direct_cases()
# What test_direct_conv_class runs: one case per class, and the deepest contraction a full-width net has on this kernel
# (512 -> 512 at 3x3: K = 4608 over eight slices) on the class that takes it.
DIRECT_RUNS = {"-".join(map(str, c)): (c,) + v for c, v in DIRECT_CASES.items()}
DIRECT_RUNS["direct-3x3s1-8-64-8-K4608"] = (("direct", "3x3s1", 8, 64, 8), 512, 40, (2, 19, 27))

# First layer: class -> (co, (n, h, w)).
FIRST_CASES = {
    ("first_fp32", 64): (115, (2, 277, 471)), ("first_fp32", 32): (85, (2, 227, 385)), ("first_fp32", 16): (72, (2, 175, 297)),
    ("first_fp32", 8): (37, (2, 45, 77)),
    ("first_mfma", 1): (13, (2, 45, 77)), ("first_mfma", 2): (24, (2, 45, 77)), ("first_mfma", 3): (40, (2, 45, 77)),
    ("first_mfma", 4): (64, (2, 45, 132)),
    ("first_pool_mfma", 1): (16, (2, 45, 77)), ("first_pool_mfma", 2): (32, (2, 61, 132)),
}

# MFMA: class -> (ci, co, (n, h, w)): ragged right and bottom tiles, odd sizes (stride 2), at least two K chunks.
_BIG, _SQ, _MID, _HALF, _HALFS = (2, 57, 251), (2, 79, 231), (2, 19, 27), (2, 131, 251), (2, 33, 47)
MFMA_CASES = {}
for _ep in ("res_relu", "res", "plain", "s2"):
    MFMA_CASES[("mfma", _ep, "8x32x64")] = (64, 128, _BIG)
    MFMA_CASES[("mfma", _ep, "16x16x64")] = (64, 128, _SQ)
    MFMA_CASES[("mfma", _ep, "8x16x64")] = (96, 64, _MID)
    MFMA_CASES[("mfma", _ep, "8x32x32")] = (64, 32, _HALF)
    MFMA_CASES[("mfma", _ep, "4x16x32")] = (64, 32, _HALFS)
for _chunks in (1, 2):
    MFMA_CASES[("mfma", "side_f32", "8x32x16", _chunks)] = (32 * _chunks, 16, _HALF)
for _chunks in (1, 2, 4, 8, 16):
    MFMA_CASES[("mfma", "side_f32", "4x16x16", _chunks)] = (32 * _chunks, 16, _MID)


def case_class(cls):
    """The class the plan queries give for the shape of B1 case `cls`."""
    if cls[0] == "direct":
        ci, co, (n, h, w) = DIRECT_CASES[cls]
        return direct_class(cls[1], n, h, w, ci, co)
    if cls[0] == "mfma":
        ci, co, (n, h, w) = MFMA_CASES[cls]
        return mfma_class(cls[1], n, h, w, ci, co)
    co, (n, h, w) = FIRST_CASES[cls]
    return first_class(cls[0], n, h, w, co)


ALL_CASES = list(DIRECT_CASES) + list(FIRST_CASES) + list(MFMA_CASES)
FULL_SIZES = ((1080, 1920), (480, 854))


def _id(cls):
    return "-".join(str(v) for v in cls)


def test_launch_classes_of_the_full_size_nets_are_covered():
    """CPU guard (no device call): each B1 case selects the class it claims, and every class the full-size nets launch is
    one of them - a planner change that moves a launch of the 1080p pass onto a class no case runs fails here and names it."""
    wrong = {_id(c): case_class(c) for c in ALL_CASES if case_class(c) != c}
    assert not wrong, f"B1 cases whose shape no longer selects the class they claim: {wrong}"
    need = {}
    for version in (18, 34):
        for e in range(4):
            for mfma in (True, False):
                for n in (1, 2):
                    for H, W in FULL_SIZES:
                        for c in net_launch_classes(version, e, mfma, n, H, W):
                            need.setdefault(c, (version, e, mfma, n, H, W))
    missing = {c: v for c, v in need.items() if c not in set(ALL_CASES)}
    assert not missing, ("launch classes of the full-size nets no GPU case runs (class: first net that launches it as "
                         f"(version, scale_down_exponent, mfma, frames, H, W)): {missing}")


# ------------------------------------------------------------------------------------------ B1: one case per class
def _nhwc(x_nchw, c_pad=None):
    n, c, h, w = x_nchw.shape
    out = torch.zeros((n, h, w, c_pad or c), dtype=torch.bfloat16)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out.to(DEV)


def _nchw(y, c):
    return y[..., :c].permute(0, 3, 1, 2).contiguous().cpu().double()


def _ru8(c):
    return (c + 7) // 8 * 8


@functools.lru_cache(maxsize=8)
def _operands(ci, co, k, stride, n, h, w):
    """bf16-rounded activations and weights, fp32 bias, the float64 conv + bias and a bf16 addend of its shape."""
    g = torch.Generator().manual_seed(ci * 131 + co * 7 + k * 3 + stride + h)
    x = bf(torch.randn(n, ci, h, w, generator=g))
    wt = bf(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5)
    bias = 0.3 * torch.randn(co, generator=g)
    term = F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=k // 2)
    add = bf(torch.randn(term.shape, generator=g))
    return x, wt, bias, term, add


@pytest.mark.gpu
@pytest.mark.parametrize("run", list(DIRECT_RUNS))
def test_direct_conv_class(run):
    from fosvos_hip import ops
    cls, ci, co, (n, h, w) = DIRECT_RUNS[run]
    _, form, cob, threads, slices = cls
    k, stride, f32 = int(form[0]), int(form[4]), form.endswith("_f32")
    assert direct_class(form, n, h, w, ci, co) == cls
    plan = ops.conv2d_plan(n, h, w, ci, co, k, stride)
    npix = n * _out(h, k, stride) * _out(w, k, stride)
    assert npix % threads != 0 and (slices == 1 or (_ru8(ci) // 8) % slices != 0 or run.endswith("K4608"))
    print(f"[{run}] {ci}->{co} @ {n}x{h}x{w}: plan {plan}, {npix} pixels, {_ru8(ci) // 8} input chunks")
    x, wt, bias, term, add = _operands(ci, co, k, stride, n, h, w)
    packed, pbias = ops.pack_conv2d_bn(wt.to(DEV), bias.to(DEV), None)
    M = Margins(run)
    xd = _nhwc(x, _ru8(ci))
    for relu, with_add in ((False, False),) if f32 else ((True, True), (False, True), (True, False), (False, False)):
        ref = term + add.double() if with_add else term
        ref = F.relu(ref) if relu else ref
        addd = _nhwc(add, _ru8(co)) if with_add else None
        y = ops.conv2d_fwd(xd, packed, pbias, ci, co, k, stride, relu, addd, out_f32=f32)
        y2 = ops.conv2d_fwd(xd, packed, pbias, ci, co, k, stride, relu, addd, out_f32=f32)
        torch.cuda.synchronize()
        tag = ("relu" if relu else "lin") + ("+add" if with_add else "")
        assert y.dtype == (torch.float32 if f32 else torch.bfloat16) and y.shape == (n, *ref.shape[2:], _ru8(co))
        M.exact(tag, "pad ch", y[..., co:], torch.zeros_like(y[..., co:]))
        M.exact(tag, "2nd launch", y.view(torch.int32 if f32 else torch.int16), y2.view(torch.int32 if f32 else torch.int16))
        if f32:
            M.rel(tag, "f32", _nchw(y, co), ref, 2e-5)
        else:
            M.bf16(tag, _nchw(y, co), ref)
    M.report()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(FIRST_CASES), ids=_id)
def test_first_layer_class(cls):
    """k_conv7x7s2_first<COB> on the fp32 frame and fp32 weights; the MFMA forms on the frame and weights rounded to bf16
    (the fused form: the pool of the rounded map, exact because rounding is monotone)."""
    from fosvos_hip import ops
    kind, _ = cls
    co, (n, h, w) = FIRST_CASES[cls]
    assert case_class(cls) == cls
    print(f"[{_id(cls)}] 3->{co} @ {n}x{h}x{w}: plan {ops.conv2d_plan(n, h, w, 3, co, 7, 2, fp32_math=kind == 'first_fp32')}")
    g = torch.Generator().manual_seed(co * 17 + h)
    x = torch.randn(n, 3, h, w, generator=g)
    wt = torch.randn(co, 3, 7, 7, generator=g) * (2.0 / 147) ** 0.5
    bias = 0.3 * torch.randn(co, generator=g)
    if kind != "first_fp32":
        x, wt = bf(x), bf(wt)
    # BatchNorm terms that fold to scale 1 exactly and shift = bias: weight 1, mean 0, variance 1, eps 0
    one, zero = torch.ones(co), torch.zeros(co)
    packed, pbias = ops.pack_conv7x7_bn(wt.to(DEV), (one.to(DEV), bias.to(DEV), zero.to(DEV), one.to(DEV), 0.0))
    ref = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), stride=2, padding=3))
    M = Margins(_id(cls))
    xd = x.to(DEV)
    if kind == "first_pool_mfma":
        run = lambda: ops.conv7x7s2_pool_first_fwd(xd, packed, pbias, co)
        ref = F.max_pool2d(ref, 3, 2, 1)
    else:
        run = lambda: ops.conv7x7s2_first_fwd(xd, packed, pbias, co, relu=True, fp32_math=kind == "first_fp32")
    y, y2 = run(), run()
    torch.cuda.synchronize()
    assert y.shape == (n, *ref.shape[2:], _ru8(co))
    M.exact("out", "pad ch", y[..., co:], torch.zeros_like(y[..., co:]))
    M.exact("out", "2nd launch", y.view(torch.int16), y2.view(torch.int16))
    M.bf16("out", _nchw(y, co), ref)
    M.report()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(MFMA_CASES), ids=_id)
def test_mfma_epilogue_class(cls):
    from fosvos_hip import ops
    ep = cls[1]
    ci, co, (n, h, w) = MFMA_CASES[cls]
    assert case_class(cls) == cls
    print(f"[{_id(cls)}] {ci}->{co} @ {n}x{h}x{w}: plan {ops.conv3x3_plan(n, h, w, ci, co)} (run unsplit), {ci // 32} K chunks")
    x, wt, bias, term, add = _operands(ci, co, 3, 1, n, h, w)
    packed, _ = ops.pack_conv3x3_weights(wt.to(DEV), want_fwd=True, want_dgrad=False)
    xd, bd = _nhwc(x), bias.to(DEV)
    M = Margins(_id(cls))
    if ep in ("res_relu", "res"):
        addd = _nhwc(add)
        run = lambda: ops.conv3x3_fwd_add(xd, packed, bd, ci, co, ep == "res_relu", addd)
        ref = term + add.double()
        ref = F.relu(ref) if ep == "res_relu" else ref
    elif ep == "plain":
        run = lambda: ops.conv3x3_fwd_add(xd, packed, bd, ci, co, True, None)
        ref = F.relu(term)
    elif ep == "s2":
        run = lambda: ops.conv3x3_s2_fwd(xd, packed, bd, ci, co, True)
        ref = F.relu(term[:, :, ::2, ::2])               # conv(stride 2, pad 1) = every other pixel of conv(stride 1, pad 1)
    else:
        run = lambda: ops.conv3x3_fwd_add(xd, packed, bd, ci, co, False, None, out_f32=True)
        ref = term
    y, y2 = run(), run()
    torch.cuda.synchronize()
    assert y.shape == (n, *ref.shape[2:], co) and y.dtype == (torch.float32 if ep == "side_f32" else torch.bfloat16)
    M.exact(ep, "2nd launch", y.view(torch.int32 if ep == "side_f32" else torch.int16),
            y2.view(torch.int32 if ep == "side_f32" else torch.int16))
    if ep == "side_f32":
        M.rel(ep, "f32", _nchw(y, co), ref, 2e-5)
    elif ep in ("res_relu", "res"):
        M.bf16_two(ep, _nchw(y, co), ref, term)
    else:
        M.bf16(ep, _nchw(y, co), ref)
    M.report()


# ------------------------------------------------------------------------------------------ B3: the head across column blocks
def _head_case(h, w, n, seed):
    from oracle import osvos_resnet_ref as R
    g = torch.Generator().manual_seed(seed)
    sizes, (hh, ww) = [], (_out(h, 7, 2), _out(w, 7, 2))
    for _ in range(4):
        hh, ww = _out(hh, 3, 2), _out(ww, 3, 2)
        sizes.append((hh, ww))
    side = [torch.randn(n, 16, a, b, generator=g) for a, b in sizes]
    sd = R.make_state_dict(18, 3, seed=5)
    return side, sd


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(4, 640), (5, 641), (37, 1281), (9, 1931), (1080, 1920)])
def test_deconv_head_across_column_blocks(h, w):
    """k_deconv_head owns 4 rows x 640 columns per workgroup: frames of one, two, three and four column blocks (window origin
    Xb / f for blockIdx.x > 0, column stride 64 p up to p = 9), heights that are no multiple of 4, two frames, with and
    without the side outputs, against conv_transpose2d + centre crop + concat + 1x1 fuse in float64 (frame by frame)."""
    from fosvos_hip import ops
    from oracle import osvos_resnet_ref as R
    n = 2
    side, sd = _head_case(h, w, n, h * 1000 + w)
    D = {k: v.double() for k, v in sd.items()}
    fused_ref, outs_ref = [], [[] for _ in range(4)]
    for i in range(n):
        ups = []
        for s in range(4):
            f = 4 << s
            x = side[s][i:i + 1].double()
            ups.append(R.center_crop(F.conv_transpose2d(x, D["upscale_side_prep.%d.weight" % s], stride=f), h, w))
            dsn = F.conv2d(x, D["score_dsn.%d.weight" % s], D["score_dsn.%d.bias" % s])
            outs_ref[s].append(R.center_crop(F.conv_transpose2d(dsn, D["upscale_score_dsn.%d.weight" % s], stride=f), h, w))
        fused_ref.append(F.conv2d(torch.cat(ups, 1), D["layer_fuse.weight"], D["layer_fuse.bias"]))
        del ups
    fused_ref = torch.cat(fused_ref)
    outs_ref = [torch.cat(o) for o in outs_ref]
    fuse_w, fuse_b = sd["layer_fuse.weight"], sd["layer_fuse.bias"]
    filt = [torch.einsum("o,iokl->kli", fuse_w[0, 16 * s:16 * s + 16, 0, 0], sd["upscale_side_prep.%d.weight" % s]).contiguous().to(DEV)
            for s in range(4)]
    filt1 = [sd["upscale_score_dsn.%d.weight" % s][0, 0].contiguous().to(DEV) for s in range(4)]
    dsn_w = torch.cat([sd["score_dsn.%d.weight" % s].reshape(1, 16) for s in range(4)]).to(DEV)
    dsn_b = torch.cat([sd["score_dsn.%d.bias" % s] for s in range(4)]).to(DEV)
    side_nhwc = [t.permute(0, 2, 3, 1).contiguous().to(DEV) for t in side]
    fused, outs = ops.deconv_head_fwd(side_nhwc, [4, 8, 16, 32], filt, filt1, dsn_w, dsn_b, fuse_b.to(DEV), h, w, True)
    fused2, none = ops.deconv_head_fwd(side_nhwc, [4, 8, 16, 32], filt, None, None, None, fuse_b.to(DEV), h, w, False)
    torch.cuda.synchronize()
    assert none is None
    M = Margins(f"head {n}x{h}x{w}")
    M.exact("fused", "no side out", fused2, fused)

    def head(layer, a, ref):
        M.add(layer, "1e-4", (a.cpu().double() - ref).abs().max().item() / (1e-4 * max(1.0, ref.abs().max().item())))

    head("fused", fused, fused_ref)
    for s in range(4):
        head(f"side_out[{s}]", outs[s], outs_ref[s])
    # ... and per column block, so that a wrong block cannot hide behind the frame's maximum
    for b in range((w + 639) // 640):
        head(f"fused cols {640 * b}..", fused[..., 640 * b:640 * b + 640], fused_ref[..., 640 * b:640 * b + 640])
    M.report()


# ------------------------------------------------------------------------------------------ B4: the pool as a general pool
@pytest.mark.gpu
@pytest.mark.parametrize("c", [8, 24, 64])
def test_maxpool3x3s2_on_negative_values(c):
    """fosvos_maxpool3x3s2_fwd against F.max_pool2d(3, 2, 1), bit for bit, on signed inputs and on maps that are negative
    everywhere (a pad value of 0 instead of -inf would win every border window there)."""
    from fosvos_hip import ops
    g = torch.Generator().manual_seed(c)
    M = Margins(f"pool c={c}")
    for h in (1, 2, 7, 10):
        for w in (1, 2, 9, 12):
            for kind in ("signed", "negative"):
                x = bf(torch.randn(2, c, h, w, generator=g))
                if kind == "negative":
                    x = bf(-x.abs() - 0.5)
                y = ops.maxpool3x3s2_fwd(_nhwc(x))
                torch.cuda.synchronize()
                want = F.max_pool2d(x, 3, 2, 1)
                assert y.shape == (2, *want.shape[2:], c)
                M.exact(f"{h}x{w}", kind, y.float().permute(0, 3, 1, 2).cpu(), want)
    M.report()


# ------------------------------------------------------------------------------------------ B5: the packed images
def unpack_conv2d_image(packed, ci, co, k):
    """fosvos_pack_conv2d_bn image, uint32 [ci chunks of 8][k * k][4 pairs][Cop] (low half: the even input channel), as fp32
    [Cop, 8 * chunks, k, k] with its padded rows and columns."""
    cic, cop = _ru8(ci) // 8, _ru8(co)
    words = packed.cpu()[:cic * k * k * 4 * cop].view(cic, k * k, 4, cop)
    lo = (words << 16).view(torch.float32)                       # bf16 bits in the upper half of an fp32
    hi = (words & -65536).view(torch.float32)
    wt = torch.stack([lo, hi], dim=3)                            # [chunk, tap, pair, half, co]
    return wt.permute(4, 0, 2, 3, 1).reshape(cop, cic * 8, k, k).contiguous()


def _bn(c, g):
    return (0.7 + 0.6 * torch.rand(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g),
            0.5 + torch.rand(c, generator=g), 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("ci,co", [(13, 21), (59, 16), (64, 72)])
def test_packed_conv2d_image(ci, co, k):
    """Every element of the image within one bf16 ulp of the float64 fold w * bn_w / sqrt(var + eps), padded rows and
    columns exact zeros; the folded bias to fp32 rounding: s carries a division (2.5 ulp), a square root (1 ulp) and one
    rounding, mean * s and the difference one each - 2^-21 of (|bn_bias| + |mean s|) covers them."""
    from fosvos_hip import ops
    g = torch.Generator().manual_seed(ci * 100 + co + k)
    wt = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
    bn = _bn(co, g)
    packed, bias = ops.pack_conv2d_bn(wt.to(DEV), None, tuple(t.to(DEV) for t in bn[:4]) + (bn[4],))
    torch.cuda.synchronize()
    s = bn[0].double() / torch.sqrt(bn[3].double() + bn[4])
    fold = wt.double() * s.view(-1, 1, 1, 1)
    got = unpack_conv2d_image(packed, ci, co, k)
    M = Margins(f"pack {ci}->{co} k{k}")
    M.exact("image", "pad rows", got[co:], torch.zeros_like(got[co:]))
    M.exact("image", "pad columns", got[:, ci:], torch.zeros_like(got[:, ci:]))
    ulp = torch.exp2(torch.floor(torch.log2(fold.abs().clamp_min(1e-30))) - 7)
    M.add("image", "bf16 ulp", ((got[:co, :ci].double() - fold).abs() / ulp).max())
    b_ref = bn[1].double() - bn[2].double() * s
    b_tol = 2.0 ** -21 * (bn[1].double().abs() + (bn[2].double() * s).abs())
    M.add("bias", "fp32", ((bias.cpu()[:co].double() - b_ref).abs() / b_tol).max())
    M.exact("bias", "pad", bias.cpu()[co:], torch.zeros_like(bias.cpu()[co:]))
    M.report()


# ------------------------------------------------------------------------------------------ B6: the pass on a poisoned arena
NETS = [(0, True), (2, True), (2, False)]   # ResNet-18: (scale_down_exponent, resnet_mfma)


def _make_net(e, mfma, seed=12):
    from networks.osvos_resnet import OSVOS_RESNET
    from oracle import osvos_resnet_ref as R
    net = OSVOS_RESNET(pretrained=False, version=18, scale_down_exponent=e)
    net.load_state_dict(R.make_state_dict(18, e, seed=seed))
    net = net.to(DEV).eval()
    net.options = dataclasses.replace(net.options, resnet_mfma=mfma, resnet_fuse_first=True, resnet_aux=False)
    return net


def _frame(n, h, w, seed=7):
    return (50.0 * torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(seed))).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 1080, 1920), (2, 217, 389)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("e,mfma", NETS)
def test_native_pass_on_a_poisoned_arena(e, mfma, shape):
    """fosvos_resnet_forward on an arena of fosvos_resnet_arena_bytes + 4096 bytes, every byte 0xFF (NaN in bf16 and fp32):
    finite outputs, the bits of the op-by-op loop and of a run on a zeroed arena, the 4096 bytes behind the arena untouched -
    one stream and with the side_prep / downsample convs on the auxiliary stream."""
    from fosvos_hip import lib, resnet_engine
    net = _make_net(e, mfma)
    x = _frame(*shape)
    want = resnet_engine.forward_ops(net, net._plan, x)              # (packs the weights)
    need = lib().fosvos_resnet_arena_bytes(ctypes.byref(net._plan.c_net), *shape)
    assert need > 0
    M = Margins(f"arena e={e} mfma={int(mfma)} {'x'.join(map(str, shape))}")
    for aux in (False, True):
        net.options = dataclasses.replace(net.options, resnet_aux=aux)
        for fill in (255, 0):
            arena = torch.full((need + 4096,), fill, dtype=torch.uint8, device=DEV)
            arena[need:] = 255
            net._plan.arena = arena
            outs = net(x)
            torch.cuda.synchronize()
            assert net._plan.arena is arena
            tag = f"{'aux' if aux else 'one stream'} 0x{fill:02X}"
            M.add(tag, "finite", 0.0 if all(bool(torch.isfinite(t).all()) for t in outs) else float("inf"))
            for i, (a, b) in enumerate(zip(outs, want)):
                M.exact(tag, f"out[{i}] vs ops", a, b)
            M.exact(tag, "guard bytes", arena[need:], torch.full_like(arena[need:], 255))
            del arena, outs
    M.report()


# ------------------------------------------------------------------------------------------ B7: teacher-forced layers at 1080p
def _folded(conv, bn, ci_p, co_p):
    """What resnet_engine._Conv hands to the MFMA packing: the conv padded to the stored widths, BatchNorm folded by
    ops.fold_conv_bn (fp32); the kernel reads its bf16 rounding."""
    from fosvos_hip import ops
    from fosvos_hip.resnet_engine import _pad_to
    k = conv.kernel_size[0]
    w = torch.zeros((co_p, ci_p, k, k), dtype=torch.float32, device=conv.weight.device)
    w[:conv.out_channels, :conv.in_channels] = conv.weight.detach()
    bnp = None
    if bn is not None:
        bnp = (_pad_to(bn.weight.detach(), co_p), _pad_to(bn.bias.detach(), co_p), _pad_to(bn.running_mean, co_p),
               _pad_to(bn.running_var, co_p, 1.0), bn.eps)
    cb = None if conv.bias is None else _pad_to(conv.bias.detach(), co_p)
    folded, _ = ops.fold_conv_bn(w.contiguous(), cb, bnp)
    return bf(folded.cpu())


def _first_weights(plan, mfma):
    """The first layer's weights as the kernel reads them: the fp32 image [tap * 3 + ci][Cop], or the bf16 MFMA fragments
    [k-step 6][k-group 4][channel NC][8] over K = 8 rows x 24 (kx-major, channel-minor) behind it."""
    cop = plan.c0
    img = plan.first[0].cpu()
    if not mfma:
        return img[:147 * cop].view(49, 3, cop).permute(2, 1, 0).reshape(cop, 3, 7, 7).contiguous()
    nc = (cop + 15) // 16 * 16
    frag = img[147 * cop + 64:].view(torch.bfloat16)[:24 * nc * 8].float().view(24, nc, 8)
    return frag.permute(1, 0, 2).reshape(nc, 8, 24)[:cop, :7, :21].reshape(cop, 7, 7, 3).permute(0, 3, 1, 2).contiguous()


def _check_conv(M, layer, conv, conv_mod, bn_mod, x, y, relu, addend=None, f32=False):
    """One launch of the pass against float64 from its own input: conv = resnet_engine._Conv, x / y / addend = the NHWC
    device tensors it read and wrote."""
    from fosvos_hip import ops
    xin = x.permute(0, 3, 1, 2).cpu().double()
    if conv.kind:
        wt = _folded(conv_mod, bn_mod, conv.ci, conv.co)
        plan = ops.conv3x3_plan(x.shape[0], x.shape[1], x.shape[2], conv.ci, conv.co)["tile"]
    else:
        wt = unpack_conv2d_image(conv.packed, conv.ci, conv.co, conv.k)[:, :conv.ci]
        plan = ops.conv2d_plan(x.shape[0], x.shape[1], x.shape[2], conv.ci, conv.co, conv.k, conv.stride)
    cop = wt.shape[0]
    term = F.conv2d(xin, wt.double(), conv.bias.cpu()[:cop].double(), stride=conv.stride, padding=conv.k // 2)
    ref = term if addend is None else term + addend.permute(0, 3, 1, 2).cpu().double()
    ref = F.relu(ref) if relu else ref
    got = y.permute(0, 3, 1, 2).cpu().double()
    assert got.shape == ref.shape, (layer, got.shape, ref.shape)
    name = f"{layer} {conv.ci}->{conv.co} k{conv.k}s{conv.stride} {'mfma' if conv.kind else 'direct'} {plan}"
    if f32:
        M.rel(name, "f32", got, ref, 2e-5)
    elif conv.kind and addend is not None:
        M.bf16_two(name, got, ref, term)
    else:
        M.bf16(name, got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("e,mfma", NETS)
def test_teacher_forced_layers_at_1080p(e, mfma):
    """The layer loop of resnet_engine.forward_ops on one 1080x1920 frame, every launch checked on its own: the padded
    channels are part of the comparison (zero weights, zero bias: exact zeros in the reference as well)."""
    from fosvos_hip import ops
    t0 = time.time()
    net = _make_net(e, mfma)
    plan = net._plan
    x = _frame(1, 1080, 1920)
    M = Margins(f"1080p e={e} mfma={int(mfma)}")
    with torch.no_grad():
        plan.refresh(net)
        w1 = _first_weights(plan, mfma)
        frame = x.cpu().double() if not mfma else bf(x.cpu()).double()
        ref = F.relu(F.conv2d(frame, w1.double(), plan.first[1].cpu()[:plan.c0].double(), stride=2, padding=3))
        if plan.fuse_first:
            y = ops.conv7x7s2_pool_first_fwd(x, plan.first[0], plan.first[1], plan.c0)
            M.bf16(f"first+pool 3->{plan.c0}", y.permute(0, 3, 1, 2).cpu().double(), F.max_pool2d(ref, 3, 2, 1))
        else:
            y0 = ops.conv7x7s2_first_fwd(x, plan.first[0], plan.first[1], plan.c0, relu=True, fp32_math=not mfma)
            M.bf16(f"first 3->{plan.c0}", y0.permute(0, 3, 1, 2).cpu().double(), ref)
            y = ops.maxpool3x3s2_fwd(y0)
            M.exact("pool", "maxpool", y.float().permute(0, 3, 1, 2).cpu(),
                    F.max_pool2d(y0.float().permute(0, 3, 1, 2).cpu(), 3, 2, 1))
        del ref, frame
        sides = []
        for s, (blocks, side) in enumerate(zip(plan.stages, plan.side)):
            for j, blk in enumerate(blocks):
                mod = net.layer_stages[s][j]
                tag = f"s{s + 1}b{j}"
                res = y
                if blk.down is not None:
                    res = blk.down(y, relu=False)
                    _check_conv(M, tag + ".down", blk.down, mod.downsample[0], mod.downsample[1], y, res, False)
                mid = blk.convs[0](y, relu=True)
                _check_conv(M, tag + ".conv1", blk.convs[0], mod.conv1, mod.bn1, y, mid, True)
                out = blk.convs[1](mid, relu=True, addend=res)
                _check_conv(M, tag + ".conv2", blk.convs[1], mod.conv2, mod.bn2, mid, out, True, addend=res)
                y = out
            sides.append(side(y, relu=False, out_f32=True))
            _check_conv(M, f"side{s + 1}", side, net.side_prep[s], None, y, sides[-1], False, f32=True)
        torch.cuda.synchronize()
    print(f"[1080p e={e} mfma={int(mfma)}] {time.time() - t0:.1f} s")
    M.report()
