"""The contraction kernels of the VGG path on exactly summable operands (tests/exact_cases.py), bit for bit against the CPU:
the MFMA forward tiles, the persistent forward kernel, the split-K epilogue, the data gradient and its fused epilogues, both
weight-gradient kernels and conv1_1.  Run with ``pytest -m gpu``.

Every operand is an integer (or a dyadic rational) that the kernel's input format holds, and every partial sum stays below
2^24 units, so an fp32 accumulation is exact in any order.  The tile, the K split, the persistent or the igemm kernel, a fold
or a slab reduction therefore cannot matter: each kernel class must produce THE bits, the round-to-nearest-even image of an
integer the CPU computes exactly (tests/test_exact_cases_cpu.py checks the reference side, and that the operands separate
round-to-nearest-even from truncation and from round-half-away).  Every assertion here is an equality; none carries a
tolerance.  A failure prints how many elements differ, the first differing index, the two values, and whether the kernel's
values are the truncated or the half-away image of the exact value - which usually names the bug.

What the tolerance tests of tests/test_gpu_ops.py cannot see and these do: a truncating or half-away output convert (their bar
is 2^-8, round-to-nearest-even errs by 2^-9); the fused and the split-K epilogue disagreeing by a rounding in the sequence
round, mask, add, round; a weight-gradient error below 5e-5 of the largest entry (one product counted twice, a halo pixel taken
at weight 0).

The matrix instructions on exact operands: the cases rest on v_mfma_f32_16x16x32_bf16, v_mfma_f32_32x32x16_bf16 and
v_dot2c_f32_bf16 returning the exact sum when every partial sum is exact in 24 bits.  Measured on an MI355X with these
cases: they do - see the section on exact operands in DESIGN.md for what was run."""
import os
import sys

import pytest
import torch

import exact_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from fosvos_hip import ops as _ops
    return _ops


def _ids(cases):
    return [c.id for c in cases]


def nhwc_bf16(t, c_pad=None):
    """fp32 NCHW (cpu) -> bf16 NHWC (gpu), zero channels up to c_pad (test plumbing; the values are bf16-exact)."""
    t = t.permute(0, 2, 3, 1).contiguous()
    if c_pad is not None and c_pad != t.shape[3]:
        t = torch.cat([t, torch.zeros(*t.shape[:3], c_pad - t.shape[3])], 3)
    return t.to(torch.bfloat16).to(DEV)


def nchw(t):
    """NHWC (gpu) -> fp32 NCHW (cpu)."""
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


class Report:
    """Collects the mismatches of one case, so that a failure lists every form that differs."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def same(self, what, got, want, pre=None):
        msg = E.compare_bits(got, want, pre)
        if msg is not None:
            self.bad.append(f"{what}: {msg}")

    def done(self):
        assert not self.bad, f"[{self.tag}] " + " || ".join(self.bad)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_forward_exact(ops, c):
    """conv3x3_fwd with bias and ReLU and in the linear form (no bias, no ReLU), conv3x3_fwd_pool on the bf16 cases: y =
    bf16(relu?(conv + b)), the pooled map the ceil-mode pool of it; the 16-channel fp32 output is the exact value itself."""
    n, h, w, ci, co = c.shape
    assert E.fwd_class(ops, c) == c.cls
    x, wt, b = E.fwd_operands(c)
    ref = E.fwd_reference(x, wt, b)
    wf, _ = ops.pack_conv3x3_weights(wt.to(DEV))
    xd, bd = nhwc_bf16(x), b.to(DEV)
    r = Report(f"{c.id} {c.shape} {c.cls}")
    if co == 16:
        r.same("fp32 conv + b", nchw(ops.conv3x3_fwd(xd, wf, bd, ci, co, relu=False, out_f32=True)), ref["bias"])
        r.same("fp32 conv", nchw(ops.conv3x3_fwd(xd, wf, None, ci, co, relu=False, out_f32=True)), ref["linear"])
        r.done()
        return
    y = nchw(ops.conv3x3_fwd(xd, wf, bd, ci, co, relu=True))
    r.same("relu(conv + b)", y, E.bf(ref["relu"]), ref["relu"])
    r.same("linear", nchw(ops.conv3x3_fwd(xd, wf, None, ci, co, relu=False)), E.bf(ref["linear"]), ref["linear"])
    y2, yp = ops.conv3x3_fwd_pool(xd, wf, bd, ci, co, relu=True)
    r.same("fwd_pool y", nchw(y2), E.bf(ref["relu"]), ref["relu"])
    r.same("fwd_pool pooled", nchw(yp), E.pool(E.bf(ref["relu"])))
    y3, yp3 = ops.conv3x3_fwd_pool(xd, wf, bd, ci, co, relu=False)  # negative values through the pool
    r.same("fwd_pool y, no ReLU", nchw(y3), E.bf(ref["bias"]), ref["bias"])
    r.same("fwd_pool pooled, no ReLU", nchw(yp3), E.pool(E.bf(ref["bias"])))
    r.done()


# ------------------------------------------------------------------------------------------ data gradient
def _dgrad_device_operands(ops, c):
    n, h, w, ci, co = c.shape
    dy, wt, src, add = E.dgrad_operands(c)
    _, wd = ops.pack_conv3x3_weights(wt.to(DEV))
    dyd = nhwc_bf16(dy, (co + 31) // 32 * 32)  # the side form: 16 real channels in a 32-wide gradient image
    return dy, wt, src, add, wd, dyd


PLAIN = [c for c in E.DGRAD_CASES if c.kind == "plain"]
UNPOOL = [c for c in E.DGRAD_CASES if c.kind == "unpool"]


@pytest.mark.parametrize("c", PLAIN, ids=_ids(PLAIN))
def test_dgrad_exact(ops, c):
    """conv3x3_dgrad plain, with relu_src, with relu_bits, with the addend aliased to out, with mask and addend together (both
    mask forms): t = bf16(sum); t = mask ? t : 0; t = t + addend in fp32; y = bf16(t) - the sequence the fused epilogue and
    k_splitk_epilogue document.  The mask as bits without an addend takes the persistent kernel where the case says so; every
    entry point and class that runs the same operands gives the same bits, since each equals the reference."""
    n, h, w, ci, co = c.shape
    assert E.dgrad_class(ops, c) == c.cls and E.dgrad_bits_class(ops, c) == getattr(c, "bits_cls", c.cls)
    dy, wt, src, add, wd, dyd = _dgrad_device_operands(ops, c)
    s = E.dgrad_sum(dy, wt)
    mask = src > 0
    srcd, addd = nhwc_bf16(src), nhwc_bf16(add)
    bits = E.relu_bits(srcd)
    r = Report(f"{c.id} {c.shape} {c.cls}")
    want, pre = E.dgrad_epilogue(s)
    r.same("plain", nchw(ops.conv3x3_dgrad(dyd, wd, ci, co)), want, pre)
    want, pre = E.dgrad_epilogue(s, mask)
    by_src = ops.conv3x3_dgrad(dyd, wd, ci, co, relu_src=srcd)
    by_bits = ops.conv3x3_dgrad(dyd, wd, ci, co, relu_bits=bits)
    r.same("relu_src", nchw(by_src), want, pre)
    r.same(f"relu_bits ({getattr(c, 'bits_cls', c.cls)})", nchw(by_bits), want, pre)
    r.same("relu_bits against relu_src", by_bits, by_src)
    want, pre = E.dgrad_epilogue(s, None, add)
    out = addd.clone()
    got = ops.conv3x3_dgrad(dyd, wd, ci, co, addend=out, out=out)
    assert got.data_ptr() == out.data_ptr()
    r.same("addend aliased to out", nchw(got), want, pre)
    want, pre = E.dgrad_epilogue(s, mask, add)
    out = addd.clone()
    by_src = ops.conv3x3_dgrad(dyd, wd, ci, co, relu_src=srcd, addend=out, out=out)
    r.same("relu_src + addend (aliased)", nchw(by_src), want, pre)
    by_bits = ops.conv3x3_dgrad(dyd, wd, ci, co, relu_bits=bits, addend=addd)
    r.same("relu_bits + addend", nchw(by_bits), want, pre)
    r.same("relu_bits + addend against relu_src + addend", by_bits, by_src)
    r.done()


@pytest.mark.parametrize("c", UNPOOL, ids=_ids(UNPOOL))
def test_dgrad_unpool_exact(ops, c):
    """conv3x3_dgrad_unpool on the three tiles that fuse the pool backward and on the 32-channel shape that runs two passes:
    the addend is the exactly routed pool gradient (first maximum in scan order, ReLU mask of the producer; the windows are
    full of ties).  The two passes on the device (maxpool_bwd, then conv3x3_dgrad with it as the addend) give the same bits."""
    n, h, w, ci, co = c.shape
    assert E.dgrad_class(ops, c) == c.cls
    dy, wt, src, dpool, wd, dyd = _dgrad_device_operands(ops, c)
    routed = E.pool_backward(src, dpool)
    want, pre = E.dgrad_epilogue(E.dgrad_sum(dy, wt), src > 0, routed)
    srcd, dpoold = nhwc_bf16(src), nhwc_bf16(dpool)
    r = Report(f"{c.id} {c.shape} {c.cls}")
    got = ops.conv3x3_dgrad_unpool(dyd, wd, ci, co, srcd, dpoold)
    r.same("dgrad_unpool", nchw(got), want, pre)
    routed_d = ops.maxpool_bwd(srcd, dpoold, relu_mask=True)
    r.same("maxpool_bwd", nchw(routed_d), routed)
    two = ops.conv3x3_dgrad(dyd, wd, ci, co, relu_src=srcd, addend=routed_d)
    r.same("two passes", nchw(two), want, pre)
    r.same("dgrad_unpool against the two passes", got, two)
    r.done()


# ------------------------------------------------------------------------------------------ weight and bias gradient
@pytest.mark.parametrize("c", E.WGRAD_CASES, ids=_ids(E.WGRAD_CASES))
def test_wgrad_exact(ops, c):
    """conv3x3_wgrad (slabs + reduction), conv3x3_wgrad_one_call, and accumulate=True onto integer prefills: the exact integers."""
    n, h, w, ci, co = c.shape
    x, dy, pw, pb = E.wgrad_operands(c)
    dw_ref, db_ref = E.wgrad_reference(x, dy)
    xd, dyd = nhwc_bf16(x), nhwc_bf16(dy, (co + 31) // 32 * 32)
    r = Report(f"{c.id} {c.shape}: {c.cls}")
    dw, db = ops.conv3x3_wgrad(xd, dyd, ci, co)
    r.same("dw", dw.cpu(), dw_ref)
    r.same("db", db.cpu(), db_ref)
    dw1, db1 = ops.conv3x3_wgrad_one_call(xd, dyd, ci, co)
    r.same("one_call dw", dw1.cpu(), dw_ref)
    r.same("one_call db", db1.cpu(), db_ref)
    dw2, db2 = ops.conv3x3_wgrad(xd, dyd, ci, co, dw=pw.to(DEV), db=pb.to(DEV), accumulate=True)
    r.same("accumulate dw", dw2.cpu(), dw_ref + pw)
    r.same("accumulate db", db2.cpu(), db_ref + pb)
    dw3, none = ops.conv3x3_wgrad(xd, dyd, ci, co, with_bias=False)
    assert none is None
    r.same("dw without the bias gradient", dw3.cpu(), dw_ref)
    r.done()


# ------------------------------------------------------------------------------------------ conv1_1
@pytest.mark.parametrize("c", E.FIRST_FWD_CASES, ids=_ids(E.FIRST_FWD_CASES))
def test_first_forward_exact(ops, c):
    """conv3x3_first_fwd on the fp32 frame and fp32 weights (the kernel splits both into two bf16 terms; on the "split" operands
    all four term products contribute and are exact): y = bf16(relu(conv + b)), the bits (y > 0) of the exact value."""
    frame, wt, b = E.first_fwd_operands(c)
    pre = E.first_fwd_reference(frame, wt, b)
    y, bits = ops.conv3x3_first_fwd(frame.to(DEV), wt.to(DEV), b.to(DEV), want_bits=True)
    r = Report(f"{c.id} {c.shape}")
    r.same("y", nchw(y), E.bf(pre), pre)
    r.same("bits", bits.cpu(), E.relu_bits(pre.permute(0, 2, 3, 1).contiguous()))
    r.same("y without the bits", nchw(ops.conv3x3_first_fwd(frame.to(DEV), wt.to(DEV), b.to(DEV))), E.bf(pre), pre)
    r.done()


@pytest.mark.parametrize("c", E.FIRST_WGRAD_CASES, ids=_ids(E.FIRST_WGRAD_CASES))
def test_first_wgrad_exact(ops, c):
    """conv3x3_first_wgrad: exact on bf16(frame) - the frame is rounded to nearest even inside the kernel (a frame with ties
    among values of more than 8 significant bits), and on more than 512 tiles."""
    frame, dy = E.first_wgrad_operands(c)
    dw_ref, db_ref = E.first_wgrad_reference(frame, dy)
    dw, db = ops.conv3x3_first_wgrad(frame.to(DEV), nhwc_bf16(dy))
    r = Report(f"{c.id} {c.shape}: {c.cls}")
    r.same("dw", dw.cpu(), dw_ref)
    r.same("db", db.cpu(), db_ref)
    if not r.bad:
        r.done()
        return
    for name, rounding in (("truncation", E.bf16_trunc), ("half-away", E.bf16_half_away), ("no rounding", lambda t: t)):
        if torch.equal(dw.cpu(), E.wgrad_reference(rounding(frame), dy)[0]):
            r.bad.append(f"dw equals the gradient on the frame rounded by {name}")
    r.done()
