"""The exact-operand cases of tests/exact_cases.py, the reference side alone (no device): so that no case of
tests/test_gpu_exact.py can pass vacuously.  For every case: the operands survive the format the kernel reads, the declared
bound holds, the fp32 reference equals the fp64 one bit for bit, the values in front of a bf16 rounding separate
round-to-nearest-even from truncation and from round-half-away (at least 5 % exact ties, 5 % that truncation rounds
otherwise, 5 % that half-away rounds otherwise), the ReLU masks are 30 - 70 % active, the pooling windows of the pool-backward
cases have tied maxima.  These are conditions on the inputs; each test prints its shares (``pytest -s``).

The shares of a forward case are taken on its linear form conv(x, w) (all outputs, both signs); those of a data-gradient
case on the plain sum, and the second rounding of the mask-and-add form is held to the same three conditions.

test_every_case_runs_the_class_it_is_listed_for is the guard: through the host-only plan queries it asserts that every case
launches the class it is listed for and that the cases cover every class of the tables."""
import os
import sys

import pytest
import torch

import exact_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

MIN_SHARE = 0.05


def _ids(cases):
    return [c.id for c in cases]


def _assert_separates(tag, pre):
    s = E.rounding_shares(pre)
    print(f"[{tag}] rounded {s['rounded']:.3f} ties {s['ties']:.3f} trunc-differs {s['trunc']:.3f} half-away-differs {s['away']:.3f}",
          end=" ")
    assert s["ties"] >= MIN_SHARE and s["trunc"] >= MIN_SHARE and s["away"] >= MIN_SHARE, (tag, s)
    # the comparison the GPU tests use tells the other roundings from the reference
    assert E.compare_bits(E.bf16_trunc(pre), E.bf(pre), pre) is not None
    assert E.compare_bits(E.bf16_half_away(pre), E.bf(pre), pre) is not None
    return s


def _assert_mask(tag, active):
    share = float(active.float().mean())
    print(f"mask {share:.3f}", end=" ")
    assert 0.30 <= share <= 0.70, (tag, share)


def _assert_bound(tag, bound):
    print(f"[{tag}] bound {bound} = {bound / E.LIMIT:.4f} x 2^24", end=" ")
    assert 0 < bound < E.LIMIT, (tag, bound)


@pytest.mark.parametrize("c", E.FWD_CASES, ids=_ids(E.FWD_CASES))
def test_forward_case(c):
    n, h, w, ci, co = c.shape
    _assert_bound(c.id, E.fwd_bound(c))
    x, wt, b = E.fwd_operands(c)
    assert E.survives_bf16(x) and E.survives_bf16(wt) and x.abs().max() <= c.xmax and wt.abs().max() <= c.wmax and b.abs().max() <= c.bmax
    assert b.abs().max() > 0 and torch.equal(b, b.round())
    r32, r64 = E.fwd_reference(x, wt, b), E.fwd_reference(x, wt, b, torch.float64)
    for k in r32:
        assert torch.equal(r32[k].double(), r64[k]), k
        assert r32[k].abs().max() <= E.fwd_bound(c)
    if co == 16:  # fp32 output: nothing is rounded
        print()
        return
    _assert_separates(c.id + " linear", r32["linear"])
    s = E.rounding_shares(r32["relu"])
    print(f"| relu form: ties {s['ties']:.3f} trunc-differs {s['trunc']:.3f} half-away-differs {s['away']:.3f}", end=" ")
    assert min(s.values()) > 0
    _assert_mask(c.id, r32["relu"] > 0)
    print()


@pytest.mark.parametrize("c", E.DGRAD_CASES, ids=_ids(E.DGRAD_CASES))
def test_dgrad_case(c):
    n, h, w, ci, co = c.shape
    _assert_bound(c.id, E.dgrad_bound(c))
    dy, wt, src, add = E.dgrad_operands(c)
    for t, amax in ((dy, c.ymax), (wt, c.wmax), (src, c.smax), (add, c.amax)):
        assert E.survives_bf16(t) and t.abs().max() <= amax
    assert src.min() == 0
    s32, s64 = E.dgrad_sum(dy, wt), E.dgrad_sum(dy, wt, torch.float64)
    assert torch.equal(s32.double(), s64) and s32.abs().max() + c.amax <= E.dgrad_bound(c)
    _assert_separates(c.id + " sum", s32)
    _assert_mask(c.id, src > 0)
    if c.kind == "plain":
        _, pre = E.dgrad_epilogue(s32, src > 0, add)
        _, pre64 = E.dgrad_epilogue(s64, src > 0, add.double())
        assert torch.equal(pre.double(), pre64)
        print("|", end=" ")
        _assert_separates(c.id + " mask+add", pre)
        _assert_separates(c.id + " add", E.dgrad_epilogue(s32, None, add)[1])
        # the bit form of the mask is the same mask
        nhwc = src.permute(0, 2, 3, 1).contiguous()
        bits = E.relu_bits(nhwc)
        back = ((bits.unsqueeze(-1).to(torch.int32) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(nhwc.shape).bool()
        assert torch.equal(back, nhwc > 0)
    else:
        routed = E.pool_backward(src, add)
        # every window's gradient lands on exactly one pixel of a live window, and on none of a dead one
        live = E.pool_windows(src).max(-1).values > 0
        assert torch.equal(E.pool_windows(routed).nan_to_num(neginf=0.0).sum(-1), add * live)
        assert not routed[src == 0].any() and E.compare_bits(routed, routed + 0.0) is None  # (and no -0: the kernels write +0)
        # ... and it is what autograd routes (torch's CPU pool takes the first maximum too)
        leaf = src.clone().requires_grad_(True)
        E.pool(leaf).backward(add)
        assert torch.equal(routed, leaf.grad * (src > 0))
        share = E.tied_window_share(src)
        print(f"tied windows {share:.3f}", end=" ")
        assert share >= MIN_SHARE
        _, pre = E.dgrad_epilogue(s32, src > 0, routed)
        s = E.rounding_shares(pre)
        print(f"| mask+routed: ties {s['ties']:.3f} trunc-differs {s['trunc']:.3f} half-away-differs {s['away']:.3f}", end=" ")
        assert min(s.values()) > 0
    print()


@pytest.mark.parametrize("c", E.WGRAD_CASES, ids=_ids(E.WGRAD_CASES))
def test_wgrad_case(c):
    _assert_bound(c.id, E.wgrad_bound(c))
    x, dy, pw, pb = E.wgrad_operands(c)
    assert E.survives_bf16(x) and E.survives_bf16(dy) and x.abs().max() <= c.xmax and dy.abs().max() <= c.ymax
    assert max(pw.abs().max(), pb.abs().max()) <= c.pmax
    (dw, db), (dw64, db64) = E.wgrad_reference(x, dy), E.wgrad_reference(x, dy, torch.float64)
    assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)
    assert torch.equal((dw + pw).double(), dw64 + pw.double()) and torch.equal((db + pb).double(), db64 + pb.double())
    assert dw.abs().max() + c.pmax <= E.wgrad_bound(c)
    # a halo pixel taken at weight 0, or one product counted twice, changes an integer: the corner taps differ from the centre
    assert not torch.equal(dw[:, :, 0, 0], dw[:, :, 1, 1])
    print(f"max|dw| {int(dw.abs().max())} max|db| {int(db.abs().max())}")


@pytest.mark.parametrize("c", E.FIRST_FWD_CASES, ids=_ids(E.FIRST_FWD_CASES))
def test_first_forward_case(c):
    _assert_bound(c.id, E.first_fwd_bound(c))
    frame, wt, b = E.first_fwd_operands(c)
    unit = c.xdiv * c.wdiv
    for t, kmax, div in ((frame, c.xkmax, c.xdiv), (wt, c.kmax, c.wdiv)):
        assert (t * div).abs().max() <= kmax and torch.equal(t * div, (t * div).round())
        lo = t - E.bf(t)
        assert E.survives_bf16(lo)  # the split into two bf16 terms is exact
        if c.kind == "split":  # ... and the low term is there
            assert float((lo != 0).float().mean()) > 0.2
    y32, y64 = E.first_fwd_reference(frame, wt, b), E.first_fwd_reference(frame, wt, b, torch.float64)
    assert torch.equal(y32.double(), y64)
    assert torch.equal(y32 * unit, (y32 * unit).round()) and (y32 * unit).abs().max() <= E.first_fwd_bound(c)
    pre = torch.nn.functional.conv2d(frame, wt, b, padding=1)
    if c.kind == "ties":
        _assert_separates(c.id + " conv+b", pre)
    else:
        s = E.rounding_shares(pre)
        print(f"[{c.id} conv+b] rounded {s['rounded']:.3f} ties {s['ties']:.4f} trunc-differs {s['trunc']:.3f} half-away-differs "
              f"{s['away']:.4f}", end=" ")
        assert s["rounded"] > 0.9 and s["trunc"] >= 0.3
    _assert_mask(c.id, y32 > 0)
    print()


@pytest.mark.parametrize("c", E.FIRST_WGRAD_CASES, ids=_ids(E.FIRST_WGRAD_CASES))
def test_first_wgrad_case(c):
    _assert_bound(c.id, E.first_wgrad_bound(c))
    frame, dy = E.first_wgrad_operands(c)
    assert E.survives_bf16(dy) and frame.abs().max() <= c.xmax and dy.abs().max() <= c.ymax
    (dw, db), (dw64, db64) = E.first_wgrad_reference(frame, dy), E.first_wgrad_reference(frame, dy, torch.float64)
    assert torch.equal(dw.double(), dw64) and torch.equal(db.double(), db64)
    assert dw.abs().max() <= E.first_wgrad_bound(c)
    if c.id == "first_wgrad_rounded_frame":
        share = E.significant_bits_over_8_share(frame)
        ties = float(E.is_tie(frame).float().mean())
        print(f"frame values of more than 8 significant bits {share:.3f}, ties {ties:.3f}", end=" ")
        assert share >= 0.30 and ties >= MIN_SHARE
        # the rounding mode of the in-kernel convert shows in the gradient
        assert not torch.equal(E.wgrad_reference(E.bf16_trunc(frame), dy)[0], dw)
        assert not torch.equal(E.wgrad_reference(E.bf16_half_away(frame), dy)[0], dw)
        assert not torch.equal(E.wgrad_reference(frame, dy)[0], dw)
        n, h, w = c.shape
        tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
        assert tiles % 4 != 0  # the last chunk of four tiles is partial
    else:
        assert E.survives_bf16(frame)
        n, h, w = c.shape
        assert n * ((h + 7) // 8) * ((w + 15) // 16) > 512
    print(f"max|dw| {int(dw.abs().max())}")


def test_every_case_runs_the_class_it_is_listed_for():
    """CPU guard (host-only plan queries): every case launches the class it is listed for, and together the cases cover
    every class of the tables; a change of the selection rule that moves a case fails here, not silently on the GPU."""
    from fosvos_hip import ops
    seen = set()
    for c in E.FWD_CASES:
        got = E.fwd_class(ops, c)
        assert got == c.cls, (c.id, got, c.cls)
        seen.add(got)
    assert seen == E.FWD_CLASSES, sorted(E.FWD_CLASSES ^ seen)
    print("forward classes covered:", sorted(seen))
    seen, seen_unpool = set(), set()
    for c in E.DGRAD_CASES:
        got = E.dgrad_class(ops, c)
        assert got == c.cls, (c.id, got, c.cls)
        (seen_unpool if c.kind == "unpool" else seen).add(got)
        if c.kind == "plain":
            bits = E.dgrad_bits_class(ops, c)
            assert bits == getattr(c, "bits_cls", c.cls), (c.id, bits)
            seen.add(bits)
    assert seen == E.DGRAD_CLASSES, sorted(E.DGRAD_CLASSES ^ seen)
    assert seen_unpool == E.UNPOOL_CLASSES, sorted(E.UNPOOL_CLASSES ^ seen_unpool)
    print("data-gradient classes covered:", sorted(seen), "with the pool backward:", sorted(seen_unpool))
    # the split-K epilogue and the fused one both carry the mask-and-add forms
    assert any(c.cls.endswith("/k16") for c in E.DGRAD_CASES) and any(c.cls.endswith("/k1") for c in E.DGRAD_CASES)
    for c in E.FIRST_FWD_CASES:
        tiles, wgs = ops.conv3x3_first_plan(*c.shape)
        assert tiles >= 1 and wgs >= 1
