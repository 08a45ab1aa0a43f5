"""The winner codes of the compact stage 1, without a device: the host reference ``stage1_codes_cases.codes`` against torch's
own max pool (first-maximum tie-breaking is the property under test), the word layout, and the argument errors and size
queries of the new entry points (which answer before any device call)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import stage1_codes_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

E_SHAPE, E_ARG = -1, -2


@pytest.fixture(scope="module")
def L():
    from fosvos_hip import lib
    return lib()


def torch_codes(y):
    """The same nibbles from max_pool2d's own indices (ceil mode, first maximum in scan order) and max > 0."""
    n, h, w, c = y.shape
    v = y.float().permute(0, 3, 1, 2).contiguous()
    m, idx = F.max_pool2d(v, 2, 2, ceil_mode=True, return_indices=True)
    iy, ix = idx // w, idx % w  # flat index into the [h, w] plane
    k = (iy % 2) * 2 + (ix % 2)
    nib = torch.where(m > 0, torch.ones_like(k) << k, torch.zeros_like(k))
    return nib.permute(0, 2, 3, 1).contiguous().to(torch.uint8)


@pytest.mark.parametrize("shape,levels,zero_share", [((2, 7, 9, 8), 3, 0.5), ((1, 1, 1, 8), 2, 0.5), ((3, 6, 5, 16), 2, 0.3),
                                                     ((1, 5, 1, 8), 4, 0.2), ((1, 1, 6, 8), 4, 0.2), ((2, 13, 11, 24), 4, 0.6)])
def test_reference_codes_match_torch_pool_indices(shape, levels, zero_share):
    y = SC.few_valued(shape, seed=sum(shape), levels=levels, zero_share=zero_share)
    got, want = SC.codes(y), torch_codes(y)
    assert torch.equal(got, want)
    # the case has what it is for: windows whose maximum is shared by several pixels, and windows that are all zero
    n, h, w, c = shape
    if h > 1 and w > 1:
        v = F.pad(y.float().permute(0, 3, 1, 2), (0, w % 2, 0, h % 2), value=-1.0)
        win = F.unfold(v.reshape(n * c, 1, *v.shape[2:]), 2, stride=2)  # [n c, 4, windows]
        ties = ((win == win.max(1, keepdim=True).values).sum(1) > 1) & (win.max(1).values > 0)
        assert ties.float().mean() > 0.05  # (of ALL windows, the all-zero ones included)
        assert (got == 0).any() and (got != 0).any()
    # one-hot or zero, never a pixel outside the image
    assert set(got.unique().tolist()) <= {0, 1, 2, 4, 8}
    if h % 2:
        assert not (got[:, -1] & 0b1100).any()
    if w % 2:
        assert not (got[:, :, -1] & 0b1010).any()


def test_later_pixel_needs_a_strictly_larger_value():
    y = torch.zeros((1, 2, 2, 8))
    y[0, :, :, 0] = torch.tensor([[1.0, 1.0], [1.0, 1.0]])   # four-way tie: pixel 0
    y[0, :, :, 1] = torch.tensor([[0.5, 1.0], [1.0, 1.0]])   # first of three: pixel 1
    y[0, :, :, 2] = torch.tensor([[0.5, 0.5], [1.0, 1.0]])   # pixel 2
    y[0, :, :, 3] = torch.tensor([[0.5, 0.5], [0.5, 1.0]])   # pixel 3
    y[0, :, :, 4] = 0.0                                       # ReLU output 0 everywhere: the gradient goes nowhere
    y[0, :, :, 5] = torch.tensor([[0.0, 0.0], [0.0, 2.0 ** -126]])  # the smallest normal value is > 0
    y[0, :, :, 6] = torch.tensor([[3.0, 2.0], [3.0, 1.0]])   # tie between pixels 0 and 2: pixel 0
    y[0, :, :, 7] = torch.tensor([[2.0, 3.0], [3.0, 3.0]])
    assert SC.codes(y)[0, 0, 0].tolist() == [1, 2, 4, 8, 0, 8, 1, 2]


def test_word_layout_round_trip():
    g = torch.Generator().manual_seed(3)
    nib = (1 << torch.randint(0, 4, (2, 3, 5, 16), generator=g)).to(torch.uint8)
    nib[0, 0, 0, :4] = 0
    words = SC.pack_words(nib)
    assert words.dtype == torch.int32 and tuple(words.shape) == (2, 3, 5, 2)
    assert torch.equal(SC.unpack_words(words), nib)
    # channel 8 g + 2 i + h at bit 4 i + 16 h
    one = torch.zeros((1, 1, 1, 8), dtype=torch.uint8)
    for ch, bit in ((0, 0), (1, 16), (2, 4), (3, 20), (4, 8), (5, 24), (6, 12), (7, 28)):
        one.zero_()
        one[..., ch] = 8
        assert (int(SC.pack_words(one)) & 0xFFFFFFFF) == 8 << bit, ch


def test_route_is_the_pool_backward_of_the_reference():
    """codes + route against autograd's max-pool backward with the ReLU mask (on values whose pool backward is unambiguous
    up to the tie rule both share)."""
    y = SC.few_valued((2, 7, 9, 8), seed=5)
    dy = torch.randn((2, 4, 5, 8))
    v = y.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(torch.relu(v), 2, 2, ceil_mode=True).backward(dy.permute(0, 3, 1, 2))
    # (relu's backward zeroes where y <= 0: a window of zeros routes to its first pixel in autograd's pool and dies in the ReLU)
    assert torch.equal(SC.route(SC.codes(y), dy, 7, 9), v.grad.permute(0, 2, 3, 1))


def test_codes_bytes_query(L):
    q = L.fosvos_conv3x3_pool_codes_bytes
    assert q(1, 1, 1, 8) == 4
    assert q(5, 480, 854, 64) == 5 * 240 * 427 * 8 * 4
    assert q(6, 121, 213, 64) == 6 * 61 * 107 * 8 * 4
    assert q(2, 240, 427, 128) == 2 * 120 * 214 * 16 * 4
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (1, 8, 8, 12), (-1, 8, 8, 8)):
        assert q(*bad) == 0, bad
    # far below the dense output it stands in for
    assert q(5, 480, 854, 64) * 15 < 5 * 480 * 854 * 64 * 2


def test_forward_entry_argument_errors(L):
    """Every refusal below is decided on the host, in front of any device call (no GPU here)."""
    f = L.fosvos_conv3x3_fwd_pool_codes
    p = 4096  # never dereferenced
    assert f(None, p, None, p, p, 2, 128, 512, 64, 64, 1, 0, None) == E_ARG      # x
    assert f(p, None, None, p, p, 2, 128, 512, 64, 64, 1, 0, None) == E_ARG      # weights
    assert f(p, p, None, None, p, 2, 128, 512, 64, 64, 1, 0, None) == E_ARG      # pooled output
    assert f(p, p, None, p, None, 2, 128, 512, 64, 64, 1, 0, None) == E_ARG      # codes
    assert f(p, p, None, p, p + 2, 2, 128, 512, 64, 64, 1, 0, None) == E_ARG     # codes not word-aligned
    assert f(p, p, None, p, p, 2, 128, 512, 64, 64, 0, 0, None) == E_ARG         # the codes are taken behind the ReLU
    assert f(p, p, None, p, p, 2, 128, 512, 64, 64, 3, 0, None) == E_ARG         # fp32 output has no pooled form
    assert f(p, p, None, p, p, 0, 128, 512, 64, 64, 1, 0, None) == E_SHAPE
    assert f(p, p, None, p, p, 2, 128, 512, 64, 32, 1, 0, None) == E_SHAPE       # Co % 64
    # shapes the persistent kernel does not take: fewer than 512 tiles of 8 x 32
    assert f(p, p, None, p, p, 1, 120, 214, 64, 64, 1, 0, None) == E_SHAPE
    assert f(p, p, None, p, p, 1, 128, 480, 64, 64, 1, 0, None) == E_SHAPE
    assert b"persistent" in L.fosvos_last_error()


def test_backward_entry_argument_errors(L):
    f = L.fosvos_maxpool2x2_ceil_bwd_codes
    p = 4096
    assert f(None, p, p, 1, 8, 8, 8, 0, None) == E_ARG
    assert f(p, None, p, 1, 8, 8, 8, 0, None) == E_ARG
    assert f(p, p, None, 1, 8, 8, 8, 0, None) == E_ARG
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (1, 8, 8, 12), (70000, 8, 8, 8), (1, 140000, 8, 8),
                (1, 8192, 8192, 64)):
        assert f(p, p, p, *bad, 0, None) == E_SHAPE, bad


def test_predicate_follows_the_forward_chains(L):
    """Compact only with the flag, and only where conv1_2 of EVERY forward chain (ceil(N/2) and floor(N/2) frames, or N
    itself for a single frame) is a launch of the persistent kernel - which is what the forward plan reports."""
    from fosvos_hip import VGG_COMPACT_STAGE1, ops
    q = L.fosvos_vgg_stage1_compact

    def chains(n):
        return [n] if n < 2 else [(n + 1) // 2, n - (n + 1) // 2]

    seen = set()
    for n, h, w in ((5, 480, 854), (1, 480, 854), (1, 240, 427), (5, 125, 499), (1, 125, 499), (3, 125, 499), (2, 128, 512),
                    (4, 128, 512), (3, 128, 512), (1, 96, 160), (5, 40, 70), (2, 1, 1)):
        want = all(ops.conv3x3_fwd_plan(k, h, w, 64, 64)["persistent"] for k in chains(n))
        assert q(VGG_COMPACT_STAGE1, n, h, w) == int(want), (n, h, w)
        assert ops.vgg_stage1_compact(n, h, w) is want
        assert q(0, n, h, w) == 0 and ops.vgg_stage1_compact(n, h, w, False) is False
        seen.add(want)
    assert seen == {True, False}
    assert q(VGG_COMPACT_STAGE1, 5, 125, 499) == 1 and q(VGG_COMPACT_STAGE1, 1, 125, 499) == 0  # the pass tests' shapes
    assert q(VGG_COMPACT_STAGE1, 3, 128, 512) == 0  # (chains of 2 and 1 frames: the second has 256 tiles)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert q(VGG_COMPACT_STAGE1, *bad) == 0


def test_flag_is_declared_and_off_by_default():
    from fosvos_hip.engine import PackedWeights, PassFlags
    from networks.osvos_vgg import OSVOS_VGG
    flags = PassFlags()
    assert flags.compact_stage1 is False
    flags.compact_stage1 = True
    assert flags.compact_stage1 is True
    assert PackedWeights().flags.compact_stage1 is False
    net = OSVOS_VGG(pretrained=0)
    assert net.compact_stage1 is False
    net.compact_stage1 = True
    assert net.pass_flags.compact_stage1 is True
    net.compact_stage1 = False
    assert net.pass_flags.compact_stage1 is False
    with pytest.raises(AttributeError):
        flags.compact_stage_1 = True
