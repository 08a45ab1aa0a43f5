"""Compact stage 1 on the device (run with ``pytest -m gpu``): conv1_2's pooled forward that stores the pool's winner codes
instead of its dense output (fosvos_conv3x3_fwd_pool_codes), the pool backward that routes from them
(fosvos_maxpool2x2_ceil_bwd_codes), and the native pass / the online loop with ``compact_stage1`` on against off.
Everything here is bit for bit: the reference of the forward op is the dense entry's own output (its pooled map, and
``stage1_codes_cases.codes`` of its ``y``), the reference of the backward op is fosvos_maxpool2x2_ceil_bwd (relu_mask = 1).
Outputs sit between poisoned margins that must come back untouched."""
import os
import sys

import pytest
import torch

import exact_cases as E
import stage1_codes_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
MARGIN = 4096
E_SHAPE = -1


@pytest.fixture(scope="module")
def ops():
    from fosvos_hip import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t


class Island:
    """A tensor between two margins of MARGIN poisoned bytes; the tensor itself starts poisoned too (0xA5 bytes: a NaN-free
    negative bf16, a code word with every nibble invalid)."""

    def __init__(self, shape, dtype):
        self.nbytes = int(torch.tensor(shape).prod()) * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * MARGIN + self.nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.buf[MARGIN:MARGIN + self.nbytes].view(dtype).view(*shape)

    def margins_untouched(self):
        return bool((self.buf[:MARGIN] == 0xA5).all()) and bool((self.buf[MARGIN + self.nbytes:] == 0xA5).all())


def conv_operands(n, h, w, ci, co, seed, wt=None, bias=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, h, w, ci), generator=g).clamp_min(0).to(BF).to(DEV)
    wt = (torch.randn((co, ci, 3, 3), generator=g) * 0.05) if wt is None else wt
    bias = (torch.randn((co,), generator=g) * 0.1) if bias is None else bias
    return x, wt.to(DEV), bias.to(DEV)


def run_forward(ops, x, wt, bias, ci, co):
    """(dense y, dense pooled, pooled island, codes island) of the two entries on the same operands."""
    n, h, w, _ = x.shape
    wf, _ = ops.pack_conv3x3_weights(wt, True, False)
    y, yp = ops.conv3x3_fwd_pool(x, wf, bias, ci, co)
    isl_p = Island((n, (h + 1) // 2, (w + 1) // 2, co), BF)
    isl_c = Island(ops.conv3x3_pool_codes_shape(n, h, w, co), torch.int32)
    ops.conv3x3_fwd_pool_codes(x, wf, bias, ci, co, out=(isl_p.t, isl_c.t))
    torch.cuda.synchronize()
    return y, yp, isl_p, isl_c, wf


def check_forward(ops, x, wt, bias, ci, co):
    n, h, w, _ = x.shape
    assert ops.conv3x3_fwd_plan(n, h, w, ci, co)["persistent"]
    y, yp, isl_p, isl_c, wf = run_forward(ops, x, wt, bias, ci, co)
    assert torch.equal(bits(isl_p.t), bits(yp)), "pooled map"
    want = SC.pack_words(SC.codes(y))
    if not torch.equal(isl_c.t, want):
        bad = (isl_c.t != want).nonzero()
        raise AssertionError("codes: %d words differ, first at %s: got %#x want %#x" % (
            bad.shape[0], bad[0].tolist(), int(isl_c.t[tuple(bad[0])]) & 0xFFFFFFFF, int(want[tuple(bad[0])]) & 0xFFFFFFFF))
    assert isl_p.margins_untouched() and isl_c.margins_untouched(), "margins"
    # a second launch into the same buffers: the same bits
    first_p, first_c = isl_p.t.clone(), isl_c.t.clone()
    ops.conv3x3_fwd_pool_codes(x, wf, bias, ci, co, out=(isl_p.t, isl_c.t))
    torch.cuda.synchronize()
    assert torch.equal(bits(isl_p.t), bits(first_p)) and torch.equal(isl_c.t, first_c), "second launch"
    assert isl_p.margins_untouched() and isl_c.margins_untouched(), "margins (second launch)"
    return y, SC.unpack_words(isl_c.t)


@pytest.mark.parametrize("shape", SC.FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_codes(ops, shape):
    n, h, w = shape
    x, wt, bias = conv_operands(n, h, w, 64, 64, seed=11 + h)
    y, nib = check_forward(ops, x, wt, bias, 64, 64)
    print("forward %s: %.1f %% of the windows route a gradient" % (shape, 100.0 * float((nib != 0).float().mean())))
    assert (nib != 0).any() and (nib == 0).any()
    # all four pixels win somewhere (in-image windows), and the ragged last row / column never names a pixel outside
    for k in range(4):
        assert (nib == 1 << k).any(), k
    if h % 2:
        assert not (nib[:, -1] & 0b1100).any()
    if w % 2:
        assert not (nib[:, :, -1] & 0b1010).any()


def test_forward_constant_positive_output(ops):
    """Zero weights, positive bias: every window is a four-way (or ragged two-way) tie - pixel 0 everywhere."""
    n, h, w = 6, 121, 213
    x, wt, bias = conv_operands(n, h, w, 64, 64, seed=3, wt=torch.zeros((64, 64, 3, 3)), bias=torch.full((64,), 0.75))
    y, nib = check_forward(ops, x, wt, bias, 64, 64)
    assert bool((y.float() == 0.75).all())
    assert bool((nib == 1).all())


def test_forward_negative_bias(ops):
    """Zero weights, negative bias: the ReLU output is 0 everywhere, every nibble is 0."""
    n, h, w = 6, 121, 213
    x, wt, bias = conv_operands(n, h, w, 64, 64, seed=4, wt=torch.zeros((64, 64, 3, 3)), bias=torch.full((64,), -0.5))
    y, nib = check_forward(ops, x, wt, bias, 64, 64)
    assert bool((y.float() == 0).all())
    assert bool((nib == 0).all())


def test_forward_exact_integers_with_ties(ops):
    """Exactly summable integer operands (tests/exact_cases.py style: small integers, sums far below 2^24 and - with these
    ranges - below 2^8, so every output is an integer bf16 holds exactly): real conv output in which many windows tie."""
    n, h, w, ci, co = 2, 128, 512, 64, 64
    g = torch.Generator().manual_seed(1234)
    xi = torch.randint(0, 2, (n, h, w, ci), generator=g).float()  # 0 / 1
    xi = xi * (torch.rand((n, h, w, 1), generator=g) < 0.5)       # half of the pixels all zero
    wt = E.ints(g, (co, ci, 3, 3), 1) * (torch.rand((co, ci, 3, 3), generator=g) < 0.02)  # sparse -1 / 0 / 1
    bias = E.ints(g, (co,), 2)
    assert 9 * ci * 1 * 1 + 2 < 2 ** 24
    x = xi.to(BF).to(DEV)
    y, nib = check_forward(ops, x, wt.to(DEV), bias.to(DEV), ci, co)
    yf = y.float()
    assert bool((yf == yf.round()).all()) and float(yf.max()) < 256  # integers, exact in bf16
    v = torch.nn.functional.pad(yf.permute(0, 3, 1, 2), (0, w % 2, 0, h % 2), value=-1.0)
    win = torch.stack([v[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])
    mx = win.max(0).values
    tied = ((win == mx).sum(0) > 1) & (mx > 0)
    print("exact integers: %.1f %% of the windows tie at a positive maximum" % (100.0 * float(tied.float().mean())))
    assert float(tied.float().mean()) > 0.1  # (measured on the host for these operands: 0.18)


def test_forward_two_channel_blocks(ops):
    """64 -> 128 channels at (2, 240, 427): two 64-channel blocks per pixel tile."""
    n, h, w = 2, 240, 427
    x, wt, bias = conv_operands(n, h, w, 64, 128, seed=8)
    check_forward(ops, x, wt, bias, 64, 128)


def test_forward_refuses_what_the_persistent_kernel_refuses(ops):
    from fosvos_hip import FosvosHipError, lib
    n, h, w = 1, 120, 214
    assert not ops.conv3x3_fwd_plan(n, h, w, 64, 64)["persistent"]
    x, wt, bias = conv_operands(n, h, w, 64, 64, seed=9)
    wf, _ = ops.pack_conv3x3_weights(wt, True, False)
    isl_p = Island((n, 60, 107, 64), BF)
    isl_c = Island((n, 60, 107, 8), torch.int32)
    rc = lib().fosvos_conv3x3_fwd_pool_codes(x.data_ptr(), wf.data_ptr(), bias.data_ptr(), isl_p.t.data_ptr(), isl_c.t.data_ptr(),
                                             n, h, w, 64, 64, 1, 0, torch.cuda.current_stream(0).cuda_stream)
    assert rc == E_SHAPE
    with pytest.raises(FosvosHipError):
        ops.conv3x3_fwd_pool_codes(x, wf, bias, 64, 64, out=(isl_p.t, isl_c.t))
    torch.cuda.synchronize()
    assert bool((isl_p.buf == 0xA5).all()) and bool((isl_c.buf == 0xA5).all())  # nothing was launched


@pytest.mark.parametrize("shape", SC.BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_from_codes(ops, shape):
    """dx from the codes == fosvos_maxpool2x2_ceil_bwd(y, dy, relu_mask = 1), signs of zeros included."""
    n, h, w, c = shape
    y = SC.few_valued((n, h, w, c), seed=h + w, levels=4, zero_share=0.4).to(DEV)
    g = torch.Generator().manual_seed(17 + h)
    dy = torch.randn((n, (h + 1) // 2, (w + 1) // 2, c), generator=g)
    dy.view(-1)[::7] = -0.0  # negative zeros travel as they are
    dy.view(-1)[3::11] = 0.0
    dy = dy.to(BF).to(DEV)
    want = ops.maxpool_bwd(y, dy, True)
    words = SC.pack_words(SC.codes(y))
    isl = Island((n, h, w, c), BF)
    ops.maxpool_bwd_codes(words, dy, h, w, out=isl.t)
    torch.cuda.synchronize()
    assert torch.equal(bits(isl.t), bits(want))  # (every in-image element was written: none kept the 0xA5 poison)
    assert isl.margins_untouched()
    assert torch.equal(bits(isl.t), bits(SC.route(SC.codes(y), dy, h, w)))
    if h * w > 1:
        assert bool((bits(isl.t) == -32768).any())  # a -0 gradient arrived as -0


# ------------------------------------------------------------------------------------------ the pass
def make_net(seed):
    from networks.osvos_vgg import OSVOS_VGG
    from oracle import osvos_ref as O
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(O.make_state_dict(seed))
    return net.to(DEV)


def frames(n, h, w, seed):
    from oracle import osvos_ref as O
    xs, gts = zip(*[O.synthetic_frame(1, h, w, seed=seed + i) for i in range(n)])
    return torch.cat(xs), torch.cat(gts)


def run_pass(net, x, gt, compact):
    """One forward + loss + backward through the drop-in module on a fresh 0xFF arena.  Returns the fused logits, the
    parameter gradients and the arena's regions."""
    from fosvos_hip import engine, lib, ops as _ops
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    n, _, h, w = x.shape
    pool = net._packs.arenas
    held = []

    def take(n_, h_, w_, device):
        held.append(torch.full((lib().fosvos_vgg_arena_bytes(n_, h_, w_) + 256,), 255, dtype=torch.uint8, device=DEV))
        return held[-1]

    pool.take = take
    try:
        net.zero_grad(set_to_none=True)
        net.compact_stage1 = compact
        net.compute_side_outputs = False
        outs = net(x.to(DEV))
        cbce(outs[-1], gt.to(DEV), size_average=False).backward()
        net.join_gradients()
        torch.cuda.synchronize()
    finally:
        del pool.take
        net.compact_stage1 = False
    assert len(held) == 1
    arena = held[0]
    lay = _ops.vgg_arena_layout(n, h, w)
    base = engine._aligned_ptr(arena)[0] - arena.data_ptr()
    regions = {}
    for c in range(13):
        regions["act%d" % c] = arena[base + lay["act"][c]: base + lay["act"][c] + lay["act_bytes"][c]]
        regions["gact%d" % c] = arena[base + lay["gact"][c]: base + lay["gact"][c] + lay["act_bytes"][c]]
    for i in range(4):
        for name, size in (("pooled", "pooled_bytes"), ("gpooled", "pooled_bytes"), ("side", "side_bytes"), ("dside", "dside_bytes")):
            regions["%s%d" % (name, i)] = arena[base + lay[name][i]: base + lay[name][i] + lay[size][i]]
    regions["bits0"] = arena[base + lay["bits0"]: base + lay["bits0"] + lay["bits0_bytes"]]
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
    return outs[-1].detach().clone(), grads, regions


@pytest.fixture(scope="module")
def pass_net():
    return make_net(31)


def test_pass_compact_equals_dense(ops, pass_net):
    n, h, w = SC.PASS_SHAPE
    assert ops.vgg_stage1_compact(n, h, w) and not ops.vgg_stage1_compact(n, h, w, False)
    x, gt = frames(n, h, w, seed=40)
    fused0, grads0, reg0 = run_pass(pass_net, x, gt, False)
    fused1, grads1, reg1 = run_pass(pass_net, x, gt, True)
    assert torch.equal(fused0, fused1)
    assert grads0.keys() == grads1.keys() and len(grads0) > 30
    for k in grads0:
        assert torch.equal(grads0[k], grads1[k]), k
    for k in reg0:
        if k != "act1":
            assert torch.equal(reg0[k], reg1[k]), k
    assert bool(torch.isfinite(reg0["gact1"].view(BF).float()).all())
    # the compact pass left the codes at the start of act[1] - those of the dense pass's conv1_2 output - and nothing behind
    y = reg0["act1"].view(BF).view(n, h, w, 64)
    words = SC.pack_words(SC.codes(y)).reshape(-1)
    got = reg1["act1"][: words.numel() * 4].view(torch.int32)
    assert torch.equal(got, words)
    assert bool((reg1["act1"][words.numel() * 4:] == 255).all())


def test_pass_single_small_frame_stays_dense(ops, pass_net):
    n, h, w = 1, SC.PASS_SHAPE[1], SC.PASS_SHAPE[2]
    assert not ops.vgg_stage1_compact(n, h, w)
    x, gt = frames(n, h, w, seed=50)
    fused0, grads0, reg0 = run_pass(pass_net, x, gt, False)
    fused1, grads1, reg1 = run_pass(pass_net, x, gt, True)
    assert bool(torch.isfinite(reg1["act1"].view(BF).float()).all())  # written in full (the arena started as NaN bytes)
    assert torch.equal(fused0, fused1)
    for k in grads0:
        assert torch.equal(grads0[k], grads1[k]), k
    for k in reg0:
        assert torch.equal(reg0[k], reg1[k]), k


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass


def _train_online(compact, loader, epochs):
    import train_online
    from util.network_provider import VGGOnlineProvider
    net = make_net(23)
    prov = VGGOnlineProvider.__new__(VGGOnlineProvider)
    prov.network = net
    prov.name = "vgg16"
    opt = prov.get_optimizer(learning_rate=1e-8)
    train_online.data_parallel = False
    ret = train_online._train(prov, loader, opt, _NullWriter(), "stage1", 0, epochs, 5, 10 ** 9, compact_stage1=compact)
    torch.cuda.synchronize()
    weights = {k: p.detach().clone() for k, p in net.named_parameters()}
    momentum = {k: opt.state[p]["momentum_buffer"].detach().clone() for k, p in net.named_parameters() if p in opt.state
                and "momentum_buffer" in opt.state[p]}
    return net, ret, weights, momentum


def test_online_loop_compact_equals_dense():
    """10 steps of the online loop on 125x499 frames, cycles of five (one batched pass of five frames each): compact on
    against forced off - weights and momentum bit for bit - and the module's flag is off again afterwards."""
    from oracle import osvos_ref as O
    h, w = SC.PASS_SHAPE[1], SC.PASS_SHAPE[2]
    loader = [{"image": x, "gt": gt} for x, gt in (O.synthetic_frame(1, h, w, seed=70 + i) for i in range(5))]
    net1, ret1, w1, m1 = _train_online(True, loader, 2)
    assert ret1["iterations"] == 10
    assert net1.compact_stage1 is False and net1.pass_flags.compact_stage1 is False
    net0, ret0, w0, m0 = _train_online(False, loader, 2)
    assert net0.compact_stage1 is False
    assert ret0["loss"] == ret1["loss"]
    assert w0.keys() == w1.keys() and m0.keys() == m1.keys() and len(m0) > 30
    for k in w0:
        assert torch.equal(w0[k], w1[k]), k
    for k in m0:
        assert torch.equal(m0[k], m1[k]), k


def test_online_loop_restores_the_flag_when_a_pass_raises():
    import train_online
    from oracle import osvos_ref as O
    from util.network_provider import VGGOnlineProvider
    net = make_net(23)
    prov = VGGOnlineProvider.__new__(VGGOnlineProvider)
    prov.network = net
    prov.name = "vgg16"
    opt = prov.get_optimizer(learning_rate=1e-8)
    train_online.data_parallel = False
    seen = []

    class Boom(RuntimeError):
        pass

    def forward(x):
        seen.append(net.pass_flags.compact_stage1)
        raise Boom()

    net.forward = forward
    x, gt = O.synthetic_frame(1, 40, 70, seed=1)
    with pytest.raises(Boom):
        train_online._train(prov, [{"image": x, "gt": gt}], opt, _NullWriter(), "boom", 0, 1, 1, 10 ** 9)
    assert seen == [True]  # the loop had set it for its passes
    assert net.pass_flags.compact_stage1 is False
