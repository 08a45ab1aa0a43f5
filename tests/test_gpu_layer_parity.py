"""Per-layer parity of the shipped native VGG pass (csrc/vgg_net.hip: fosvos_vgg_forward[_streams] / fosvos_vgg_backward) at
the shapes of the training step, by teacher forcing: every tensor the pass leaves in its arena is read back
(fosvos_vgg_arena_layout), and each layer is recomputed on the CPU in torch fp32 from the pass's OWN inputs - the bf16
values the previous layer wrote.  That removes the propagation of bf16 noise through 13 layers, so the op tests' one-rounding
tolerances (tests/test_gpu_ops.py) apply to every layer of the pass as it ships: its two frame chains, two streams, events,
arena regions and split-K workspaces.

Every pass runs on a freshly allocated arena filled with 0xFF bytes (NaN in bf16 and in fp32), so a region the pass should
have written and did not shows up as non-finite.  Each case asserts the launch classes it is about (persistent forward, igemm
tile and K split) through the plan queries, and test_plan_classes_of_the_step_are_covered (CPU) asserts that every class the
step's supported shapes launch appears in one of the cases.

Tolerance forms, all from tests/test_gpu_ops.py:
  * bf16 output of one fp32-accumulated value: |err| <= 2^-8 |ref| + 1e-5 max|ref|                       (assert_bf16_close)
  * bf16 sum of a rounded data-gradient term and an addend: 2^-7 |ref| + 1e-5 max|ref| + 2^-7 |term|  (test_conv3x3_dgrad)
  * fp32 side_prep output: rel-to-max 2e-5; head outputs 1e-5, head parameter gradients 2e-5        (test_head_fwd_bwd)
  * weight / bias gradients: rel-to-max 5e-5 against fp32 per image summed in fp64                   (_wgrad_ref)
  * pool selection and routing, bit masks: exact
Each case prints one line per layer: the worst error in units of its tolerance (1.0 = on the bar).
"""
import ctypes
import os
import sys
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import osvos_ref as O
from test_gpu_ops import _head_ref, bf, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

DEV = "cuda:0"
HEAD_SCALE = 0.02  # on the seeded fuse weights, as bench.py does: finite loss gradient, ReLU masks about half active

STAGE_OF = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
FIRST = (0, 2, 4, 7, 10)
LAST = (1, 3, 6, 9, 12)
STAGE_CH = (64, 128, 256, 512, 512)


# ------------------------------------------------------------------------------------------ launch classes (host only)
def _stage_sizes(h, w):
    sh, sw = [h], [w]
    for _ in range(4):
        sh.append((sh[-1] + 1) // 2)
        sw.append((sw[-1] + 1) // 2)
    return sh, sw


def _cls(plan, contraction):
    if plan["persistent"]:
        return "pp<=64" if contraction <= 64 else "pp-reload"
    return "%dx%dx%d/k%d" % (*plan["tile"], plan["k_splits"])


def launch_classes(n, h, w):
    """(op, class) of every 3x3 conv launch of the native pass over n frames of h x w (csrc/vgg_net.hip): the forward convs of
    each frame chain (ceil(n/2) and floor(n/2) frames) and their side_prep convs; the data gradients of the pass (conv1_2's on
    the bit mask, side_prep's with the fused pool backward for stages 2-4).  class = the persistent kernel (by regime) or the
    igemm tile and K split."""
    from fosvos_hip import ops
    sh, sw = _stage_sizes(h, w)
    out = set()
    for nf in ([n] if n == 1 else [(n + 1) // 2, n // 2]):
        for c in range(1, 13):
            s = STAGE_OF[c]
            out.add(("fwd", _cls(ops.conv3x3_fwd_plan(nf, sh[s], sw[s], CIN[c], COUT[c]), CIN[c])))
        for s in range(1, 5):
            out.add(("side", _cls(ops.conv3x3_plan(nf, sh[s], sw[s], STAGE_CH[s], 16), STAGE_CH[s])))
    for c in range(1, 13):
        s = STAGE_OF[c]
        if c == 1:  # fosvos_conv3x3_dgrad_bits takes the persistent kernel where the forward conv of its shape would
            pp = ops.conv3x3_fwd_plan(n, h, w, 64, 64)
            out.add(("dgrad_bits", _cls(pp if pp["persistent"] else ops.conv3x3_plan(n, h, w, 64, 64), 64)))
        else:
            out.add(("dgrad", _cls(ops.conv3x3_plan(n, sh[s], sw[s], COUT[c], CIN[c]), COUT[c])))
    for s in range(1, 5):
        out.add(("dgrad_unpool" if s < 4 else "dgrad", _cls(ops.conv3x3_plan(n, sh[s], sw[s], 16, STAGE_CH[s]), 16)))
    return out


# The GPU cases: (id, frames, height, width, objective) and the launch classes each one is there for (asserted in the case)
CASES = {
    "step_5x480x854": ((5, 480, 854), "online", {
        ("fwd", "pp<=64"), ("fwd", "pp-reload"), ("fwd", "8x32x64/k1"), ("fwd", "16x16x64/k1"), ("fwd", "8x16x64/k1"),
        ("side", "8x32x16/k1"), ("side", "4x16x16/k2"), ("dgrad_bits", "pp<=64"), ("dgrad", "8x32x64/k1"),
        ("dgrad", "16x16x64/k1"), ("dgrad_unpool", "8x32x64/k1"), ("dgrad_unpool", "16x16x64/k1")}),
    "offline_3x384x683": ((3, 384, 683), "offline", {
        ("fwd", "8x16x64/k2"), ("fwd", "8x16x64/k4"), ("side", "4x16x16/k8"), ("dgrad", "8x16x64/k2")}),
    "single_1x480x854": ((1, 480, 854), "online", {
        ("fwd", "8x16x64/k2"), ("side", "4x16x16/k3"), ("side", "4x16x16/k8"), ("dgrad_unpool", "8x16x64/k1")}),
    "half_2x240x427": ((2, 240, 427), "online", {("fwd", "8x16x64/k8"), ("side", "4x16x16/k16"), ("dgrad", "8x16x64/k4")}),
    "half_1x240x427": ((1, 240, 427), "online", {("dgrad_bits", "16x16x64/k1")}),
    "igemm_4x97x130": ((4, 97, 130), "online", {("dgrad_bits", "8x16x64/k1"), ("dgrad", "8x16x64/k3"), ("dgrad", "8x16x64/k8"),
                                                ("fwd", "8x16x64/k3")}),
    "odd_5x121x213": ((5, 121, 213), "online", {("dgrad", "8x16x64/k6"), ("fwd", "8x16x64/k16")}),
}

# the step's supported shapes (the online loop batches up to five frames, the offline loop 16; the mixed-size loop runs
# scales 0.8 and 0.5 of the 480x854 frame)
STEP_SHAPES = [(n, 480, 854) for n in (1, 2, 3, 5, 16)] + [(n, h, w) for n in range(1, 6) for h, w in ((384, 683), (240, 427))]


def test_plan_classes_of_the_step_are_covered():
    """CPU guard: every launch class the native pass takes at the step's shapes is exercised by a GPU case below, so that a
    plan change which moves a launch of the step onto a class no case runs fails here, not silently on the GPU."""
    covered = set()
    for (shape, _, about) in CASES.values():
        got = launch_classes(*shape)
        assert about <= got, (shape, sorted(about - got))
        covered |= got
    step = set()
    for shape in STEP_SHAPES:
        step |= launch_classes(*shape)
    assert not step - covered, f"launch classes of the step no GPU case runs: {sorted(step - covered)}"


# ------------------------------------------------------------------------------------------ tolerance forms
class Margins:
    """Worst error per (layer, check) in units of its tolerance; failures are collected and asserted at the end so that a
    case prints every layer's margin."""

    def __init__(self, tag):
        self.tag, self.rows, self.bad = tag, [], []

    def add(self, layer, what, m):
        m = float(m)
        self.rows.append((layer, what, m))
        if not m <= 1.0:  # (NaN fails)
            self.bad.append(f"{layer} {what}: {m:.3g}x the tolerance")

    def bf16(self, layer, a, ref):  # assert_bf16_close
        tol = (2.0 ** -8) * ref.abs() + 1e-5 * ref.abs().max()
        self.add(layer, "bf16", ((a - ref).abs() / tol.clamp_min(1e-30)).max())

    def bf16_two(self, layer, a, ref, term):  # the mask + add bound of test_conv3x3_dgrad
        tol = (2.0 ** -7) * ref.abs() + 1e-5 * ref.abs().max() + (2.0 ** -7) * term.abs()
        self.add(layer, "bf16x2", ((a - ref).abs() / tol.clamp_min(1e-30)).max())

    def rel(self, layer, what, a, ref, bound):
        self.add(layer, what, rel_err(a.double(), ref.double()) / bound)

    def exact(self, layer, what, a, b):
        n = int((a != b).sum()) if a.shape == b.shape else -1
        self.add(layer, what + " exact", 0.0 if n == 0 else float("inf"))

    def report(self):
        for layer, what, m in self.rows:
            print(f"[{self.tag}] {layer:<12s} {what:<14s} {m:.3f}")
        worst = max(self.rows, key=lambda r: r[2] if r[2] == r[2] else float("inf"))
        print(f"[{self.tag}] worst: {worst[0]} {worst[1]} {worst[2]:.3f} of the tolerance ({len(self.rows)} checks)")
        assert not self.bad, f"{self.tag}: " + "; ".join(self.bad)


def _wgrad(x, dy, ci, co):
    """Weight and bias gradient in torch fp32 on the CPU, image by image, the images added in float64 (_wgrad_ref of
    tests/test_gpu_ops.py, without the forward conv autograd would also run)."""
    dw = torch.zeros(co, ci, 3, 3, dtype=torch.float64)
    db = torch.zeros(co, dtype=torch.float64)
    wt = torch.zeros(co, ci, 3, 3)
    for i in range(x.shape[0]):
        _, gw, gb = torch.ops.aten.convolution_backward(dy[i:i + 1], x[i:i + 1], wt, [co], [1, 1], [1, 1], [1, 1], False,
                                                        [0, 0], 1, [False, True, True])
        dw += gw.double()
        db += gb.double()
    return dw, db


def _dgrad(dy, wt):  # input gradient of conv2d(x, wt, padding=1)
    return F.conv_transpose2d(dy, bf(wt), padding=1)


# ------------------------------------------------------------------------------------------ running the pass
def make_net(seed, uniform_head=True):
    from networks.osvos_vgg import OSVOS_VGG
    sd = O.make_state_dict(seed)
    sd["fuse.weight"] = sd["fuse.weight"] * HEAD_SCALE
    if not uniform_head:  # per-channel upsampling filters: the general (not channel-contracted) head kernels
        g = torch.Generator().manual_seed(seed)
        for i in range(4):
            wt = sd[f"upscale.{i}.weight"].clone()
            for c in range(16):
                wt[c, c] = wt[c, c] * (1.0 + 0.05 * c) + 0.01 * torch.randn(wt.shape[2:], generator=g)
            sd[f"upscale.{i}.weight"] = wt
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(sd)
    return net.to(DEV)


def fresh_arena(n, h, w):
    """A new arena (never one of the pool's free list), every byte 0xFF: NaN in bf16 and in fp32."""
    from fosvos_hip import lib
    return torch.full((lib().fosvos_vgg_arena_bytes(n, h, w) + 256,), 255, dtype=torch.uint8, device=DEV)


def arena_views(arena, n, h, w):
    """Device views of every region of the pass's arena (fosvos_vgg_arena_layout)."""
    from fosvos_hip import engine, ops
    L = ops.vgg_arena_layout(n, h, w)
    base = engine._aligned_ptr(arena)[0] - arena.data_ptr()
    sh, sw = L["stage_h"], L["stage_w"]

    def region(off, nbytes, dtype, shape):
        return arena[base + off: base + off + nbytes].view(dtype).view(*shape)

    v = {"act": [], "gact": [], "pooled": [], "gpooled": [], "side": [], "dside": []}
    for c in range(13):
        s, nb = STAGE_OF[c], L["act_bytes"][c]
        shape = (n, sh[s], sw[s], COUT[c])
        v["act"].append(region(L["act"][c], nb, torch.bfloat16, shape))
        v["gact"].append(region(L["gact"][c], nb, torch.bfloat16, shape))
    for i in range(4):
        shape = (n, sh[i + 1], sw[i + 1])
        v["pooled"].append(region(L["pooled"][i], L["pooled_bytes"][i], torch.bfloat16, shape + (STAGE_CH[i],)))
        v["gpooled"].append(region(L["gpooled"][i], L["pooled_bytes"][i], torch.bfloat16, shape + (STAGE_CH[i],)))
        v["side"].append(region(L["side"][i], L["side_bytes"][i], torch.float32, shape + (16,)))
        v["dside"].append(region(L["dside"][i], L["dside_bytes"][i], torch.bfloat16, shape + (32,)))
    v["bits0"] = region(L["bits0"], L["bits0_bytes"], torch.uint8, (n, h, w, 8))
    return v


def run_module(net, x, gt, objective, **flags):
    """forward + class-balanced BCE + backward through the drop-in module (the engine's own flags), on a fresh 0xFF arena.
    Returns the arena, the five outputs, the upstream gradients the backward pass received and the parameter gradients."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    pool = net._packs.arenas
    held = []

    def take(n, h, w, device):
        held.append(fresh_arena(n, h, w))
        return held[-1]

    pool.take = take
    try:
        for k, v in flags.items():
            setattr(net, k, v)
        net.compute_side_outputs = objective == "offline"
        outs = net(x)
        d_outs = [None] * 5
        for i, o in enumerate(outs):
            if o.requires_grad:
                o.register_hook(lambda g, i=i: d_outs.__setitem__(i, g.detach().clone()))
        losses = [cbce(o, gt, size_average=False) for o in (outs if objective == "offline" else outs[4:])]
        total = (1 - 60 / 240) * sum(losses[:4]) + losses[4] if objective == "offline" else losses[0]
        total.backward()
        net.join_gradients()
        torch.cuda.synchronize()
    finally:
        del pool.take
    assert len(held) == 1  # (one pass, one arena)
    grads = {name: p.grad.detach().clone() for name, p in net.named_parameters() if p.grad is not None}
    return held[0], [o.detach() for o in outs], d_outs, grads


def _grad_buffers(net, fill):
    """Gradient buffers of every parameter the online objective produces, pre-filled (fill: name, param -> tensor)."""
    from fosvos_hip import engine
    names = [n for pair in engine._CONV_NAMES for n in pair]
    names += [f"side_prep.{i}.{k}" for i in range(4) for k in ("weight", "bias")] + ["fuse.weight", "fuse.bias"]
    P = dict(net.named_parameters())
    return {n: fill(n, P[n]).contiguous() for n in names}


def run_abi(net, x, d_fused, *, streams, aux, last_pass, buckets=1, accumulate=0, defer_join=0, fill=None):
    """The same pass through the two ABI entry points directly (the online objective, d_fused given), for the flag variants the
    module does not set: forward with or without the second stream, backward with or without it, and the gradient flags.
    Gradients go into buffers pre-filled by `fill` (default: NaN)."""
    from fosvos_hip import VggGrads, check, engine, lib
    n, _, h, w = x.shape
    pool = net._packs.arenas
    P = dict(zip(engine.PARAM_NAMES, net._ordered_params()))
    wts, keep = engine._weights_struct(P, net._packs)
    arena = fresh_arena(n, h, w)
    ap, an = engine._aligned_ptr(arena)
    fused = torch.empty((n, 1, h, w), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream(0).cuda_stream
    aux_h = pool.aux_stream(0) if aux else 0
    if streams:
        check(lib().fosvos_vgg_forward_streams(pool.ctx(0), ctypes.byref(wts), x.data_ptr(), n, h, w, ap, an, fused.data_ptr(),
                                               None, st, aux_h or None), "vgg_forward_streams")
    else:
        check(lib().fosvos_vgg_forward(ctypes.byref(wts), x.data_ptr(), n, h, w, ap, an, fused.data_ptr(), None, 0, st),
              "vgg_forward")
    G = _grad_buffers(net, fill or (lambda _n, p: torch.full_like(p, float("nan"))))
    g = VggGrads()
    for c, (wn, bn) in enumerate(engine._CONV_NAMES):
        g.conv_w[c], g.conv_b[c] = G[wn].data_ptr(), G[bn].data_ptr()
    for i in range(4):
        g.side_w[i], g.side_b[i] = G[f"side_prep.{i}.weight"].data_ptr(), G[f"side_prep.{i}.bias"].data_ptr()
    g.fuse_w, g.fuse_b = G["fuse.weight"].data_ptr(), G["fuse.bias"].data_ptr()
    g.accumulate, g.defer_join, g.bucket_events, g.last_pass_of_cycle = accumulate, defer_join, buckets, last_pass
    check(lib().fosvos_vgg_backward(pool.ctx(0), ctypes.byref(wts), ctypes.byref(g), x.data_ptr(), n, h, w, ap, an,
                                    d_fused.data_ptr(), None, st, aux_h or None), "vgg_backward")
    if defer_join:  # the caller's join: the weight gradients are complete on the auxiliary stream only
        torch.cuda.current_stream(0).wait_stream(pool._aux[0])
    torch.cuda.synchronize()
    del keep
    return arena, fused, G


# ------------------------------------------------------------------------------------------ the checks
def _cpu(t):  # NHWC device view -> fp32 NCHW on the host
    return t.permute(0, 3, 1, 2).float().contiguous().cpu()


def check_invariants(M, v):
    """Whole-tensor invariants on the device: every region written (finite: the 0xFF poison is NaN), no gradient where the
    ReLU output is 0, the pad channels of d_side zero, conv1_1's bit mask equal to its output's sign."""
    for key in ("act", "gact", "pooled", "gpooled", "side", "dside"):
        for i, t in enumerate(v[key]):
            M.add(f"{key}[{i}]", "finite", 0.0 if bool(torch.isfinite(t).all()) else float("inf"))
    for c in range(13):
        leak = int(((v["act"][c] == 0) & (v["gact"][c] != 0)).sum())
        M.add(f"gact[{c}]", "0 at act==0", 0.0 if leak == 0 else float("inf"))
    for i in range(4):
        M.exact(f"dside[{i}]", "pad ch", v["dside"][i][..., 16:], torch.zeros_like(v["dside"][i][..., 16:]))
    n, h, w, _ = v["act"][0].shape
    pos = (v["act"][0] > 0).reshape(n, h, w, 8, 8).to(torch.uint8)
    bits = (pos * (2 ** torch.arange(8, device=pos.device, dtype=torch.uint8))).sum(-1, dtype=torch.uint8)
    M.exact("bits0", "act0>0", v["bits0"], bits)


def head_params(net):  # (float64, on the host)
    P = {k: t.detach().cpu().double() for k, t in net.named_parameters()}
    up = [P[f"upscale.{i}.weight"] for i in range(4)]
    up1 = [P[f"upscale_.{i}.weight"] for i in range(4)]
    dsn_w = torch.stack([P[f"score_dsn.{i}.weight"].reshape(16) for i in range(4)])
    dsn_b = torch.cat([P[f"score_dsn.{i}.bias"] for i in range(4)])
    return up, up1, dsn_w, dsn_b, P["fuse.weight"].reshape(64), P["fuse.bias"]


def check_pass(M, net, x, v, outs, d_outs, grads):
    """Teacher-forced per-layer checks of one pass (v: arena_views, outs / d_outs / grads: what run_module returned)."""
    from fosvos_hip import engine
    P = {k: t.detach().cpu() for k, t in net.named_parameters()}
    x_cpu = x.cpu()
    with_so = d_outs[0] is not None
    H, W = x.shape[2:]

    # ---- head: forward outputs and backward, from the arena's side maps.  In float64: the bias gradients are sums over every
    # pixel of the batch (2 M terms that largely cancel), where an fp32 reference would measure its own summation order
    side = [_cpu(t) for t in v["side"]]
    up, up1, dsn_w, dsn_b, fuse_w, fuse_b = head_params(net)
    leaves = [t.double().requires_grad_(True) for t in side]
    dw_l, db_l = dsn_w.clone().requires_grad_(True), dsn_b.clone().requires_grad_(True)
    fw_l, fb_l = fuse_w.clone().requires_grad_(True), fuse_b.clone().requires_grad_(True)
    ref = _head_ref(leaves, up, up1, dw_l, db_l, fw_l, fb_l, H, W)
    M.rel("head", "fused", outs[4].cpu(), ref[4].detach(), 1e-5)
    if with_so:
        for i in range(4):
            M.rel("head", f"side_out[{i}]", outs[i].cpu(), ref[i].detach(), 1e-5)
        torch.autograd.backward(ref, [d.cpu().double() for d in d_outs])
    else:
        ref[4].backward(d_outs[4].cpu().double())
    for i in range(4):
        M.bf16(f"dside[{i}]", _cpu(v["dside"][i][..., :16]), leaves[i].grad)
    M.rel("fuse", "dw", grads["fuse.weight"].reshape(64).cpu(), fw_l.grad, 2e-5)
    M.rel("fuse", "db", grads["fuse.bias"].cpu(), fb_l.grad, 2e-5)
    if with_so:
        for i in range(4):
            M.rel(f"score_dsn{i}", "dw", grads[f"score_dsn.{i}.weight"].reshape(16).cpu(), dw_l.grad[i], 2e-5)
            M.rel(f"score_dsn{i}", "db", grads[f"score_dsn.{i}.bias"].cpu(), db_l.grad[i:i + 1], 2e-5)
    del leaves, ref

    # ---- stages, last to first: every conv's forward, data gradient and weight gradient from the arena's own operands
    for s in range(4, -1, -1):
        first, last = FIRST[s], LAST[s]
        acts = {c: _cpu(v["act"][c]) for c in range(first, last + 1)}
        gacts = {c: _cpu(v["gact"][c]) for c in range(first, last + 1)}
        if s < 4:  # the pool the stage's last conv fused into its epilogue: exact
            M.exact(f"pooled[{s}]", "maxpool", _cpu(v["pooled"][s]), F.max_pool2d(acts[last], 2, 2, ceil_mode=True))
        mask = (acts[last] > 0).float()
        if s > 0:  # side_prep[s-1]: forward (fp32 output), weight gradient, data gradient into gact[last]
            wn, bn = f"side_prep.{s - 1}.weight", f"side_prep.{s - 1}.bias"
            M.rel(f"side[{s - 1}]", "fwd", side[s - 1], F.conv2d(acts[last], bf(P[wn]), P[bn], padding=1), 2e-5)
            dside = _cpu(v["dside"][s - 1][..., :16])
            dw, db = _wgrad(acts[last], dside, STAGE_CH[s], 16)
            M.rel(f"side_prep{s - 1}", "dw", grads[wn].cpu(), dw, 5e-5)
            M.rel(f"side_prep{s - 1}", "db", grads[bn].cpu(), db, 5e-5)
            term = mask * _dgrad(dside, P[wn])
            del dside
        if s in (1, 2, 3):  # + the next stage's pool backward (first maximum, ReLU mask), fused into the same pass
            xr = acts[last].clone().requires_grad_(True)
            F.max_pool2d(xr, 2, 2, ceil_mode=True).backward(_cpu(v["gpooled"][s]))
            M.bf16_two(f"gact[{last}]", gacts[last], term + mask * xr.grad, term)
        elif s == 4:
            M.bf16(f"gact[{last}]", gacts[last], term)
        else:  # stage 1's output: the pool backward alone, exact
            xr = acts[last].clone().requires_grad_(True)
            F.max_pool2d(xr, 2, 2, ceil_mode=True).backward(_cpu(v["gpooled"][0]))
            M.exact(f"gact[{last}]", "unpool", gacts[last], xr.grad * mask)
        del mask
        stage_in = x_cpu if s == 0 else _cpu(v["pooled"][s - 1])
        for c in range(last, first - 1, -1):
            wn, bn = engine._CONV_NAMES[c]
            if c == 0:  # conv1_1 from the fp32 frame (fp32 weights); its weight gradient contracts the bf16 frame
                M.bf16("act[0]", acts[0], F.relu(F.conv2d(x_cpu, P[wn], P[bn], padding=1)))
                dw, db = _wgrad(bf(x_cpu), gacts[0], 3, 64)
            else:
                xin = stage_in if c == first else acts[c - 1]
                M.bf16(f"act[{c}]", acts[c], F.relu(F.conv2d(xin, bf(P[wn]), P[bn], padding=1)))
                dw, db = _wgrad(xin, gacts[c], CIN[c], COUT[c])
                dg = _dgrad(gacts[c], P[wn])
                if c == first:  # into the pool-output gradient, unmasked (the pool backward applies the producer's mask)
                    M.bf16(f"gpooled[{s - 1}]", _cpu(v["gpooled"][s - 1]), dg)
                else:
                    M.bf16(f"gact[{c - 1}]", gacts[c - 1], (acts[c - 1] > 0).float() * dg)
                del dg
            M.rel(f"conv{c}", "dw", grads[wn].cpu(), dw, 5e-5)
            M.rel(f"conv{c}", "db", grads[bn].cpu(), db, 5e-5)
        del acts, gacts, stage_in


def assert_case_classes(case):
    shape, _, about = CASES[case]
    got = launch_classes(*shape)
    assert about <= got, f"{case}: the plan no longer launches {sorted(about - got)}"


def _frame(shape, seed):
    x, gt = O.synthetic_frame(*shape, seed=seed)
    return x.to(DEV), gt.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c != "step_5x480x854"])
def test_layer_parity(case):
    """One pass of the shipped module per case (engine defaults), every layer against its teacher-forced reference."""
    t0 = time.time()
    assert_case_classes(case)
    shape, objective, _ = CASES[case]
    net = make_net(21, uniform_head=objective == "online")
    if objective == "offline":
        assert net._packs.head_uniform_mask(dict(zip(__import__("fosvos_hip").engine.PARAM_NAMES, net._ordered_params()))) == 0
    x, gt = _frame(shape, 300 + shape[1])
    arena, outs, d_outs, grads = run_module(net, x, gt, objective)
    M = Margins(case)
    v = arena_views(arena, *shape)
    check_invariants(M, v)
    check_pass(M, net, x, v, outs, d_outs, grads)
    print(f"[{case}] {time.time() - t0:.1f} s")
    M.report()


def _max_scale(t):
    return t.abs().max().clamp_min(1e-30)


@pytest.mark.gpu
def test_layer_parity_training_step():
    """The step's pass - five 480x854 frames, online objective, the module with the training loop's flags (gradient buckets
    published, last pass of the cycle, auxiliary stream) - per layer; then the same pass through the ABI with the other flag
    variants, against the first run: the other weight-gradient split count (last_pass_of_cycle=0), one stream for both
    passes, and accumulate=1 into pre-filled buffers with the join deferred to the caller.  Activations and data gradients
    bit for bit; weight gradients within the wgrad tolerance, or exactly prefill + first run where the flags agree."""
    t0 = time.time()
    case = "step_5x480x854"
    assert_case_classes(case)
    shape = CASES[case][0]
    net = make_net(22)
    x, gt = _frame(shape, 305)
    arena, outs, d_outs, grads = run_module(net, x, gt, "online", publish_grad_buckets=True, last_pass_of_cycle=True)
    M = Margins(case)
    v = arena_views(arena, *shape)
    check_invariants(M, v)
    check_pass(M, net, x, v, outs, d_outs, grads)
    print(f"[{case}] per-layer checks {time.time() - t0:.1f} s")
    M.report()

    data = ("gact", "gpooled", "dside")
    variants = [("last_pass_of_cycle=0", dict(streams=True, aux=True, last_pass=0), False),
                ("one stream", dict(streams=False, aux=False, last_pass=1), False),
                ("accumulate+defer_join", dict(streams=True, aux=True, last_pass=1, accumulate=1, defer_join=1), True)]
    for tag, kw, acc in variants:
        V = Margins(f"{case} {tag}")
        prefill = (lambda name, p: torch.linspace(-1.0, 1.0, p.numel(), device=DEV).reshape(p.shape) * _max_scale(grads[name]))
        a2, fused2, G = run_abi(net, x, d_outs[4], fill=prefill if acc else None, **kw)
        v2 = arena_views(a2, *shape)
        V.exact("fused", "vs first", fused2, outs[4])
        for key in ("act", "pooled", "side") + data:
            for i, (t1, t2) in enumerate(zip(v[key], v2[key])):
                V.exact(f"{key}[{i}]", "vs first", t2, t1)
        for name, g2 in G.items():
            if acc:  # one fp32 add of the pass's sum onto what the buffer held
                V.exact(name, "prefill+first", g2, prefill(name, g2) + grads[name].reshape(g2.shape))
            else:
                V.rel(name, "vs first", g2.cpu(), grads[name].reshape(g2.shape).cpu(), 5e-5)
        V.report()
        del a2, v2, G
    print(f"[{case}] {time.time() - t0:.1f} s")
