"""The offline loop's batched accumulation cycle on a real MI355X: the multi-map per-frame loss kernel
(fosvos_cbce_loss_frames_multi) against the existing per-map kernel bit for bit and against the definition, its argument
checks, the autograd node, and ``train_offline._train(..., microbatch_group=N)`` against the one-by-one loop, against itself
on pre-bucketed minibatches, and against the CPU oracle's offline loop.  Tolerances are DESIGN.md section 4's."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_REL_L2 = 0.15           # applied deltas, grouped against one-by-one and against the fp32 oracle
LOSS_RTOL_GROUPED = 2e-2     # epoch losses, grouped against one-by-one
LOSS_RTOL_ORACLE = 3e-2      # losses against the fp32 oracle (test_shipped_offline_train_vs_golden's bar)
SCALES = [0.15, 0.31, 1.7, 0.0123, 0.2, 3.3, 0.9, 1.0 / 7.0]  # distinct, none of them 1


# ------------------------------------------------------------------------------------------ kernel
def _case(n, m, h, w, seed=0):
    """M logit maps and one label batch.  With three frames: frame 1 has no positive pixel, frame 2 only positive ones."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    logits = [(torch.randn(n, 1, h, w, generator=g) * 3).to(DEV) for _ in range(m)]
    label = (torch.rand(n, 1, h, w, generator=g) > 0.7).float()
    if n >= 3:
        label[1] = 0.0
        label[2] = 1.0
    return logits, label.to(DEV), SCALES[:m]


_REFERENCE = {}


def _reference(n, m, h, w, size_average):
    """M calls of the existing per-frame kernel with grad_scale = map_scale[m]; computed once per case."""
    from fosvos_hip import ops
    key = (n, m, h, w, size_average)
    if key not in _REFERENCE:
        logits, label, scales = _case(n, m, h, w)
        parts = [ops.cbce_loss_frames(x, label, size_average=size_average, grad_scale=s) for x, s in zip(logits, scales)]
        _REFERENCE[key] = (torch.stack([p[0] for p in parts], dim=1).cpu(), [p[1].cpu() for p in parts])
    return _REFERENCE[key]


SHAPES = [(3, 5, 24, 36),      # one block per frame
          (3, 5, 40, 52),      # 3 blocks, ragged last block
          (2, 5, 1028, 1024),  # more than kMaxBlocks * 1024 pixels: the stride loop runs
          (2, 1, 40, 52), (2, 8, 40, 52),  # the ends of the range of M
          (1, 5, 61, 107)]     # odd H x W, legal for one frame


@pytest.mark.parametrize("size_average", [False, True])
@pytest.mark.parametrize("n,m,h,w", SHAPES)
def test_multi_loss_equals_the_per_map_kernel_bit_for_bit(n, m, h, w, size_average):
    from fosvos_hip import ops
    logits, label, scales = _case(n, m, h, w)
    ref_loss, ref_grads = _reference(n, m, h, w, size_average)
    losses, grads = ops.cbce_loss_frames_multi(logits, label, scales, size_average=size_average)
    assert tuple(losses.shape) == (n, m) and len(grads) == m
    assert torch.equal(losses.cpu(), ref_loss)
    for k in range(m):
        assert torch.equal(grads[k].cpu(), ref_grads[k]), k
    if n >= 3:  # no positive pixel: every weight of the frame is 0 or multiplies an empty sum
        assert float(losses[1].abs().max()) == 0.0 and all(float(g_[1].abs().max()) == 0.0 for g_ in grads)
        assert float(losses[2].abs().max()) == 0.0
    # a second launch
    losses2, grads2 = ops.cbce_loss_frames_multi(logits, label, scales, size_average=size_average)
    assert torch.equal(losses2, losses) and all(torch.equal(a, b) for a, b in zip(grads2, grads))
    # values only
    losses3, none = ops.cbce_loss_frames_multi(logits, label, scales, size_average=size_average, want_grad=False)
    assert none is None and torch.equal(losses3, losses)


@pytest.mark.parametrize("size_average", [False, True])
@pytest.mark.parametrize("n,m,h,w", [SHAPES[1], SHAPES[2], SHAPES[5]])
def test_staged_multi_loss_equals_the_one_call(n, m, h, w, size_average):
    """Count first, finish last, other work - this library's and torch's, on the same stream - in between."""
    from fosvos_hip import ops
    logits, label, scales = _case(n, m, h, w)
    ref_loss, ref_grads = _reference(n, m, h, w, size_average)
    other_x, other_y, _ = _case(2, 1, 40, 52, seed=7)
    staged = ops.CbceFramesMultiStaged(label, m)
    ops.cbce_loss_frames(other_x[0], other_y)          # (uses the ops' shared scratch: the staged loss has its own)
    busy = torch.randn(256, 256, device=DEV) @ torch.randn(256, 256, device=DEV)
    losses, grads = staged.loss(logits, scales, size_average=size_average)
    ops.cbce_loss_frames_multi(other_x, other_y, [2.0])
    busy = busy @ busy
    assert staged.finish() is losses
    assert torch.equal(losses.cpu(), ref_loss)
    for k in range(m):
        assert torch.equal(grads[k].cpu(), ref_grads[k]), k
    del busy


def test_multi_loss_against_the_definition():
    """float64 numpy of src/layers/osvos_layers.py:17-44 per frame and map, on the 40x52 case: gradients within 2e-5 of the
    largest element, loss 1e-5 relative."""
    from fosvos_hip import ops
    n, m, h, w = SHAPES[1]
    logits, label, scales = _case(n, m, h, w)
    for size_average in (False, True):
        losses, grads = ops.cbce_loss_frames_multi(logits, label, scales, size_average=size_average)
        losses = losses.cpu().double().numpy()
        for i in range(n):
            y = (label[i].cpu().double().numpy() >= 0.5).astype(np.float64)
            n_tot = float(y.size)
            n_pos = y.sum()
            n_neg = n_tot - n_pos
            for k in range(m):
                x = logits[k][i].cpu().double().numpy()
                val = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
                loss = n_neg / n_tot * (y * val).sum() + n_pos / n_tot * ((1 - y) * val).sum()
                grad = np.where(y > 0, n_neg / n_tot, n_pos / n_tot) * (1.0 / (1.0 + np.exp(-x)) - y) * scales[k]
                if size_average:
                    loss, grad = loss / n_tot, grad / n_tot
                assert abs(losses[i, k] - loss) <= 1e-5 * abs(loss), (i, k, losses[i, k], loss)
                err = np.abs(grads[k][i].cpu().double().numpy() - grad).max()
                assert err <= 2e-5 * np.abs(grad).max(), (i, k, err)


def test_multi_loss_rejects_bad_arguments_before_any_launch():
    import fosvos_hip
    from fosvos_hip import ops
    logits, label, scales = _case(2, 5, 40, 52)
    odd_logits, odd_label, _ = _case(2, 5, 61, 107)
    nine = logits + logits[:4]
    need = ops.cbce_multi_workspace_bytes(label, 5)
    assert need == 2 * 5 * fosvos_hip.lib().fosvos_cbce_workspace_bytes(40 * 52)
    short = torch.empty((need - 8,), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with fosvos_hip.LaunchProfile(0, max_launches=16) as prof:
        with pytest.raises(fosvos_hip.FosvosHipError, match="n_maps=0"):
            ops.cbce_loss_frames_multi([], label, [])
        with pytest.raises(fosvos_hip.FosvosHipError, match="n_maps=9"):
            ops.cbce_loss_frames_multi(nine, label, SCALES + [0.5])
        with pytest.raises(fosvos_hip.FosvosHipError, match="16-byte boundary"):
            ops.cbce_loss_frames_multi(odd_logits, odd_label, scales)
        with pytest.raises(fosvos_hip.FosvosHipError, match="16-byte boundary"):
            ops.CbceFramesMultiStaged(odd_label, 5)
        with pytest.raises((RuntimeError, ValueError)):  # a label on another device
            ops.cbce_loss_frames_multi(logits, label.cpu(), scales)
        with pytest.raises(fosvos_hip.FosvosHipError, match="workspace"):
            ops.cbce_loss_frames_multi(logits, label, scales, workspace=short)
        with pytest.raises(ValueError):
            ops.cbce_loss_frames_multi(logits, label, scales[:4])
        with pytest.raises(fosvos_hip.FosvosHipError, match="aligned"):  # a view that starts off a 16-byte boundary
            ops.cbce_loss_frames_multi([logits[0].reshape(-1)[1:1 + 40 * 52].reshape(1, 1, 40, 52)] * 5,
                                       label[:1], scales)
    assert prof.records == {}, prof.records
    # the same arguments with the workspace the library asks for are accepted
    full = torch.empty((need,), dtype=torch.uint8, device=DEV)
    losses, _ = ops.cbce_loss_frames_multi(logits, label, scales, workspace=full)
    assert torch.equal(losses.cpu(), _reference(2, 5, 40, 52, True)[0])


def test_multi_loss_autograd_leaves_the_kernels_gradient():
    """One autograd node over all maps: .sum().backward() leaves in each output's .grad exactly the kernel's gradient, and a
    backward pass with the announced seed passes the gradients through without touching them."""
    import layers.osvos_layers as L
    from fosvos_hip import ops
    n, m, h, w = SHAPES[1]
    logits, label, scales = _case(n, m, h, w)
    _, ref_grads = ops.cbce_loss_frames_multi(logits, label, scales, size_average=False)
    ref_loss, _ = _reference(n, m, h, w, False)
    outs = [x.clone().requires_grad_(True) for x in logits]
    losses = L.class_balanced_cross_entropy_loss_frames_multi(outs, label, scales)
    assert tuple(losses.shape) == (n, m) and torch.equal(losses.detach().cpu(), ref_loss)
    losses.sum().backward()
    for k in range(m):
        assert torch.equal(outs[k].grad, ref_grads[k]), k
    # announced seed, staged
    outs = [x.clone().requires_grad_(True) for x in logits]
    ones = torch.ones((n + 2, m), device=DEV)
    staged = L.stage_frames_loss_multi(label, m)
    hits = L.seed_hits
    losses = L.class_balanced_cross_entropy_loss_frames_multi(outs, label, scales, backward_seed=(ones, 1.0), staged=staged)
    losses.backward(ones[:n])
    staged.finish()
    assert L.seed_hits == hits + 1
    assert torch.equal(losses.detach().cpu(), ref_loss)
    for k in range(m):
        assert torch.equal(outs[k].grad, ref_grads[k]), k
    # any other incoming gradient is still applied
    outs = [x.clone().requires_grad_(True) for x in logits]
    losses = L.class_balanced_cross_entropy_loss_frames_multi(outs, label, scales, backward_seed=(ones, 1.0))
    (losses * 2).sum().backward()
    assert torch.equal(outs[3].grad, ref_grads[3] * 2)
    with pytest.raises(ValueError):
        L.class_balanced_cross_entropy_loss_frames_multi(outs[:2], label[:, :, :-1], scales[:2])


# ------------------------------------------------------------------------------------------ loop
class _NullWriter:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


class _EpochLoader:
    """A dataloader that yields `epochs[i]` on its i-th pass and nothing afterwards: the shipped `_train` then runs exactly
    len(epochs) epochs of a 240-epoch schedule (`1 - epoch / n_epochs` needs both numbers), the later ones over nothing."""

    def __init__(self, epochs):
        self._epochs, self._pass = [list(e) for e in epochs], 0

    def __len__(self):
        return len(self._epochs[0])

    def __iter__(self):
        i, self._pass = self._pass, self._pass + 1
        return iter(self._epochs[i] if i < len(self._epochs) else ())


def _make_net(seed):
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    sd = O.make_state_dict(seed)
    net.load_state_dict(sd)
    return net.to(DEV), sd


def _train_offline(epochs, seed, avg, group, lr=1e-8):
    """`train_offline._train` from epoch 60 of 240 on a freshly seeded net, at the recipe's learning rate unless told otherwise
    (src/util/network_provider.py:98-125); returns (weights, initial state, result, pass shapes)."""
    import train_offline
    from util.network_provider import VGGOfflineProvider
    net, sd = _make_net(seed)
    prov = VGGOfflineProvider.__new__(VGGOfflineProvider)
    prov.network = net
    prov.name = "vgg16"
    opt = prov.get_optimizer(learning_rate=lr)
    shapes = []
    fwd = net.forward
    net.forward = lambda x: (shapes.append(tuple(x.shape)), fwd(x))[1]
    train_offline.data_parallel = False
    kw = {} if group is None else {"microbatch_group": group}
    ret = train_offline._train(prov, _EpochLoader(epochs), None, opt, _NullWriter(), 60, 240, avg, 10 ** 9, False, 5, **kw)
    del net.forward
    assert net.defer_wgrad_join is False
    return {n_: p.detach().clone() for n_, p in net.named_parameters()}, sd, ret, shapes


def _delta_ratios(got_w, ref_w, sd, frozen=("upscale",)):
    """Per tensor: (rel-L2 of the applied delta against the reference run's, the same before the allowance, |delta| of the
    reference over the allowance).  The formula is test_gpu_network._check_deltas': an update of lr * grad sits near the fp32
    resolution of the weight, so two steps of it per element are not counted.  Frozen tensors must not have moved at all."""
    ratios = {}
    for name, ref in ref_w.items():
        init = sd[name].to(ref.device)
        d_ref = (ref - init).double().reshape(-1)
        d_got = (got_w[name].to(ref.device) - init).double().reshape(-1)
        if name.startswith(frozen):
            assert float(d_got.abs().max()) == 0.0 and float(d_ref.abs().max()) == 0.0, name
            continue
        if float(d_ref.abs().max()) == 0.0:
            continue
        ulp = float(np.spacing(np.float32(max(sd[name].abs().max().item(), 1e-30))))
        noise = 2 * ulp * float(np.sqrt(d_ref.numel()))
        err, size = float((d_got - d_ref).norm()), float(d_ref.norm())
        ratios[name] = (max(err - noise, 0.0) / size, err / size, size / noise)
    return ratios


def _check_ratios(tag, ratios):
    """Every tensor within GRAD_REL_L2; and the comparison can see an error of that size: in at least 30 tensors the
    reference's delta is ten times the fp32 allowance or more."""
    worst = max(ratios, key=lambda k: ratios[k][1])
    rms = float(np.sqrt(np.mean(np.square([r[0] for r in ratios.values()]))))
    print(f"[{tag}] worst delta rel-L2 {ratios[worst][0]:.3e} ({ratios[worst][1]:.3e} before the fp32 allowance) at {worst}; "
          f"RMS {rms:.3e} over {len(ratios)} tensors")
    assert sum(r[2] >= 10.0 for r in ratios.values()) >= 30, sorted(r[2] for r in ratios.values())
    for name, r in ratios.items():
        assert r[0] <= GRAD_REL_L2, (name, r)


SIZES = {"a": (48, 86), "b": (64, 108), "o": (61, 107)}  # "o": odd H x W - it must take the one-frame path
DRAWS = ["a", "b", "a", "o", "b", "a", "a", "b", "o", "b", "a", "b"]  # 12 one-frame minibatches per epoch


def _minibatches():
    frames = [O.synthetic_frame(1, *SIZES[t], seed=400 + i) for i, t in enumerate(DRAWS)]
    return [{"image": x, "gt": gt} for x, gt in frames]


_LOOP_RUNS = {}


def _loop_run(group):
    """2 epochs of the 12 minibatches, a step every 5 (the cycles straddle the epoch end); shared by the tests below."""
    if group not in _LOOP_RUNS:
        mbs = _minibatches()
        _LOOP_RUNS[group] = _train_offline([mbs, mbs], 31, 5, group)
    return _LOOP_RUNS[group]


def test_grouped_offline_loop_against_one_by_one():
    """microbatch_group = 5 against 1 on the same minibatches and the same seeded net: epoch losses within 2 %, every tensor's
    delta rel-L2 <= 0.15, frozen tensors exactly unchanged (the bars DESIGN.md section 4 states for grouped against
    one-by-one), fewer passes than iterations."""
    w1, sd, ret1, shapes1 = _loop_run(1)
    w5, _, ret5, shapes5 = _loop_run(5)
    assert ret1["iterations"] == ret5["iterations"] == 24
    assert ret1["passes"] == 24 == len(shapes1) and all(s[0] == 1 for s in shapes1)
    assert ret5["passes"] == len(shapes5) and ret5["passes"] < ret5["iterations"]
    # the windows are [0-4] [5-9] [10-11] | [0-2] [3-7] [8-11]: "a" and "b" buckets, every odd frame alone at its place
    A, B, Od = (3, 48, 86), (3, 64, 108), (3, 61, 107)
    assert shapes5 == [(2,) + A, (2,) + B, (1,) + Od,   (2,) + A, (2,) + B, (1,) + Od,   (1,) + A, (1,) + B,
                       (2,) + A, (1,) + B,   (1,) + Od, (2,) + B, (2,) + A,   (1,) + Od, (2,) + B, (1,) + A]
    assert len(ret5["losses_train"]) == 2 and len(ret5["losses_train"][0]) == 5
    print("epoch losses, grouped:", ret5["losses_train"], "one by one:", ret1["losses_train"])
    np.testing.assert_allclose(ret5["losses_train"], ret1["losses_train"], rtol=LOSS_RTOL_GROUPED)
    _check_ratios("offline group 5 vs one-by-one", _delta_ratios(w5, w1, sd))


def test_offline_bucketing_is_what_it_says():
    """The same minibatches in draw order and re-ordered so that every window lists its buckets pass by pass run the
    IDENTICAL passes: weights and loss log bit for bit."""
    mbs = _minibatches()
    windows = [[(0, 5), (5, 10), (10, 12)], [(0, 3), (3, 8), (8, 12)]]  # a step every 5, 12 minibatches per epoch

    def by_bucket(window):
        keys = [mb["image"].shape[-2:] if mb["image"].shape[-2:].numel() % 4 == 0 else ("alone", i)
                for i, mb in enumerate(window)]
        first = {}
        for i, k in enumerate(keys):
            first.setdefault(k, i)
        return [window[i] for i in sorted(range(len(window)), key=lambda i: first[keys[i]])]  # (stable)

    presorted = [[mb for lo, hi in wins for mb in by_bucket(mbs[lo:hi])] for wins in windows]
    assert any(a is not b for a, b in zip(presorted[0], mbs))
    w_draw, _, ret_draw, shapes_draw = _loop_run(5)
    w_sorted, _, ret_sorted, shapes_sorted = _train_offline(presorted, 31, 5, 5)
    assert shapes_sorted == shapes_draw
    assert ret_sorted["losses_train"] == ret_draw["losses_train"]
    for name in w_draw:
        assert torch.equal(w_draw[name], w_sorted[name]), name


def test_grouped_offline_loop_against_the_oracle(monkeypatch):
    """`oracle.osvos_ref.offline_loop` (fp32, CPU) against the shipped loop at microbatch_group = 4: 8 one-frame iterations
    cycling 4 frames, epoch 60 of 240, a step every 4; per-iteration losses rtol 3e-2, deltas rel-L2 <= 0.15."""
    import train_offline
    frames = [O.synthetic_frame(1, 48, 86, seed=500 + i) for i in range(4)]
    sd = O.make_state_dict(33)
    trace, ref = O.offline_loop(sd, [x for x, _ in frames], [gt for _, gt in frames], 8, epoch=60, n_epochs=240,
                                avg_grad_every_n=4, lr=1e-6)
    seen = []
    real = train_offline.class_balanced_cross_entropy_loss_frames_multi

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]

    monkeypatch.setattr(train_offline, "class_balanced_cross_entropy_loss_frames_multi", spy)
    loader = [{"image": x, "gt": gt} for x, gt in frames] * 2
    w, sd_, ret, shapes = _train_offline([loader], 33, 4, 4, lr=1e-6)  # (the rate of the golden offline schedule)
    assert shapes == [(4, 3, 48, 86)] * 2 and ret["passes"] == 2 and ret["iterations"] == 8
    per_iteration = torch.cat([t.detach() for t in seen]).cpu().numpy()  # [8,5]: a pass holds its frames in draw order
    print("per-iteration losses, shipped:", per_iteration.tolist(), "oracle:", trace)
    np.testing.assert_allclose(per_iteration, np.array(trace), rtol=LOSS_RTOL_ORACLE)
    np.testing.assert_allclose(np.array(ret["losses_train"][0]), np.array(trace).mean(axis=0), rtol=LOSS_RTOL_ORACLE)
    _check_ratios("offline group 4 vs oracle", _delta_ratios(w, {k: v for k, v in ref.items() if k in w}, sd))


def test_grouped_offline_loop_guards():
    """data_parallel with a group raises at entry; a minibatch that holds two frames keeps the class balance of its whole
    tensor: a grouped run of such minibatches leaves the weights of the ungrouped run, bit for bit."""
    import train_offline
    x, gt = O.synthetic_frame(2, 33, 47, seed=23)
    pairs = [{"image": x, "gt": gt}] * 4
    w1, _, ret1, shapes1 = _train_offline([pairs], 8, 2, None)
    w5, _, ret5, shapes5 = _train_offline([pairs], 8, 2, 5)
    assert shapes1 == shapes5 == [(2, 3, 33, 47)] * 4
    assert ret5["passes"] == ret5["iterations"] == 4
    assert ret5["losses_train"] == ret1["losses_train"]
    for name in w1:
        assert torch.equal(w1[name], w5[name]), name
    net, _ = _make_net(8)
    prov = type("P", (), {"network": net, "name": "vgg16"})()
    train_offline.data_parallel = True
    try:
        with pytest.raises(ValueError, match="data_parallel"):
            train_offline._train(prov, pairs, None, None, _NullWriter(), 60, 240, 2, 10 ** 9, False, 5, microbatch_group=2)
    finally:
        train_offline.data_parallel = False
