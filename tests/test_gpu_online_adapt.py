"""Online adaptation on a real MI355X: the distance gate and the labelling (csrc/adapt.hip) against their numpy definitions
(util/online_adapt.py) with exact equality, the void form of the class-balanced loss (csrc/loss.hip) against the plain form
bit for bit and against ``cbce_void`` within the loss kernel's own tolerances, its autograd face, and ``test_adaptive`` end
to end on a small net."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import osvos_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import online_adapt_cases as C  # noqa: E402
from util import experiment_helper, io_helper, online_adapt as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_REL_L2 = 0.15  # tests/test_gpu_network.py: batched against per-frame gradients


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(a, ref):
    return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


# ------------------------------------------------------------------------------------------ distance_gate
@pytest.mark.parametrize("shape", C.SHAPES, ids=["%dx%d" % s for s in C.SHAPES])
def test_distance_gate_equals_far_from(shape):
    from fosvos_hip import ops
    n = 0
    for name, mask, d in C.gate_cases():
        if mask.shape != shape:
            continue
        for invert in (False, True):
            got = ops.distance_gate(dev(mask[None]), d, invert)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + shape
            assert torch.equal(got.cpu(), torch.from_numpy(A.far_from(mask, d, invert)[None])), (name, invert)
            n += 1
    assert n >= 6 * 6 * 2


def test_distance_gate_frames_and_out():
    from fosvos_hip import ops
    for name, stack, d in C.stacks():
        for invert in (False, True):
            want = torch.from_numpy(np.stack([A.far_from(m, d, invert) for m in stack]))
            out = torch.full(stack.shape, 0xA5, dtype=torch.uint8, device=DEV)
            back = ops.distance_gate(dev(stack), d, invert, out=out)
            assert back is out and torch.equal(out.cpu(), want), (name, invert)
    m = dev(np.zeros((1, 4, 4), np.uint8))
    for bad in (lambda: ops.distance_gate(m, -1), lambda: ops.distance_gate(m, 4096), lambda: ops.distance_gate(m, 1.5),
                lambda: ops.distance_gate(m[0], 1), lambda: ops.distance_gate(m.float(), 1),
                lambda: ops.distance_gate(m, 1, out=m), lambda: ops.distance_gate(m, 1, out=torch.empty((1, 4, 5), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.distance_gate(m.cpu(), 1)


# ------------------------------------------------------------------------------------------ adapt_labels
def test_adapt_labels_equals_the_definition():
    from fosvos_hip import ops
    n = 0
    for name, x, m, t, d, e in C.label_cases():
        label, void, counts = ops.adapt_labels(dev(x[None, None]), dev(m[None]), t, d, e)
        want_l, want_v, want_c = A.adapt_labels(x, m, t, d, e)
        assert torch.equal(label.cpu(), torch.from_numpy(want_l)[None, None]), name
        assert torch.equal(void.cpu(), torch.from_numpy(want_v)[None, None]), name
        assert counts.cpu().tolist() == [want_c.tolist()], name
        # the call zeroes its counts: a second call into the same rows gives the same numbers
        ops.adapt_labels(dev(x[None, None]), dev(m[None]), t, d, e, label=label, void=void, counts=counts)
        assert counts.cpu().tolist() == [want_c.tolist()], name
        n += 1
    assert n >= 5 * 2 * 7


def test_adapt_labels_frames_and_arguments():
    from fosvos_hip import ops
    h, w = 49, 83
    xs = np.stack([C.logits_for(h, w, seed=s)[0] for s in range(3)])
    ms = C.masks(h, w, 5)
    masks = np.stack([C.ellipse(h, w), ms["empty"], ms["corner"]])
    t = C.pos_logit(C.NET_LIKE["pos_prob"])
    counts = torch.full((5, 3), -7, dtype=torch.int32, device=DEV)
    for e in C.ERODES:
        label, void, rows = ops.adapt_labels(dev(xs[:, None]), dev(masks), t, C.NET_LIKE["neg_distance"], e, counts=counts[1:4])
        for k in range(3):
            want_l, want_v, want_c = A.adapt_labels(xs[k], masks[k], t, C.NET_LIKE["neg_distance"], e)
            assert torch.equal(label[k, 0].cpu(), torch.from_numpy(want_l)) and torch.equal(void[k, 0].cpu(), torch.from_numpy(want_v))
            assert counts[1 + k].cpu().tolist() == want_c.tolist()
        assert counts[0].cpu().tolist() == [-7] * 3 and counts[4].cpu().tolist() == [-7] * 3   # the neighbours' rows stay
    x, m = dev(xs[:1, None]), dev(masks[:1])
    for bad in (lambda: ops.adapt_labels(x, m, t, -1), lambda: ops.adapt_labels(x, m, t, 4096), lambda: ops.adapt_labels(x, m, t, 5, 4096),
                lambda: ops.adapt_labels(x, m, t, 5, 1.0), lambda: ops.adapt_labels(x, m, float("nan"), 5),
                lambda: ops.adapt_labels(x, m[:, :4], t, 5), lambda: ops.adapt_labels(x[0], m, t, 5),
                lambda: ops.adapt_labels(x, m, t, 5, counts=torch.zeros((1, 3), dtype=torch.int64, device=DEV)),
                lambda: ops.adapt_labels(x, m, t, 5, void=torch.zeros((1, h, w), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.adapt_labels(x, m.cpu(), t, 5)


# ------------------------------------------------------------------------------------------ the void loss
LOSS_SHAPES = [(1, 1, 3, 5), (2, 1, 40, 52), (3, 1, 48, 86)]


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["%dx%dx%dx%d" % s for s in LOSS_SHAPES])
@pytest.mark.parametrize("size_average", [False, True])
def test_void_loss_with_no_void_is_the_plain_loss_bit_for_bit(shape, size_average):
    from fosvos_hip import ops
    n, _, h, w = shape
    x, y, _ = C.loss_inputs(n, h, w)
    x, y = dev(x), dev(y)
    want_l, want_g = ops.cbce_loss_frames(x, y, size_average=size_average, grad_scale=0.2)
    got_l, got_g = ops.cbce_loss_frames(x, y, size_average=size_average, grad_scale=0.2, void=torch.zeros(shape, dtype=torch.uint8, device=DEV))
    assert torch.equal(got_l, want_l) and torch.equal(got_g, want_g)
    only_l, none = ops.cbce_loss_frames(x, y, size_average=size_average, want_grad=False, void=torch.zeros(shape, dtype=torch.uint8, device=DEV))
    assert none is None and torch.equal(only_l, want_l)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=["%dx%dx%dx%d" % s for s in LOSS_SHAPES])
def test_void_loss_against_the_definition(shape):
    from fosvos_hip import ops
    n, _, h, w = shape
    x, y, v = C.loss_inputs(n, h, w)
    for size_average in (False, True):
        loss, grad = ops.cbce_loss_frames(dev(x), dev(y), size_average=size_average, void=dev(v))
        again_l, again_g = ops.cbce_loss_frames(dev(x), dev(y), size_average=size_average, void=dev(v))
        assert torch.equal(loss, again_l) and torch.equal(grad, again_g)                  # two calls agree bit for bit
        for k in range(n):
            ref, gref = A.cbce_void(x[k], y[k], v[k], size_average)
            print("frame %d of %s size_average=%s: loss %.9g (definition %.9g), gradient rel-err %.3g"
                  % (k, shape, size_average, loss[k].item(), ref, rel_err(grad[k].cpu().double(), torch.from_numpy(gref))))
            assert abs(loss[k].item() - ref) <= 2e-6 * abs(ref) + 1e-6
            assert rel_err(grad[k].cpu().double(), torch.from_numpy(gref)) < 1e-6
            # frame k of the batch is the frame alone
            one_l, one_g = ops.cbce_loss_frames(dev(x[k:k + 1]), dev(y[k:k + 1]), size_average=size_average, void=dev(v[k:k + 1]))
            assert torch.equal(one_l, loss[k:k + 1]) and torch.equal(one_g, grad[k:k + 1])
        # +0.0, bit for bit, on every void pixel
        bits = grad.cpu().view(torch.int32)
        assert (bits[torch.from_numpy(v != 0)] == 0).all()
        # whatever stands in a void pixel's logit changes no bit of the result
        for poison in (np.nan, np.inf, -np.inf):
            xp = x.copy()
            xp[v != 0] = poison
            p_l, p_g = ops.cbce_loss_frames(dev(xp), dev(y), size_average=size_average, void=dev(v))
            assert torch.equal(p_l, loss) and torch.equal(p_g.view(torch.int32), grad.view(torch.int32)), poison
        # every pixel void: loss 0, gradient +0.0
        z_l, z_g = ops.cbce_loss_frames(dev(xp), dev(y), size_average=size_average, void=torch.full(shape, 3, dtype=torch.uint8, device=DEV))
        assert (z_l == 0).all() and (z_g.view(torch.int32) == 0).all()


def test_void_loss_entry_rejects_bad_arguments_before_any_launch():
    """The C entry called directly: each bad argument is refused with its message and without a single launch; the same
    call with the workspace the library asks for gives ops.cbce_loss_frames' values."""
    import fosvos_hip
    from fosvos_hip import ops
    L = fosvos_hip.lib()
    x, y, v = (dev(a) for a in C.loss_inputs(2, 40, 52))
    per = 40 * 52
    need = L.fosvos_cbce_void_workspace_bytes(per, 2)
    assert need == 2 * L.fosvos_cbce_workspace_bytes(per) + 2 * 1024 * 8
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    losses, grad = torch.empty((2,), device=DEV), torch.empty_like(x)
    X, Y, V, LO, G, W = x.data_ptr(), y.data_ptr(), v.data_ptr(), losses.data_ptr(), grad.data_ptr(), ws.data_ptr()
    d, st = 0, torch.cuda.current_stream(0).cuda_stream
    cases = [("16-byte boundary", lambda: L.fosvos_cbce_loss_frames_void(X, Y, V, 15, 2, 0, 1.0, LO, G, W, need, d, st)),
             ("workspace", lambda: L.fosvos_cbce_loss_frames_void(X, Y, V, per, 2, 0, 1.0, LO, G, W, need - 8, d, st)),
             ("aligned", lambda: L.fosvos_cbce_loss_frames_void(X + 4, Y, V, per, 1, 0, 1.0, LO, G, W, need, d, st)),
             ("4-byte", lambda: L.fosvos_cbce_loss_frames_void(X, Y, V + 1, per, 1, 0, 1.0, LO, G, W, need, d, st)),
             ("null void", lambda: L.fosvos_cbce_loss_frames_void(X, Y, None, per, 2, 0, 1.0, LO, G, W, need, d, st)),
             ("null", lambda: L.fosvos_cbce_loss_frames_void(X, Y, V, per, 2, 0, 1.0, None, G, W, need, d, st)),
             ("n_frames", lambda: L.fosvos_cbce_loss_frames_void(X, Y, V, per, 0, 0, 1.0, LO, G, W, need, d, st))]
    torch.cuda.synchronize()
    with fosvos_hip.LaunchProfile(0, max_launches=16) as prof:
        for fragment, call in cases:
            with pytest.raises(fosvos_hip.FosvosHipError, match=fragment):
                fosvos_hip.check(call(), "cbce_loss_frames_void")
    assert prof.records == {}, prof.records
    fosvos_hip.check(L.fosvos_cbce_loss_frames_void(X, Y, V, per, 2, 0, 0.2, LO, G, W, need, d, st), "cbce_loss_frames_void")
    want_l, want_g = ops.cbce_loss_frames(x, y, size_average=False, grad_scale=0.2, void=v)
    assert torch.equal(losses, want_l) and torch.equal(grad, want_g)
    for bad in (lambda: ops.cbce_loss_frames(x, y, void=v.float()), lambda: ops.cbce_loss_frames(x, y, void=v[:1])):
        with pytest.raises((TypeError, ValueError)):
            bad()


def test_void_loss_through_autograd():
    from fosvos_hip import ops
    from layers import osvos_layers as Ls
    x, y, v = (dev(a) for a in C.loss_inputs(3, 40, 52))
    want_l, want_g = ops.cbce_loss_frames(x[:1], y[:1], size_average=False, void=v[:1])
    seed = torch.ones((), device=DEV) / 5
    # the whole-tensor loss: the kernel's gradient lands in x.grad, with and without an announced seed
    leaf = x[:1].clone().requires_grad_(True)
    loss = Ls.class_balanced_cross_entropy_loss(leaf, y[:1], size_average=False, void_pixels=v[:1])
    assert loss.dim() == 0 and torch.equal(loss.detach(), want_l[0])
    loss.backward()
    assert torch.equal(leaf.grad, want_g)
    hits = Ls.seed_hits
    scaled_l, scaled_g = ops.cbce_loss_frames(x[:1], y[:1], size_average=False, void=v[:1], grad_scale=0.2)
    leaf = x[:1].clone().requires_grad_(True)
    Ls.class_balanced_cross_entropy_loss(leaf, y[:1], size_average=False, void_pixels=v[:1], backward_seed=(seed, 0.2)).backward(seed)
    assert Ls.seed_hits == hits + 1 and torch.equal(leaf.grad, scaled_g)
    leaf = x[:1].clone().requires_grad_(True)
    Ls.class_balanced_cross_entropy_loss(leaf, y[:1], size_average=False, void_pixels=v[:1], backward_seed=(seed, 0.2)).backward()
    assert rel_err(leaf.grad, want_g) < 1e-6                                       # another incoming gradient: divided first
    # the whole tensor of three frames is ONE loss: the classes are balanced over all its valid pixels
    ref, gref = A.cbce_void(x.cpu().numpy(), y.cpu().numpy(), v.cpu().numpy(), False)
    leaf = x.clone().requires_grad_(True)
    loss = Ls.class_balanced_cross_entropy_loss(leaf, y, size_average=False, void_pixels=v)
    loss.backward()
    assert abs(loss.item() - ref) <= 2e-6 * abs(ref) + 1e-6 and rel_err(leaf.grad.cpu().double(), torch.from_numpy(gref)) < 1e-6
    # per frame, with a seed per frame
    all_l, all_g = ops.cbce_loss_frames(x, y, size_average=False, void=v)
    leaf = x.clone().requires_grad_(True)
    losses = Ls.class_balanced_cross_entropy_loss_frames(leaf, y, size_average=False, void_pixels=v)
    assert torch.equal(losses.detach(), all_l)
    w = torch.tensor([1.0, 0.5, 2.0], device=DEV)
    losses.backward(w)
    assert torch.equal(leaf.grad, all_g * w.view(3, 1, 1, 1))
    seed3 = torch.full((3,), 0.2, device=DEV)
    leaf = x.clone().requires_grad_(True)
    Ls.class_balanced_cross_entropy_loss_frames(leaf, y, size_average=False, void_pixels=v, backward_seed=(seed3, 0.2)).backward(seed3)
    assert torch.equal(leaf.grad, ops.cbce_loss_frames(x, y, size_average=False, void=v, grad_scale=0.2)[1])
    # what does not combine is refused with the reason
    counts = torch.tensor([10.0, 100.0], dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="batch_counts"):
        Ls.class_balanced_cross_entropy_loss(x, y, void_pixels=v, batch_counts=counts)
    with pytest.raises(ValueError, match="staged"):
        Ls.class_balanced_cross_entropy_loss_frames(x, y, void_pixels=v, staged=Ls.stage_frames_loss(y))
    with pytest.raises(ValueError, match="uint8"):
        Ls.class_balanced_cross_entropy_loss(x, y, void_pixels=v.float())
    with pytest.raises(ValueError, match="void_pixels"):
        Ls.class_balanced_cross_entropy_loss_frames(x, y, void_pixels=v[:2])


# ------------------------------------------------------------------------------------------ test_adaptive
SIZE = (48, 84)
TRAINED = ("stages.", "side_prep.", "fuse.")  # the parameters the online recipe trains; upscale / upscale_ are frozen (lr 0)


class Centred(torch.nn.Module):
    """The real OSVOS_VGG forward with each frame's median taken off the fused logits (about half of the pixels are object,
    ragged contours), so that the pseudo-labels hold all three classes."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        outs = list(self.net.forward(x))
        fused = outs[-1]
        outs[-1] = fused - fused.flatten(1).median(dim=1).values.view(-1, 1, 1, 1)
        return outs


class Provider:
    def __init__(self, seed=2):
        from networks.osvos_vgg import OSVOS_VGG
        from util.network_provider import VGGOnlineProvider
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        self.inner = VGGOnlineProvider.__new__(VGGOnlineProvider)
        self.inner.network = net.to(DEV)
        self.network = Centred(self.inner.network)
        self.learning_rates = []

    def get_optimizer(self, learning_rate=1e-8):
        self.learning_rates.append(learning_rate)
        return self.inner.get_optimizer(learning_rate=learning_rate)

    def weights(self):
        return {k: p.detach().clone() for k, p in self.inner.network.named_parameters()}


def sequence(n_frames=3):
    loader = io_helper.get_data_loader_test(None, 1, "blob", synthetic=SIZE, n_frames=n_frames)
    train = io_helper.get_data_loader_train(None, 1, "blob", synthetic=SIZE)
    return loader, {"image": train.dataset[0]["image"], "gt": train.dataset[0]["gt"]}


def test_adaptive_without_steps_is_test_fast(tmp_path):
    from fosvos_hip.options import AdaptOptions
    prov = Provider()
    loader, first = sequence()
    before = prov.weights()
    fast = experiment_helper.test_fast(prov, loader, tmp_path / "fast", loader.dataset.annotation, group=1, seq_name="blob")
    score = experiment_helper.test_adaptive(prov, loader, tmp_path / "adapt", first, AdaptOptions(steps=0, neg_distance=12, erode=2),
                                            loader.dataset.annotation, seq_name="blob")
    assert prov.learning_rates == []                                                # no optimizer was constructed
    names = sorted(p.name for p in (tmp_path / "fast" / "blob").iterdir())
    assert names == ["%05d.png" % k for k in range(3)] == sorted(p.name for p in (tmp_path / "adapt" / "blob").iterdir())
    for name in names:
        assert (tmp_path / "fast" / "blob" / name).read_bytes() == (tmp_path / "adapt" / "blob" / name).read_bytes(), name
    for key in ("counts", "J", "F", "fnames", "scored", "radius"):
        assert score[key] == fast[key], key
    after = prov.weights()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert experiment_helper.last_fast["png_bytes"] == sum(p.stat().st_size for p in (tmp_path / "adapt" / "blob").iterdir())


def test_adaptive_with_steps(tmp_path):
    from fosvos_hip.options import AdaptOptions
    prov = Provider()
    loader, first = sequence()
    adapt = AdaptOptions(steps=2, pos_prob=0.97, neg_distance=12, erode=2, frame_weight=0.5, first_weight=1.0, learning_rate=1e-7)
    before = prov.weights()
    trace = []
    score = experiment_helper.test_adaptive(prov, loader, tmp_path, first, adapt, loader.dataset.annotation, seq_name="blob",
                                            trace=trace)
    assert prov.learning_rates == [1e-7] and len(trace) == 3
    assert torch.equal(trace[0]["last_mask"].cpu()[0], (first["gt"][0] >= 0.5).to(torch.uint8))
    for t, item in enumerate(trace):
        want_l, want_v, want_c = A.adapt_labels(item["logits0"][0, 0].cpu().numpy(), item["last_mask"][0].cpu().numpy(),
                                                adapt.pos_logit, adapt.neg_distance, adapt.erode)
        assert torch.equal(item["label"].cpu()[0, 0], torch.from_numpy(want_l)), t
        assert torch.equal(item["void"].cpu()[0, 0], torch.from_numpy(want_v)), t
        assert score["adapt"]["counts"][t] == want_c.tolist(), t
        print("frame %d: positives %d, negatives %d, void %d" % ((t,) + tuple(want_c)))
        if t + 1 < len(trace):  # (the PNG bytes are stretched to the frame's own range: byte >= 128 is another statement)
            assert torch.equal(trace[t + 1]["last_mask"], (item["logits1"][:, 0] >= 0).to(torch.uint8)), t
    assert score["adapt"]["steps"] == 2 and score["adapt"]["pos_logit"] == adapt.pos_logit
    assert experiment_helper.last_fast["adapt"] == score["adapt"] and score == experiment_helper.last_score
    assert sorted(p.name for p in (tmp_path / "blob").iterdir()) == ["%05d.png" % k for k in range(3)]
    after = prov.weights()
    frozen = [k for k in before if k.startswith("upscale")]
    assert len(frozen) == 8 and all(torch.equal(before[k], after[k]) for k in frozen)
    # what the online optimizer steps (score_dsn is not in it) - but for fuse.bias: Centred takes the median off the fused
    # logits, so they do not depend on it and its gradient is exactly zero
    trained = [k for k in before if k.startswith(TRAINED) and k != "fuse.bias"]
    still = [k for k in trained if torch.equal(before[k], after[k])]
    assert len(trained) > 30 and not still, still


def test_one_accumulation_is_the_weighted_sum_of_two_passes():
    prov = Provider(seed=5)
    net = prov.inner.network  # the bare net: with the median taken off, fuse.bias would have no gradient to compare
    loader, first = sequence(2)
    frames = [mb["image"] for mb in loader]
    x = frames[1].to(DEV)
    first_image, first_gt = first["image"][None].to(DEV), first["gt"][None].to(DEV)
    rng = np.random.default_rng(9)
    label = dev((rng.random((1, 1) + SIZE) < 0.3).astype(np.float32))
    void = dev((rng.random((1, 1) + SIZE) < 0.3).astype(np.uint8))
    weights = torch.tensor([1.0, 0.5], device=DEV)
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce

    def grads():
        got = {k: p.grad.detach().clone() for k, p in prov.inner.network.named_parameters() if p.grad is not None}
        prov.inner.network.zero_grad(set_to_none=True)
        return got

    assert SIZE[0] * SIZE[1] % 4 == 0                                               # the one-pass form
    experiment_helper.adapt_accumulate(net, first_image, first_gt, x, label, void, weights)
    one = grads()
    cbce(net.forward(first_image)[-1], first_gt, size_average=False).backward()
    g_first = grads()
    cbce(net.forward(x)[-1], label, size_average=False, void_pixels=void).backward()
    g_frame = grads()
    trainable = [k for k in one if k.startswith(TRAINED)]
    assert len(trainable) > 30
    for k in trainable:
        want = 1.0 * g_first[k] + 0.5 * g_frame[k]
        err = (one[k] - want).norm().item() / max(want.norm().item(), 1e-30)
        assert err <= GRAD_REL_L2, (k, err)
    # without the first frame: the frame's gradient alone, times its weight
    experiment_helper.adapt_accumulate(net, first_image, first_gt, x, label, void, weights, with_first=False)
    alone = grads()
    for k in trainable:
        err = (alone[k] - 0.5 * g_frame[k]).norm().item() / max(g_frame[k].norm().item() * 0.5, 1e-30)
        assert err <= 1e-5, (k, err)


def test_train_online_adapt_steps_end_to_end(tmp_path, monkeypatch):
    """``train_online.py --synthetic --adapt-steps 1 --score --png-fitted``: the test pass is ``test_adaptive``; a second call
    that does not train takes the first sample from the training loader all the same."""
    import shutil
    import yaml
    import train_online
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    flags = ["--synthetic", "--height", "48", "--width", "84", "-s", "synthetic", "--n-epochs", "5", "--adapt-steps", "1",
             "--adapt-distance", "12", "--adapt-erode", "2", "--score", "--png-fitted"]
    try:
        for extra in ([], ["--no-training"]):
            if extra:  # the reference's naming: training saves epoch n - 1, a test-only call loads epoch n
                saved = tmp_path / "models" / "vgg16" / "online"
                shutil.copy(str(saved / "vgg16_synthetic_epoch-4.pth"), str(saved / "vgg16_synthetic_epoch-5.pth"))
            train_online.main(flags + extra)
            score = train_online.scored_sequences[-1]
            assert score["adapt"]["steps"] == 1 and (score["adapt"]["neg_distance"], score["adapt"]["erode"]) == (12, 2)
            assert len(score["adapt"]["counts"]) == 4 and all(sum(c) == 48 * 84 for c in score["adapt"]["counts"])
            assert experiment_helper.last_fast["png_huffman"] == "fitted"
            out = tmp_path / "results" / "vgg16" / "online" / "synthetic"
            assert sorted(p.name for p in out.glob("*.png")) == ["%05d.png" % k for k in range(4)]
            with open(str(out / "scores.yml")) as fh:
                assert yaml.safe_load(fh)["adapt"]["counts"] == score["adapt"]["counts"]
    finally:
        train_online.adapt, train_online.score, train_online.png_fitted, train_online.synthetic_size = None, False, False, None
