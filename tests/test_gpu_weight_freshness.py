"""Host-side state kept between passes: do the cached weight images follow every weight write?

The op tests compare each kernel with torch on the operands it is GIVEN.  Which operands it is given is decided on the host:
``engine.PackedWeights`` (bf16 MFMA images of 17 conv weights, the score_dsn concatenations, the deconv diagonals and the
head's uniform mask, each keyed by ``(data_ptr, _version)``) and ``resnet_engine.ResnetPlan`` (folded BatchNorm images,
watched per parameter, buffer, module link and BatchNorm eps).  A stale entry leaves every kernel correct and the pass
wrong: part of it reads the fp32 masters live (conv1_1, biases, fuse), the rest last step's images.

Oracle for "fresh": a COLD module - newly constructed, empty caches - loaded with ``state_dict()`` of the warm, mutated
module and run on the same input.  Outputs (and for VGG the gradients of all 52 parameters after one forward + class-balanced
BCE on the five outputs + backward) must be ``torch.equal``.  That is a fair demand because two cold modules with the same
weights agree bit for bit (``test_*_two_cold_modules_agree_bit_for_bit``: the kernels are deterministic, the control passes
for every output and gradient, so no output is compared at a tolerance).  One case per model is also anchored to the CPU
oracle at the tolerances its neighbours use (``test_gpu_network.LOGIT_TOL``, ``test_gpu_resnet._check_net``).

INTEGRATION.md ("Which weight writes the caches see") states the contract these cases pin.
"""
import copy
import os
import pickle
import sys

import pytest
import torch
import torch.nn as nn

from oracle import osvos_ref as O
from oracle import osvos_resnet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from test_gpu_network import LOGIT_TOL, rel_to_max  # noqa: E402  (the VGG anchor's helper and tolerance)
from test_gpu_resnet import _check_net  # noqa: E402  (the ResNet anchor)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# One entry per kind of cache entry: a stage 3x3 weight read by forward and dgrad, conv1_1 (fp32 master read live), a
# side_prep weight, a score_dsn weight and bias (the `small` concatenations), fuse (read live), a bias (read live).
VGG_TARGETS = ("stages.2.1.weight", "stages.0.0.weight", "side_prep.1.weight", "score_dsn.2.weight", "score_dsn.2.bias",
               "fuse.weight", "stages.3.3.bias")
VGG_EARLY = ("stages.4.", "stages.3.")  # what the online loop steps and repacks early
RES_TARGETS = ("layer_stages.2.0.conv1.weight", "layer_base.0.weight", "side_prep.1.weight", "score_dsn.2.weight",
               "score_dsn.2.bias", "layer_fuse.weight", "layer_stages.1.0.downsample.0.weight")
RES_E = 3  # ResNet-18 at scale_down_exponent 3: 8, 16, 32 and 64 channels


# ------------------------------------------------------------------------------------------------ shared, read-only inputs
@pytest.fixture(scope="module")
def vgg_sd():
    return O.make_state_dict(61), O.make_state_dict(62)


@pytest.fixture(scope="module")
def vgg_frame():
    x, gt = O.synthetic_frame(1, 48, 86, seed=161)
    return x.to(DEV), gt.to(DEV)


@pytest.fixture(scope="module")
def res_sd():
    return R.make_state_dict(18, RES_E, seed=71), R.make_state_dict(18, RES_E, seed=72)


@pytest.fixture(scope="module")
def res_frame():
    return (50.0 * torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(171))).to(DEV)


def _param(net, name):
    mod, leaf = name.rsplit(".", 1)
    return getattr(net.get_submodule(mod), leaf)


# ------------------------------------------------------------------------------------------------ VGG plumbing
def _vgg(sd):
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    net.load_state_dict(sd)
    return net.to(DEV)


def _vgg_pass(net, frame):
    """One forward + class-balanced BCE on all five outputs + backward: (five logit maps, gradient per parameter name)."""
    from layers.osvos_layers import class_balanced_cross_entropy_loss as cbce
    x, gt = frame
    net.zero_grad(set_to_none=True)
    outs = net(x)
    sum(cbce(o, gt, size_average=False) for o in outs).backward()
    torch.cuda.synchronize()
    grads = {n: None if p.grad is None else p.grad.detach().clone() for n, p in net.named_parameters()}
    assert len(grads) == 52
    return [o.detach().clone() for o in outs], grads


def _assert_same_pass(got, want, what):
    (outs_a, grads_a), (outs_b, grads_b) = got, want
    for i, (a, b) in enumerate(zip(outs_a, outs_b)):
        assert torch.isfinite(a).all(), f"{what}: output {i} is not finite"
        assert torch.equal(a, b), f"{what}: output {i} differs by {(a - b).abs().max().item():.4g}"
    assert grads_a.keys() == grads_b.keys()
    for n in grads_a:
        a, b = grads_a[n], grads_b[n]
        assert (a is None) == (b is None), f"{what}: gradient of {n} present on one side only"
        if a is not None:
            assert torch.equal(a, b), f"{what}: gradient of {n} differs by {(a - b).abs().max().item():.4g}"


def _vgg_assert_fresh(net, frame, before, what):
    """`net` (warm, mutated) against a cold module with its state_dict; returns the warm module's pass."""
    got = _vgg_pass(net, frame)
    cold = _vgg({k: v.detach().clone() for k, v in net.state_dict().items()})
    want = _vgg_pass(cold, frame)
    _assert_same_pass(got, want, what)
    # a mutation that did nothing cannot pass: the fused map and the side map behind the mutated score_dsn layer both moved
    assert not torch.equal(got[0][4], before[0][4]), f"{what}: the fused output did not change"
    assert not torch.equal(got[0][2], before[0][2]), f"{what}: side output 2 did not change"
    return got


def _rescale_grads(net, share=0.1):
    """Gradients of a pass, rescaled per tensor to `share` of the weight's norm: an optimizer step at lr 1 then moves every
    tensor by 10 % whatever the loss scale - far more than rounding, far from overflow."""
    with torch.no_grad():
        for p in net.parameters():
            if p.grad is not None:
                assert float(p.grad.abs().max()) > 0.0
                p.grad.mul_(share * float(p.norm()) / float(p.grad.norm()))


def _mul_no_grad(net, names):
    with torch.no_grad():
        for n in names:
            _param(net, n).mul_(1.5)


def _copy_no_grad(net, names):
    with torch.no_grad():
        for n in names:
            p = _param(net, n)
            p.copy_(p.detach() * 1.5)


def _mul_detached(net, names):
    for n in names:
        _param(net, n).detach().mul_(1.5)


def _init_normal(net, names):
    torch.manual_seed(7)
    for n in names:
        nn.init.normal_(_param(net, n), 0.0, 0.05)


def _rebind_data(net, names):
    for n in names:
        p = _param(net, n)
        p.data = p.detach() * 1.5


def _rebind_parameter(net, names):
    for n in names:
        mod, leaf = n.rsplit(".", 1)
        setattr(net.get_submodule(mod), leaf, nn.Parameter(_param(net, n).detach() * 1.5))


def _mul_data_in_place(net, names):
    """The write no key can see: in place through `.data` (no version bump, same address)."""
    for n in names:
        _param(net, n).data.mul_(1.5)


def _noop_casts(net, names):
    _mul_no_grad(net, names)
    assert net.float() is net and net.to(DEV) is net


IN_PLACE = {"no_grad_mul": _mul_no_grad, "no_grad_copy": _copy_no_grad, "detach_mul": _mul_detached,
            "init_normal": _init_normal, "rebind_data": _rebind_data, "rebind_parameter": _rebind_parameter,
            "float_and_to_are_no_ops": _noop_casts}


def _aba(net, names):
    """`p.data = a; p.data = b` with no pass between (networks/osvos_vgg.py `_load_from_caffe`): `b` is allocated while the
    warm storage has no owner but a cache, so the allocator may hand `b` the warm address - same key, other contents.
    Returns the names whose address recurred."""
    warm = {n: _param(net, n).data_ptr() for n in names}
    for n in names:
        p = _param(net, n)
        a = p.detach() * 1.5          # allocated while the warm storage is alive
        p.data = a                    # ... which loses its last owner here (unless a cache holds it)
        del a
        b = p.detach().clone()        # allocated while the warm address is free
        p.data = b                    # `a` is released; `p` holds 1.5 x the warm values
        del b
    return [n for n in names if _param(net, n).data_ptr() == warm[n]]


# ------------------------------------------------------------------------------------------------ VGG cases
def test_vgg_two_cold_modules_agree_bit_for_bit(vgg_sd, vgg_frame):
    """The control that makes bit-equality a fair demand: same weights, two newly built modules, same bits - all five outputs
    and all 44 gradients (the 8 frozen upscale filters get none on either side)."""
    a, b = _vgg_pass(_vgg(vgg_sd[0]), vgg_frame), _vgg_pass(_vgg(vgg_sd[0]), vgg_frame)
    _assert_same_pass(a, b, "two cold modules")
    assert sum(g is not None for g in a[1].values()) == 44


def test_vgg_load_state_dict_and_oracle_anchor(vgg_sd, vgg_frame):
    """`load_state_dict` of another seed after a warm pass: fresh, and (the one anchor of this model) the mutated module's
    logits against the fp32 CPU oracle on the NEW weights at test_forward_vs_reference_golden's tolerance."""
    net = _vgg(vgg_sd[0])
    before = _vgg_pass(net, vgg_frame)
    net.load_state_dict(vgg_sd[1])
    got = _vgg_assert_fresh(net, vgg_frame, before, "load_state_dict")
    ref = O.forward(vgg_sd[1], vgg_frame[0].cpu())
    for i, (o, r) in enumerate(zip(got[0], ref)):
        err = rel_to_max(o.cpu(), r)
        assert err < LOGIT_TOL, f"output {i}: {err:.3e} of the logit range"


@pytest.mark.parametrize("mutation", sorted(IN_PLACE))
def test_vgg_weight_write_reaches_the_next_pass(vgg_sd, vgg_frame, mutation):
    net = _vgg(vgg_sd[0])
    before = _vgg_pass(net, vgg_frame)
    IN_PLACE[mutation](net, VGG_TARGETS)
    _vgg_assert_fresh(net, vgg_frame, before, mutation)


@pytest.mark.parametrize("fused", [False, True], ids=["torch_sgd", "fused_sgd"])
def test_vgg_optimizer_step_reaches_the_next_pass(vgg_sd, vgg_frame, fused):
    """A stock `torch.optim.SGD.step()` and a `FusedSGD.step()` (raw-pointer writes + `increment_version` by hand) on the
    gradients of the warm pass - twice, so that images packed AFTER a step are replaced by the next one too."""
    from fosvos_hip.sgd import FusedSGD
    net = _vgg(vgg_sd[0])
    opt = (FusedSGD if fused else torch.optim.SGD)(net.parameters(), lr=1.0, momentum=0.9)
    before = _vgg_pass(net, vgg_frame)
    for step in range(2):
        _rescale_grads(net)
        opt.step()
        before = _vgg_assert_fresh(net, vgg_frame, before, f"step {step}")


def test_vgg_split_step_with_prepack_twice(vgg_sd, vgg_frame):
    """The online loop's order: `step(only=early)`, `prepack_weights(early prefixes)` - which caches images of the early layers
    under their post-step versions - then the rest.  Then the same AGAIN: the second early step must make those images stale."""
    from fosvos_hip.sgd import FusedSGD
    net = _vgg(vgg_sd[0])
    named = list(net.named_parameters())
    early = [p for n, p in named if n.startswith(VGG_EARLY)]
    rest = [p for n, p in named if not n.startswith(VGG_EARLY)]
    assert len(early) == 12 and len(rest) == 40
    opt = FusedSGD(net.parameters(), lr=1.0, momentum=0.9)
    before = _vgg_pass(net, vgg_frame)
    for step in range(2):
        _rescale_grads(net)
        opt.step(only=early, tag="early")
        net.prepack_weights(VGG_EARLY)
        opt.step(only=rest, tag="rest")
        before = _vgg_assert_fresh(net, vgg_frame, before, f"split step {step}")


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_vgg_copies_carry_no_weight_images(vgg_sd, vgg_frame, how):
    """`copy.deepcopy` and a pickle round trip go through `__getstate__/__setstate__`.  The original is written in place
    through `.data` first - a write its own caches cannot see - so the copy is fresh only if it starts without them."""
    net = _vgg(vgg_sd[0])
    before = _vgg_pass(net, vgg_frame)
    _mul_data_in_place(net, VGG_TARGETS)
    twin = copy.deepcopy(net) if how == "deepcopy" else pickle.loads(pickle.dumps(net))
    assert twin._packs is not net._packs and not twin._packs._cache
    _vgg_assert_fresh(twin, vgg_frame, before, how)


def test_vgg_address_recurrence(vgg_sd, vgg_frame):
    """ABA on every 3x3 weight (and one score_dsn weight) at once.  Prints how many of the 18 addresses came back to their
    warm values and asserts freshness whatever the count.  With the caches holding the storage they packed from, only a
    tensor that has no image can recur (conv1_1: its kernel reads the fp32 master).  Before they did, all 18 recurred on the
    MI355X and the pass ran on the warm images."""
    net = _vgg(vgg_sd[0])
    before = _vgg_pass(net, vgg_frame)
    names = [n for n, p in net.named_parameters() if p.dim() == 4 and p.shape[-1] == 3]
    assert len(names) == 17
    recurred = _aba(net, names + ["score_dsn.2.weight"])
    print(f"[vgg ABA] {len(recurred)} of {len(names) + 1} data_ptr()s returned to their warm values: {recurred}")
    _vgg_assert_fresh(net, vgg_frame, before, f"ABA ({len(recurred)} addresses recurred)")


def test_vgg_in_place_data_write_then_invalidate(vgg_sd, vgg_frame):
    """`p.data.mul_()` bumps no version and moves nothing; `invalidate_weight_images()` is the documented way to say so.
    (What a pass computes WITHOUT the call is deliberately not asserted.)  Arenas and the context are left alone."""
    net = _vgg(vgg_sd[0])
    before = _vgg_pass(net, vgg_frame)
    arenas = net._packs.arenas
    _mul_data_in_place(net, VGG_TARGETS)
    net.invalidate_weight_images()
    assert net._packs.arenas is arenas and not net._packs._cache and not net._packs._uniform
    _vgg_assert_fresh(net, vgg_frame, before, ".data.mul_ + invalidate_weight_images")


def test_vgg_head_caches_follow_the_upscale_filters(vgg_sd, vgg_frame):
    """The deconv diagonals and the head's uniform mask: after a warm pass with the bilinear (uniform) filters, per-channel
    different diagonal filters in upscale[2] drop bit 2 of the mask and reach the pass; an off-diagonal entry is still
    refused by the warm module."""
    from fosvos_hip import engine
    net = _vgg(vgg_sd[0])
    before = _vgg_pass(net, vgg_frame)

    def mask():
        return net._packs.head_uniform_mask(dict(zip(engine.PARAM_NAMES, net._ordered_params())))

    assert mask() == 0b1111
    with torch.no_grad():
        net.upscale[2].weight.mul_((1.0 + 0.1 * torch.arange(16, device=DEV)).view(16, 1, 1, 1))
    got = _vgg_pass(net, vgg_frame)
    assert mask() == 0b1011
    cold = _vgg({k: v.detach().clone() for k, v in net.state_dict().items()})
    _assert_same_pass(got, _vgg_pass(cold, vgg_frame), "per-channel upscale[2]")
    assert not torch.equal(got[0][4], before[0][4])
    with torch.no_grad():
        net.upscale[2].weight[0, 1, 0, 0] = 0.5
    with pytest.raises(NotImplementedError, match="off-diagonal"):
        net(vgg_frame[0])


# ------------------------------------------------------------------------------------------------ ResNet plumbing
def _prune(net):
    """What src/prune.py does to one block: three filters of layer_stages[1][0].conv1 removed, the block rebuilt as a
    BasicBlockDummy (as tests/test_gpu_resnet.py::test_pruned_block_with_odd_channel_counts, but usable after a warm pass)."""
    from networks.osvos_resnet import BasicBlockDummy
    blk = net.layer_stages[1][0]
    dev = blk.conv1.weight.device
    keep = torch.tensor([i for i in range(blk.conv1.out_channels) if i not in (3, 7, 12)], device=dev)
    conv1 = nn.Conv2d(blk.conv1.in_channels, len(keep), 3, stride=blk.conv1.stride, padding=1, bias=False).to(dev)
    conv1.weight.data = blk.conv1.weight.data[keep].clone()
    bn1 = nn.BatchNorm2d(len(keep)).to(dev)
    for name in ("weight", "bias", "running_mean", "running_var"):
        getattr(bn1, name).data = getattr(blk.bn1, name).data[keep].clone()
    conv2 = nn.Conv2d(len(keep), blk.conv2.out_channels, 3, padding=1, bias=False).to(dev)
    conv2.weight.data = blk.conv2.weight.data[:, keep].clone()
    net.layer_stages[1][0] = BasicBlockDummy(conv1, bn1, blk.relu, conv2, blk.bn2, blk.downsample, blk.stride)


def _set_eps(net):
    net.layer_stages[2][0].bn1.eps = 0.5
    net.layer_base[1].eps = 0.5


def _res(sd, structure=None):
    from networks.osvos_resnet import OSVOS_RESNET
    net = OSVOS_RESNET(pretrained=False, version=18, scale_down_exponent=RES_E)
    if structure is not None:
        structure(net)  # (what a state_dict does not carry: module classes, channel counts, eps)
    net.load_state_dict(sd)
    return net.to(DEV).eval()


def _res_pass(net, x):
    with torch.no_grad():
        outs = net(x)
    torch.cuda.synchronize()
    assert len(outs) == 5
    return [o.detach().clone() for o in outs]


def _assert_same_outputs(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a).all(), f"{what}: output {i} is not finite"
        assert torch.equal(a, b), f"{what}: output {i} differs by {(a - b).abs().max().item():.4g}"


def _res_assert_fresh(net, x, before, what, structure=None, side=2):
    got = _res_pass(net, x)
    cold = _res({k: v.detach().clone() for k, v in net.state_dict().items()}, structure)
    _assert_same_outputs(got, _res_pass(cold, x), what)
    assert not torch.equal(got[4], before[4]), f"{what}: the fused output did not change"
    if side is not None:
        assert not torch.equal(got[side], before[side]), f"{what}: side output {side} did not change"
    return got


# ------------------------------------------------------------------------------------------------ ResNet cases
def test_resnet_two_cold_modules_agree_bit_for_bit(res_sd, res_frame):
    _assert_same_outputs(_res_pass(_res(res_sd[0]), res_frame), _res_pass(_res(res_sd[0]), res_frame), "two cold modules")


def test_resnet_load_state_dict_and_oracle_anchor(res_sd, res_frame):
    """`load_state_dict` of another seed - weights, BatchNorm affine terms, running_mean and running_var all change - and the
    one anchor of this model: the warm, mutated module through `_check_net` against the fp32 CPU oracle on the new weights."""
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    net.load_state_dict(res_sd[1])
    _res_assert_fresh(net, res_frame, before, "load_state_dict")
    _check_net(net, res_sd[1], res_frame.cpu())


def test_resnet_running_statistics_through_load_state_dict(res_sd, res_frame):
    """Only buffers change: the running statistics of the other seed, every weight as before."""
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    sd = {k: (res_sd[1][k] if k.endswith(("running_mean", "running_var")) else v) for k, v in res_sd[0].items()}
    net.load_state_dict(sd)
    _res_assert_fresh(net, res_frame, before, "running statistics", side=None)


@pytest.mark.parametrize("mutation", sorted(IN_PLACE))
def test_resnet_weight_write_reaches_the_next_pass(res_sd, res_frame, mutation):
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    IN_PLACE[mutation](net, RES_TARGETS)
    _res_assert_fresh(net, res_frame, before, mutation)


@pytest.mark.parametrize("fused", [False, True], ids=["torch_sgd", "fused_sgd"])
def test_resnet_optimizer_step_reaches_the_next_pass(res_sd, res_frame, fused):
    """The path has no backward pass; the gradients are set by hand (0.3 x the weight: a step at lr 1 scales it by 0.7)."""
    from fosvos_hip.sgd import FusedSGD
    net = _res(res_sd[0])
    opt = (FusedSGD if fused else torch.optim.SGD)(net.parameters(), lr=1.0, momentum=0.9)
    before = _res_pass(net, res_frame)
    for step in range(2):
        for n in RES_TARGETS:
            p = _param(net, n)
            p.grad = 0.3 * p.detach()
        opt.step()
        before = _res_assert_fresh(net, res_frame, before, f"step {step}")


def test_resnet_batchnorm_weight(res_sd, res_frame):
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    with torch.no_grad():
        net.layer_stages[2][0].bn1.weight.mul_(1.5)
        net.layer_base[1].weight.mul_(1.5)
    _res_assert_fresh(net, res_frame, before, "BatchNorm weight", side=None)


def test_resnet_batchnorm_eps(res_sd, res_frame):
    """`eps` is folded into the images but is an attribute, not a tensor: the plan compares it by value."""
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    _set_eps(net)
    _res_assert_fresh(net, res_frame, before, "BatchNorm eps", structure=_set_eps, side=None)


def test_resnet_pruned_block_swapped_in_after_the_warm_pass(res_sd, res_frame):
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    _prune(net)
    assert net.state_dict()["layer_stages.1.0.conv1.weight"].shape[0] == 13
    _res_assert_fresh(net, res_frame, before, "BasicBlockDummy", structure=_prune, side=None)


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_resnet_copies_carry_no_weight_images(res_sd, res_frame, how):
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    _mul_data_in_place(net, RES_TARGETS)
    twin = copy.deepcopy(net) if how == "deepcopy" else pickle.loads(pickle.dumps(net))
    assert twin._plan is not net._plan and twin._plan.signature is None
    _res_assert_fresh(twin, res_frame, before, how)


def test_resnet_address_recurrence(res_sd, res_frame):
    """ABA on every 3x3 weight of the net at once (`ResnetPlan` keeps the parameter object alive, which does not keep the
    storage `p.data = ...` drops).  Prints the recurrence count, asserts freshness whatever it is.  (Before the plan held the
    storages, two runs on the MI355X: 21 of 21 addresses recurred and the pass ran on the warm images; 20 of 21 recurred and
    the pass was fresh only because the plan rebuilds every image when ONE watched tensor moved.)"""
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    names = [n for n, p in net.named_parameters() if p.dim() == 4 and p.shape[-1] == 3]
    assert len(names) == 20  # 16 block convs + 4 side_prep
    recurred = _aba(net, names + ["score_dsn.2.weight"])
    print(f"[resnet ABA] {len(recurred)} of {len(names) + 1} data_ptr()s returned to their warm values: {recurred}")
    _res_assert_fresh(net, res_frame, before, f"ABA ({len(recurred)} addresses recurred)")


def test_resnet_in_place_data_write_then_invalidate(res_sd, res_frame):
    net = _res(res_sd[0])
    before = _res_pass(net, res_frame)
    arena = net._plan.arena
    _mul_data_in_place(net, RES_TARGETS)
    net.invalidate_weight_images()
    assert net._plan.signature is None and net._plan.arena is arena
    _res_assert_fresh(net, res_frame, before, ".data.mul_ + invalidate_weight_images")
