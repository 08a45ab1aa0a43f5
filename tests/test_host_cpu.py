"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol the header declares,
the drop-in module surface (state_dict, optimizer recipe, flags), and loud failure without a GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from oracle import osvos_ref as O  # noqa: E402


def test_library_exports_every_header_symbol():
    import fosvos_hip
    header = open(fosvos_hip.HEADER_PATH).read()
    declared = set(re.findall(r"\b(fosvos_[a-z0-9_]+)\s*\(", header))
    declared -= {"fosvos_sgd_entry"}
    assert declared == set(fosvos_hip.SIGNATURES), (declared ^ set(fosvos_hip.SIGNATURES))
    lib = fosvos_hip.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.fosvos_abi_version() == fosvos_hip.ABI_VERSION
    assert lib.fosvos_build_arch() == b"gfx950"
    # pure host-side queries (no GPU needed)
    assert lib.fosvos_packed_weight_elems(64, 64) == 64 * 64 * 9
    assert lib.fosvos_packed_weight_elems(16, 40) == 16 * 64 * 9     # contraction side padded to 32
    assert lib.fosvos_conv3x3_wgrad_workspace_bytes(1, 480, 854, 64, 64) > 0
    assert lib.fosvos_conv3x3_workspace_bytes(1, 480, 854, 64, 64) == 0      # enough pixel tiles: no split-K
    assert lib.fosvos_conv3x3_workspace_bytes(1, 30, 54, 512, 512) > 0       # stage 5: split-K slabs
    assert lib.fosvos_head_bwd_workspace_bytes(1, 480, 854) > 0
    assert lib.fosvos_cbce_workspace_bytes(480 * 854) > 0
    assert lib.fosvos_ctx_device(None) == -1


def _plan(n, h, w, ci, co):
    import ctypes
    import fosvos_hip
    info = fosvos_hip.Conv3x3PlanInfo()
    fosvos_hip.check(fosvos_hip.lib().fosvos_conv3x3_plan(n, h, w, ci, co, ctypes.byref(info)), "conv3x3_plan")
    return (info.tile_h, info.tile_w, info.tile_co, info.k_splits, info.workgroups)


def test_conv_plan_of_the_480p_step():
    """Which igemm instantiation each layer of the 854x480 step gets (host arithmetic of fosvos_conv3x3_plan): the GPU op
    tests assert the same query for their cases, so this table is what ties them to the benchmarked configuration."""
    # (N, H, W, Ci, Co) -> tile: stages 1-3 of one frame and every stage-1-4 layer of a five-frame pass run 256-pixel tiles
    assert _plan(1, 480, 854, 64, 64)[:4] == (8, 32, 64, 1)
    assert _plan(1, 240, 427, 64, 128)[:4] == (16, 16, 64, 1)
    assert _plan(1, 240, 427, 128, 128)[:4] == (16, 16, 64, 1)
    assert _plan(5, 120, 214, 128, 256)[:4] == (8, 32, 64, 1)
    assert _plan(5, 60, 107, 512, 512)[:4] == (16, 16, 64, 1)
    assert _plan(5, 30, 54, 512, 512)[:4] == (8, 32, 64, 1)        # stage 5 of five frames: 320 workgroups of 256 pixels
    assert _plan(3, 30, 54, 512, 512)[:4] == (8, 16, 64, 1)        # ... of a three-frame forward chain: 384 128-pixel tiles
    assert _plan(1, 120, 214, 64, 64)[:3] == (8, 16, 64)           # 105 blocks of 256 px: the 128-pixel tile
    assert _plan(1, 30, 54, 512, 512)[3] > 1                       # stage 5 of one frame: split-K
    assert _plan(1, 240, 427, 128, 16)[:3] == (8, 32, 16)          # side_prep at large maps
    import ctypes
    import fosvos_hip
    tiles, wgs = ctypes.c_int(), ctypes.c_int()
    fosvos_hip.check(fosvos_hip.lib().fosvos_conv3x3_first_plan(1, 480, 854, ctypes.byref(tiles), ctypes.byref(wgs)), "plan")
    assert (tiles.value, wgs.value) == (60 * 27, 1024)             # the persistent conv1_1 loop iterates at 480x854


@pytest.mark.parametrize("h,w", [(480, 854), (384, 683), (240, 427), (33, 47), (1, 1)])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
def test_vgg_arena_layout(n, h, w):
    """fosvos_vgg_arena_layout (what the layer-parity tests read the native pass back through): every tensor region and
    workspace is 256-byte aligned, inside fosvos_vgg_arena_bytes, disjoint from every other, and as large as its layout;
    the stage resolutions are the ceil-halvings of the frame."""
    import fosvos_hip
    from fosvos_hip import ops
    L = ops.vgg_arena_layout(n, h, w)
    assert L["total"] == fosvos_hip.lib().fosvos_vgg_arena_bytes(n, h, w) > 0
    sh, sw = [h], [w]
    for _ in range(4):
        sh.append((sh[-1] + 1) // 2)
        sw.append((sw[-1] + 1) // 2)
    assert L["stage_h"] == sh and L["stage_w"] == sw
    stage_of = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
    cout = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
    px = [n * sh[s] * sw[s] for s in range(5)]
    regions = []  # (name, offset, bytes)
    for c in range(13):
        want = px[stage_of[c]] * cout[c] * 2
        assert L["act_bytes"][c] == want, c
        regions += [(f"act{c}", L["act"][c], want), (f"gact{c}", L["gact"][c], want)]
        regions.append((f"wsa_conv{c}", L["wsa_conv"][c], L["wsa_conv_bytes"][c]))
    for i in range(4):
        s = i + 1
        assert L["pooled_bytes"][i] == px[s] * (64, 128, 256, 512)[i] * 2
        assert L["side_bytes"][i] == px[s] * 16 * 4 and L["dside_bytes"][i] == px[s] * 32 * 2
        regions += [(f"pooled{i}", L["pooled"][i], L["pooled_bytes"][i]), (f"gpooled{i}", L["gpooled"][i], L["pooled_bytes"][i]),
                    (f"side{i}", L["side"][i], L["side_bytes"][i]), (f"dside{i}", L["dside"][i], L["dside_bytes"][i]),
                    (f"wsa_side{i}", L["wsa_side"][i], L["wsa_side_bytes"][i])]
    assert L["bits0_bytes"] == px[0] * 8
    regions += [("bits0", L["bits0"], L["bits0_bytes"]), ("ws", L["ws"], L["ws_bytes"]), ("hws", L["hws"], L["hws_bytes"])]
    assert L["ws_bytes"] > 0 and L["hws_bytes"] > 0
    regions.sort(key=lambda r: r[1])
    for name, off, nb in regions:
        assert off % 256 == 0, name
        assert off + nb <= L["total"], name
    for (a, oa, na), (b, ob, _) in zip(regions, regions[1:]):
        assert oa + na <= ob, f"{a} [{oa}, {oa + na}) overlaps {b} at {ob}"


def test_module_surface_matches_reference_contract():
    from networks.osvos_vgg import OSVOS_VGG
    from fosvos_hip import engine
    net = OSVOS_VGG(pretrained=0)
    spec = O.state_dict_spec()
    assert list(net.state_dict().keys()) == list(spec.keys()) == engine.PARAM_NAMES
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == spec[k], k
    # the reference's initialisation: N(0, 1e-3) convs, zero biases, diagonal bilinear deconvs
    assert abs(net.stages[2][1].weight.std().item() - 1e-3) < 5e-5
    assert net.stages[2][1].bias.abs().max().item() == 0
    for i in range(4):
        assert torch.equal(net.upscale[i].weight.data, O.bilinear_deconv_weight(16, 4 << i))
        assert torch.equal(net.upscale_[i].weight.data, O.bilinear_deconv_weight(1, 4 << i))
    # module indices inside the stages (pool first in stages 1..4)
    assert isinstance(net.stages[0][0], torch.nn.Conv2d) and isinstance(net.stages[1][0], torch.nn.MaxPool2d)
    assert net.stages[1][0].ceil_mode
    # whole-module pickles keep working and carry no device caches
    import pickle
    clone = pickle.loads(pickle.dumps(net))
    assert list(clone.state_dict().keys()) == list(spec.keys())
    # ... also after a training loop attached its flat gradient buffer (and possibly pending collectives) to the module
    import parallel
    named = list(net.named_parameters())
    flat = parallel.FlatGrads.attach(net, [p for _, p in named], names=[n for n, _ in named])
    flat._works.append(object())
    assert net._fosvos_flat_grads is flat
    clone = pickle.loads(pickle.dumps(net))
    assert not hasattr(clone, "_fosvos_flat_grads") and all(p.grad is None for p in clone.parameters())
    assert list(clone.state_dict().keys()) == list(spec.keys())


def test_no_cpu_fallback():
    from networks.osvos_vgg import OSVOS_VGG
    from layers.osvos_layers import class_balanced_cross_entropy_loss
    net = OSVOS_VGG(pretrained=0)
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="GPU"):
        class_balanced_cross_entropy_loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_optimizer_recipe_matches_reference(golden):
    from networks.osvos_vgg import OSVOS_VGG
    from util.network_provider import VGGOfflineProvider, VGGOnlineProvider
    k = golden("loops.npz")
    for mode, cls in (("online", VGGOnlineProvider), ("offline", VGGOfflineProvider)):
        prov = cls.__new__(cls)
        prov.network = OSVOS_VGG(pretrained=0)
        opt = prov.get_optimizer()
        assert isinstance(opt, torch.optim.SGD)
        names = {id(p): n for n, p in prov.network.named_parameters()}
        rows = [f"{gi}|{names[id(p)]}|{grp['lr']!r}|{grp['weight_decay']!r}|{grp['momentum']!r}"
                for gi, grp in enumerate(opt.param_groups) for p in grp["params"]]
        assert rows == [str(s) for s in k[f"groups_{mode}"]]


def test_layer_helpers_match_reference(golden):
    from layers import osvos_layers as L
    import numpy as np
    k = golden("kat.npz")
    for size in (3, 4, 5, 8, 16, 32):
        np.testing.assert_array_equal(L.upsample_filt(size), k[f"filt_{size}"])
    src = torch.from_numpy(k["crop_src"])
    for h, w in k["crop_cases"]:
        np.testing.assert_array_equal(L.center_crop(src, int(h), int(w)).numpy(), k[f"crop_{h}_{w}"])
    for c, size in ((16, 4), (1, 8), (3, 16)):
        lay = torch.nn.ConvTranspose2d(c, c, size, stride=size // 2, bias=False)
        np.testing.assert_array_equal(L.interp_surgery(lay).numpy(), k[f"surgery_{c}_{size}"])


def test_cli_flags():
    from util import args_helper
    a = args_helper.parse_args(True, ["--gpu-id", "0", "-s", "blackswan", "-sg", "1", "-sgs", "4", "--variant-online", "2",
                                      "--no-testing", "--eval-speeds"])
    assert (a.gpu_id, a.sequence_name, a.sequence_group, a.sequence_group_size, a.variant_online) == (0, "blackswan", 1, 4, 2)
    assert a.is_training and not a.is_testing and a.eval_speeds and a.network == "vgg16"
    b = args_helper.parse_args(False, [])
    assert not hasattr(b, "sequence_name") and b.variant_offline is None


def test_sequence_sharding_matches_reference_rule():
    import parallel
    import train_online
    seqs = train_online.sequences_val
    assert len(seqs) == 20
    parts = [parallel.shard_sequences(seqs, g, 8) for g in range(8)]
    assert sorted(sum(parts, [])) == sorted(seqs)
    assert parts[3] == [s for i, s in enumerate(seqs) if i % 8 == 3]  # src/train_online.py:184-186
    assert parallel.shard_sequences(seqs, None, None) == seqs
    assert parallel.split_accumulation(8, 8) == 1 and parallel.split_accumulation(10, 2) == 5
    with pytest.raises(ValueError):
        parallel.split_accumulation(5, 8)


def test_png_bytescale_known_answers():
    """scipy.misc.imsave's scaling (what src/util/experiment_helper.py:64 relied on): stretch to the map's own range,
    round half up; a constant map becomes zeros."""
    from util.experiment_helper import bytescale
    assert bytescale(np.array([[0.2, 0.7], [0.45, 0.2]])).tolist() == [[0, 255], [128, 0]]
    assert bytescale(np.full((2, 3), 0.37)).tolist() == [[0, 0, 0], [0, 0, 0]]
    assert bytescale(np.array([[0.0, 1.0, 0.5, 0.25]])).tolist() == [[0, 255, 128, 64]]


# every switch: (options class, field, environment variable, a value that selects the non-default)
_SWITCHES = [("LoopOptions", "microbatch_group", "FOSVOS_MICROBATCH_GROUP", "3"),
             ("LoopOptions", "group_window", "FOSVOS_GROUP_WINDOW", "7"),
             ("LoopOptions", "defer_join", "FOSVOS_DEFER_JOIN", "0"),
             ("LoopOptions", "split_step", "FOSVOS_SPLIT_STEP", "0"),
             ("LoopOptions", "stage_loss", "FOSVOS_STAGE_LOSS", "0"),
             ("LoopOptions", "grad_overwrite", "FOSVOS_GRAD_OVERWRITE", "0"),
             ("LoopOptions", "pass_streams", "FOSVOS_PASS_STREAMS", "0"),
             ("LoopOptions", "comm_timing", "FOSVOS_COMM_TIMING", "1"),
             ("EngineOptions", "two_streams", "FOSVOS_TWO_STREAMS", "0"),
             ("EngineOptions", "fwd_aux", "FOSVOS_FWD_AUX", "0"),
             ("EngineOptions", "head_uniform", "FOSVOS_HEAD_UNIFORM", "0"),
             ("EngineOptions", "stream_probe", "FOSVOS_STREAM_PROBE", "0"),
             ("EngineOptions", "resnet_mfma", "FOSVOS_RESNET_MFMA", "0"),
             ("EngineOptions", "resnet_fuse_first", "FOSVOS_RESNET_FUSE_FIRST", "0"),
             ("EngineOptions", "resnet_aux", "FOSVOS_RESNET_AUX", "1")]


def test_options_from_an_empty_environment_are_the_defaults():
    import dataclasses
    from fosvos_hip import options
    assert options.LoopOptions.from_env({}) == options.LoopOptions()
    assert options.EngineOptions.from_env({}) == options.EngineOptions()
    assert options.LoopOptions() == options.LoopOptions(
        microbatch_group=5, group_window=16, defer_join=True, split_step=True, stage_loss=True, grad_overwrite=True,
        pass_streams=True, comm_timing=False)
    assert options.EngineOptions() == options.EngineOptions(
        two_streams=True, fwd_aux=True, head_uniform=True, stream_probe=True, resnet_mfma=True, resnet_fuse_first=True,
        resnet_aux=False)
    assert options.native_loop_from_env({}) and not options.native_loop_from_env({"FOSVOS_PY_ENGINE": "1"})
    # the table above covers every field of both classes
    for cls in (options.LoopOptions, options.EngineOptions):
        assert {f.name for f in dataclasses.fields(cls)} == {s[1] for s in _SWITCHES if s[0] == cls.__name__}


@pytest.mark.parametrize("cls_name,field,var,value", _SWITCHES)
def test_each_variable_changes_exactly_its_own_field(cls_name, field, var, value):
    import dataclasses
    from fosvos_hip import options
    for name in ("LoopOptions", "EngineOptions"):
        cls = getattr(options, name)
        got, default = cls.from_env({var: value}), cls()
        for f in dataclasses.fields(cls):
            if name == cls_name and f.name == field:
                assert getattr(got, f.name) != getattr(default, f.name), f.name
                if f.type == "int":
                    assert getattr(got, f.name) == int(value)
            else:
                assert getattr(got, f.name) == getattr(default, f.name), f.name
    with pytest.raises(dataclasses.FrozenInstanceError):
        setattr(getattr(options, cls_name)(), field, None)


@pytest.mark.parametrize("value,group,window", [("", 5, 16), ("five", 5, 16), ("2.5", 5, 16), ("0", 1, 1), ("-3", 1, 1),
                                                ("4", 4, 4)])
def test_malformed_and_non_positive_counts_fall_back(value, group, window):
    from fosvos_hip.options import LoopOptions
    got = LoopOptions.from_env({"FOSVOS_MICROBATCH_GROUP": value, "FOSVOS_GROUP_WINDOW": value})
    assert (got.microbatch_group, got.group_window) == (group, window)


def test_pass_flags_are_declared():
    """A misspelt flag raises; the module's attributes of the same names are the flags."""
    import dataclasses
    from fosvos_hip.engine import PackedWeights, PassFlags
    from networks.osvos_vgg import OSVOS_VGG
    flags = PassFlags()
    assert [f.name for f in dataclasses.fields(flags)] == ["defer_wgrad_join", "forward_one_stream", "publish_grad_buckets",
                                                          "overwrite_grads", "last_pass_of_cycle", "compact_stage1"]
    assert not any(getattr(flags, f.name) for f in dataclasses.fields(flags))
    with pytest.raises(AttributeError):
        flags.no_such_flag = True
    with pytest.raises(AttributeError):
        flags.no_such_flag
    assert isinstance(PackedWeights().flags, PassFlags)
    net = OSVOS_VGG(pretrained=0)
    assert net.pass_flags is net._packs.flags and net.options is net._packs.options
    for f in dataclasses.fields(PassFlags):
        assert getattr(net, f.name) is False
        setattr(net, f.name, 1)
        assert getattr(net.pass_flags, f.name) is True and getattr(net, f.name) is True
        setattr(net, f.name, False)
        assert getattr(net.pass_flags, f.name) is False
    net.options = dataclasses.replace(net.options, head_uniform=False)
    assert net._packs.options.head_uniform is False


class _ScalarLog:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append((tag, value, step))


def test_loss_log_keeps_iteration_order():
    """`train_online._LossLog` on CPU tensors: the passes of a window arrive bucket by bucket (out of iteration order), the
    log - `loss_tr` and the add_scalar calls - follows the reference's iteration order (src/train_online.py:84-90): the
    running sum of the losses over the iterations since the last logging point, divided by n_samples, at every iteration of a
    logging epoch."""
    import train_online
    n_samples, log_every, n_epochs = 3, 2, 4
    g = torch.Generator().manual_seed(11)
    loss = {(ep, mb): torch.rand((), generator=g) for ep in range(n_epochs) for mb in range(n_samples)}
    writer = _ScalarLog()
    log = train_online._LossLog(None, n_samples, log_every, "seq", writer)
    its = sorted(loss)
    for lo in range(0, len(its), 5):                 # windows of five iterations (they cross epoch ends)
        window = its[lo:lo + 5]
        passes = [window[0::2][::-1], window[1::2]]  # two passes per window: iterations 4 2 0, then 1 3
        for group in passes:
            log.record([(ep, mb, None, False) for ep, mb in group], torch.stack([loss[key] for key in group]))
        assert log.window
        log.close_window()
        assert not log.window
    log.flush(True)
    assert not log.pending
    # the plain loop
    want, running = [], 0.0
    for ep in range(n_epochs):
        for mb in range(n_samples):
            running += float(loss[(ep, mb)])
            if ep % log_every == log_every - 1:
                want.append((running / n_samples, ep))
                running = 0.0
    assert len(want) == 6 and log.loss_tr == [v for v, _ in want]
    assert writer.calls == [("data/total_loss_epoch", v, ep) for v, ep in want]


def test_which_weight_writes_torch_counts():
    """The torch behaviour the weight-image caches rest on ("Which weight writes the caches see"): they key
    every image by `(data_ptr(), _version)` of its fp32 master.  Row 1 of the table there: these writes bump the version and
    keep the address.  Row 2: in-place writes through `.data` or a numpy alias do neither - nothing can see them, the caller
    says so (`increment_version` / `invalidate_weight_images()`).  Row 3: `p.data = t` moves the address without a bump.  A
    torch upgrade that changes a row fails here, on the CPU, instead of as stale weights on the GPU."""
    import torch.nn as nn
    m = nn.Conv2d(4, 4, 3)
    p = m.weight

    def probe(write):
        version, address = p._version, p.data_ptr()
        write()
        return p._version - version, p.data_ptr() == address

    def no_grad_mul():
        with torch.no_grad():
            p.mul_(1.5)

    def no_grad_copy():
        with torch.no_grad():
            p.copy_(torch.ones_like(p))

    def sgd_step():
        opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
        p.grad, m.bias.grad = torch.ones_like(p), torch.ones_like(m.bias)
        opt.step()

    def numpy_alias():
        p.detach().numpy()[...] = 3.0

    seen = {"no_grad mul_": no_grad_mul, "no_grad copy_": no_grad_copy, "detach().add_": lambda: p.detach().add_(1.0),
            "nn.init.normal_": lambda: nn.init.normal_(p, 0.0, 0.1), "nn.init.constant_": lambda: nn.init.constant_(p, 0.5),
            "load_state_dict": lambda: m.load_state_dict({k: v * 2 for k, v in m.state_dict().items()}),
            "optim.SGD.step": sgd_step, "increment_version": lambda: torch.autograd.graph.increment_version(p)}
    for name, write in seen.items():
        bumps, same_address = probe(write)
        assert bumps >= 1 and same_address, (name, bumps, same_address)
    unseen = {".data.mul_": lambda: p.data.mul_(2.0), ".data.copy_": lambda: p.data.copy_(torch.ones_like(p)),
              "numpy alias": numpy_alias}
    for name, write in unseen.items():
        before = p.detach().clone()
        bumps, same_address = probe(write)
        assert not torch.equal(p.detach(), before), name                # the write did land ...
        assert bumps == 0 and same_address, (name, bumps, same_address)  # ... and left no trace
    keep = p.data  # (the old storage stays allocated, so the new one cannot take its address)
    bumps, same_address = probe(lambda: setattr(p, "data", torch.zeros_like(p)))
    assert bumps == 0 and not same_address and keep.data_ptr() != p.data_ptr()


def test_invalidate_weight_images_is_part_of_both_modules():
    """The public way to say "my weights changed behind torch's back": drops the images, keeps arenas and options; a module
    that comes out of a pickle starts without images."""
    import pickle
    from networks.osvos_resnet import OSVOS_RESNET
    from networks.osvos_vgg import OSVOS_VGG
    net = OSVOS_VGG(pretrained=0)
    packs, arenas, options = net._packs, net._packs.arenas, net.options
    w = net.stages[1][1].weight
    packs._cache["probe"] = ((w.data_ptr(), w._version), None, w.untyped_storage())
    packs._uniform["upscale.0.weight"] = True
    net.invalidate_weight_images()
    assert net._packs is packs and packs.arenas is arenas and net.options is options
    assert not packs._cache and not packs._uniform
    assert not pickle.loads(pickle.dumps(net))._packs._cache
    res = OSVOS_RESNET(pretrained=False, scale_down_exponent=3)
    plan, options = res._plan, res.options
    plan.signature = ("stale",)
    res.invalidate_weight_images()
    assert res._plan is plan and plan.signature is None and res.options is options
    assert pickle.loads(pickle.dumps(res))._plan.signature is None


def test_deconv_diagonal_check_counts_instead_of_summing():
    """`PackedWeights.deconv_diag` refuses a transposed-conv weight with cross-channel entries.  The check must be exact: as a
    difference of two fp32 sums taken in different orders it came out nonzero for a purely diagonal weight whose values are
    no dyadic fractions (per-channel scaled bilinear filters: -1.2e-4), and such a weight was refused."""
    from fosvos_hip import engine
    packs = engine.PackedWeights()
    w = O.bilinear_deconv_weight(16, 16) * (1.0 + 0.1 * torch.arange(16.0)).view(16, 1, 1, 1)
    diag = packs.deconv_diag("upscale.2.weight", w)
    assert tuple(diag.shape) == (16, 16, 16) and packs._uniform["upscale.2.weight"] is False
    assert torch.equal(diag[:, :, 5], w[5, 5])
    packs.deconv_diag("upscale.1.weight", O.bilinear_deconv_weight(16, 8))
    assert packs._uniform["upscale.1.weight"] is True
    w2 = w.clone()
    w2[0, 1, 0, 0] = 1e-30  # far below the rounding of any sum
    with pytest.raises(NotImplementedError, match="off-diagonal"):
        packs.deconv_diag("upscale.2.weight", w2)
