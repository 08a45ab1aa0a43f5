"""Every cross-stream dependency on a real MI355X, by delaying one stream at a time (tests/stream_delays.py states the method;
DESIGN.md section 4.3 lists the scenarios and the edges each covers).  Every leg is compared with the undelayed leg of the same
configuration, run in the same process, by EXACT equality; nothing here has a tolerance and nothing asserts a time.  Both
legs end with a device synchronisation before anything they allocated is released.  Run with ``-s`` for the calibration, L and
t_cycle of every scenario and the sighted / blind pairs."""
import copy
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "fosvos_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stream_delays as D  # noqa: E402
from oracle import osvos_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-8


def _say(msg):
    print("stream_delays: " + msg, flush=True)


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


# ---------------------------------------------------------------------------------------------- streams and pairs
def _loop_streams():
    """role -> stream of the loops: the caller's (the current one) and the library's three (engine.shared_stream)."""
    from fosvos_hip import engine
    engine.shared_stream(0, "comm")  # (creates "aux" and "pass" in front of it, in the fixed order)
    roles = {"caller": torch.cuda.current_stream(torch.device(DEV))}
    for r in ("aux", "pass", "comm"):
        roles[r] = engine.shared_stream(0, r)
    return roles


_PAIRS = {}


def _probe_says(a, b):
    """What the engine's own probe found for two of caller / aux / pass: (overlap or None, figures)."""
    from fosvos_hip import engine
    order = ("caller", "aux", "pass")
    if a not in order or b not in order:
        return None, "never probed by the engine"
    late, early = (a, b) if order.index(a) > order.index(b) else (b, a)
    rec = engine.STREAM_PROBE.get((0, late), {})
    return rec.get("overlaps_with", {}).get(early), "engine probe %s/%s ms [alone, pair] = %s after %s tries" % (
        late, early, rec.get("ms", {}).get(early), rec.get("tries"))


def _loop_pair(delayed, other, streams):
    """True where a missing wait of ``other`` on ``delayed`` can show.  A blind pair is never passed silently: caller/aux and
    caller/pass (and aux/pass) must be sighted whenever the engine's probe says they overlap - a contradiction fails -, and a
    pair the probe found serialised, or a pair with ``comm`` (which the engine never probes), skips with the figures."""
    key = (delayed, other)
    if key not in _PAIRS:
        ok = D.sighted(streams[delayed], streams[other])
        assert D.ordered(streams[delayed], streams[other]), "%s waits for %s and still reads zeros" % (other, delayed)
        _PAIRS[key] = ok
        _say("pair delayed=%s other=%s: %s" % (delayed, other, "sighted" if ok else "BLIND"))
    if _PAIRS[key]:
        return True
    overlap, figures = _probe_says(delayed, other)
    if overlap:
        pytest.fail("pair %s/%s is blind although the engine's probe says the two overlap (%s)" % (delayed, other, figures))
    pytest.skip("blind pair %s/%s: a sleep on one holds the other back (%s)" % (delayed, other, figures))


def _others(role, used):
    return [r for r in used if r != role]


def _sighted_instance(make, pairs_of, what):
    """An object with streams of its own (a segmenter, a loader) whose pairs are all sighted: up to four tries with freshly
    created streams, the earlier objects kept alive so that the round-robin over the hardware queues moves on."""
    kept, blind = [], []
    for attempt in range(4):
        obj = make()
        kept.append(obj)
        blind = []
        for name, a, b in pairs_of(obj):
            assert D.ordered(a, b), "%s: %s with a wait still reads zeros" % (what, name)
            if not D.sighted(a, b):
                blind.append(name)
        if not blind:
            if attempt:
                _say("%s: sighted at try %d" % (what, attempt + 1))
            return obj, kept
        _say("%s: try %d, blind pair(s) %s" % (what, attempt + 1, blind))
    pytest.skip("%s: pair(s) %s stay blind after 4 tries with fresh streams (two streams on one hardware queue)" % (what, blind))


def test_the_detector_on_two_fresh_streams():
    """``sighted`` and its with-wait counterpart on two fresh streams: without a wait the clone is all zeros (the reader ran
    ahead of the sleeping writer), with ``wait_stream`` all ones.  The spin is at least as long as asked for."""
    cal = D.calibration(DEV)
    assert D.calibrate(DEV) == cal.cycles_per_ms > 0
    for ms in (2.0, 7.5):
        assert cal.measured(ms) >= ms
        _say("a spin asked for %.1f ms measured %.3f ms (%d cycles)" % (ms, cal.measured(ms), cal.cycles_for(ms)))
    kept = []

    def make():
        pair = (torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV))
        kept.append(pair)
        return pair

    (a, b), _ = _sighted_instance(make, lambda p: [("a->b", p[0], p[1]), ("b->a", p[1], p[0])], "two fresh streams")
    assert D.sighted(a, b) and D.ordered(a, b) and D.sighted(b, a) and D.ordered(b, a)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the training loops
_TEMPLATES = {}


def _fresh_net(seed=29):
    """make_net of tests/test_gpu_network.py (OSVOS_VGG(pretrained=0) with O.make_state_dict(seed, 'kaiming')), built once on
    the host and copied per leg."""
    if seed not in _TEMPLATES:
        from networks.osvos_vgg import OSVOS_VGG
        net = OSVOS_VGG(pretrained=0)
        sd = O.make_state_dict(seed, "kaiming")
        net.load_state_dict(sd)
        _TEMPLATES[seed] = (net, sd)
    net, sd = _TEMPLATES[seed]
    return copy.deepcopy(net).to(DEV), sd


def _provider(kind, net):
    from util.network_provider import VGGOfflineProvider, VGGOnlineProvider
    cls = VGGOnlineProvider if kind == "online" else VGGOfflineProvider
    prov = cls.__new__(cls)
    prov.network = net
    prov.name = "vgg16"
    return prov


_FRAMES = {}


def _loader(sizes, steps, seed0):
    """``steps`` cycles of frames of ``sizes``, every iteration a frame of its own seed: a stale buffer holds another frame."""
    key = (tuple(sizes), steps, seed0)
    if key not in _FRAMES:
        frames = [O.synthetic_frame(1, h, w, seed=seed0 + i) for i, (h, w) in enumerate(list(sizes) * steps)]
        _FRAMES[key] = [{"image": x, "gt": gt} for x, gt in frames]
    return _FRAMES[key]


def _state(net, opt, ret_losses):
    """What a leg is compared by: the 52 parameters, every momentum buffer, every p.grad at return, the losses."""
    out = {"loss": ret_losses}
    for n, p in net.named_parameters():
        out["w/" + n] = p.detach().clone()
        if p.grad is not None:
            out["g/" + n] = p.grad.detach().clone()
        buf = opt.state.get(p, {}).get("momentum_buffer")
        if buf is not None:
            out["m/" + n] = buf.detach().clone()
    torch.cuda.synchronize()
    return out


def _differences(a, b):
    assert sorted(a) == sorted(b)
    return ["loss"] * int(a["loss"] != b["loss"]) + [k for k in a if k != "loss" and not torch.equal(a[k], b[k])]


def _online_leg(cfg, split, injector_of, mutate=None):
    import train_online
    from fosvos_hip.options import LoopOptions
    sizes, avg, fields = D.ONLINE_CONFIGS[cfg]
    loader = _loader(sizes, 3, 260)
    net, _ = _fresh_net()
    prov = _provider("online", net)
    opt = prov.get_optimizer(learning_rate=LR)
    train_online.data_parallel = False
    inj = injector_of(net, opt)
    with inj:
        if mutate is not None:
            mutate(net)   # (inside the context: the injector's exit removes it with its own wrapper)
        ret, inj.ms = D.timed(lambda: train_online._train(prov, loader, opt, _NullWriter(), cfg, 0, 1, avg, 10 ** 9,
                                                          options=LoopOptions(split_step=split, **fields)), DEV, 1)
    assert ret["iterations"] == 3 * avg
    return _state(net, opt, ret["loss"]), inj


def _offline_leg(group, injector_of):
    import train_offline
    from fosvos_hip.options import LoopOptions
    sizes = [(40, 70), (40, 70), (32, 56), (40, 70), (32, 56)]
    loader = _loader(sizes, 2, 700)
    net, _ = _fresh_net()
    prov = _provider("offline", net)
    opt = prov.get_optimizer(learning_rate=LR)
    train_offline.data_parallel = False
    inj = injector_of(net, opt)
    with inj:
        ret, inj.ms = D.timed(lambda: train_offline._train(prov, loader, None, opt, _NullWriter(), 0, 1, 5, 10 ** 9, False, 5,
                                                           options=LoopOptions(), microbatch_group=group), DEV, 1)
    assert ret["iterations"] == 10 and len(ret["losses_train"]) == 1 and len(ret["losses_train"][0]) == 5
    return _state(net, opt, ret["losses_train"]), inj


_BASE = {}


def _baseline(key, leg, units):
    """The undelayed leg of a configuration, once per process: a first run records the points of every unit (and warms the
    arenas and the streams up), the second one's `_train` call is timed between two device synchronisations: t_cycle is that
    time over the units (accumulation cycles) of the call, and from it L."""
    if key not in _BASE:
        _, rec = leg(lambda net, opt: D.Injector().wrap_training(net, opt))
        state, timed = leg(lambda net, opt: D.Injector().wrap_training(net, opt))
        t_cycle = timed.ms / units
        L = D.delay_length(t_cycle)
        got = D.calibration(DEV).measured(L)
        occ = rec.units
        _say("%s: t_cycle %.3f ms, L %.3f ms (measured %.3f ms); points of a unit: %s" % (key, t_cycle, L, got, occ[0]))
        # the loop did train: at least 30 tensors moved from their initial values
        sd = _TEMPLATES[29][1]
        moved = sum(int(not torch.equal(v.cpu(), sd[k[2:]])) for k, v in state.items() if k.startswith("w/"))
        assert moved >= 30, moved
        assert sum(k.startswith("w/") for k in state) == 52
        _BASE[key] = (state, occ, L)
    return _BASE[key]


def _delayed_legs(key, leg, units, role, points):
    """Every point of ``points`` the configuration holds, with ``role``'s stream delayed there at a rotating occurrence."""
    streams = _loop_streams()
    for other in _others(role, ("caller", "aux", "pass") if role != "comm" else ("caller", "comm")):
        _loop_pair(role, other, streams)
        if role == "caller" or other == "caller":
            _loop_pair(other, role, streams)
    base, occ, L = _baseline(key, leg, units)
    ran = 0
    for point in points:
        offs = D.offsets(occ, point)
        fired = []
        for off in offs:
            state, inj = leg(lambda net, opt: D.Injector(lambda: D.sleep_ms(streams[role], L), point, occ, off)
                             .wrap_training(net, opt))
            assert inj.counts == _recorded(occ, inj), (key, point)
            assert inj.fired, (key, point)
            diff = _differences(base, state)
            assert not diff, "%s: %s delayed at %s (offset %d): %d tensors differ, first %s" % (key, role, point, off,
                                                                                               len(diff), diff[:3])
            fired.append(inj.fired)
            ran += 1
        assert D.covered(occ, point, fired), (key, point)
    _say("%s: %s delayed, %d legs equal the undelayed leg" % (key, role, ran))
    assert ran


def _recorded(occ, inj):
    """The delayed leg ran the recorded program: the same points in the same units."""
    return occ + [{}] * (len(inj.counts) - len(occ))


@pytest.mark.parametrize("role", D.LOOP_STREAMS)
@pytest.mark.parametrize("split", [True, False], ids=["split_step", "one_step"])
@pytest.mark.parametrize("cfg", list(D.ONLINE_CONFIGS))
def test_online_loop_with_one_stream_late(cfg, split, role):
    """`train_online._train` (typed options; defer_join, grad_overwrite and pass_streams on), three optimizer steps: the weights,
    momentum buffers, gradients and losses are bit for bit the undelayed run's with one stream late at every point."""
    _delayed_legs(("online", cfg, "split" if split else "one_step"), lambda inj: _online_leg(cfg, split, inj), 3, role,
                  D.LOOP_POINTS)


@pytest.mark.parametrize("role", D.LOOP_STREAMS)
@pytest.mark.parametrize("group", D.OFFLINE_GROUPS)
def test_offline_loop_with_one_stream_late(group, role):
    """`train_offline._train`, two optimizer steps of five frames of two shapes, one by one and as batched passes: the same,
    and the five losses of the epoch."""
    _delayed_legs(("offline", group), lambda inj: _offline_leg(group, inj), 2, role,
                  D.OFFLINE_POINTS)


# ---------------------------------------------------------------------------------------------- the mutation checks
def test_mutation_training_a_missing_pass_stream_wait_is_seen():
    """The harness has teeth at these shapes.  The planted missing wait: the wait of the second pass stream on the caller's
    stream in front of a two-stream window (train_online: run_window) is suppressed, with the caller's stream late in front of
    the late optimizer step.  The next window's first pass then reads weights the step has not written and adds to gradients
    the window's memset has not zeroed yet (stale but valid memory): the weights differ (measured: 73 of the compared tensors).

    Why not ``net.wait_grad_bucket``.  Replaced by a no-op, with ``aux`` late in front of the early ``optimizer.step``, of
    ``forward`` or of the backward pass, in one_pass and in two_singles, it changed 0 tensors in 6 of 6 scenarios - and no
    scenario can do better: a cycle's closing pass runs with ``last_pass_of_cycle``, whose tail offload makes the main stream
    wait for kStage2WgradEvent (csrc/vgg_net.hip, the end of fosvos_vgg_backward_flags) before the call returns, and the
    weight-gradient stream records that event behind the bucket events of stages 5-3.  The early step's three bucket waits
    are implied by it: an edge ordered twice, which a delay cannot tell from an edge ordered once."""
    streams = _loop_streams()
    _loop_pair("caller", "pass", streams)
    key = ("online", "two_pairs", "split")
    base, occ, L = _baseline(key, lambda inj: _online_leg("two_pairs", True, inj), 3)
    real = torch.cuda.Stream.wait_stream
    side = streams["pass"].cuda_stream
    skipped = []

    def wait_stream(self, other):
        if self.cuda_stream == side:
            skipped.append(1)
            return None
        return real(self, other)

    torch.cuda.Stream.wait_stream = wait_stream
    try:
        state, inj = _online_leg("two_pairs", True, lambda net, opt: D.Injector(
            lambda: D.sleep_ms(streams["caller"], L), "step:late", occ, 0).wrap_training(net, opt))
    finally:
        torch.cuda.Stream.wait_stream = real
    torch.cuda.synchronize()
    diff = _differences(base, state)
    _say("mutation pass.wait_stream(caller) suppressed (%d times), caller delayed at step:late: %d tensors differ"
         % (len(skipped), len(diff)))
    assert skipped and inj.fired
    assert diff


# ---------------------------------------------------------------------------------------------- data parallel, one RCCL rank
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker_one_rccl_rank(port, out_dir):
    """The child of test_data_parallel_on_one_rccl_rank: the baseline, then one leg per (stream, point) of D.DP_LEGS."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      FOSVOS_DP_SINGLE_RANK="1")
    import parallel
    import train_online
    from fosvos_hip.options import LoopOptions
    assert parallel.init_distributed("nccl") and parallel.collectives_on() and parallel.world_size() == 1
    loader = _loader([(40, 70)] * 4, 2, 170)

    def leg(injector_of):
        net, _ = _fresh_net()
        prov = _provider("online", net)
        opt = prov.get_optimizer(learning_rate=LR)
        train_online.data_parallel = True
        inj = injector_of(net, opt)
        with inj:
            ret, inj.ms = D.timed(lambda: train_online._train(prov, loader, opt, _NullWriter(), "dp", 0, 1, 4, 10 ** 9,
                                                              options=LoopOptions()), DEV, 1)
        assert ret["iterations"] == 8
        return _state(net, opt, ret["loss"]), inj

    streams = _loop_streams()
    _, rec = leg(lambda net, opt: D.Injector().wrap_training(net, opt))
    base, timed = leg(lambda net, opt: D.Injector().wrap_training(net, opt))
    t_cycle = timed.ms / 2
    L = D.delay_length(t_cycle)
    occ = rec.units
    _say("data parallel, one RCCL rank: t_cycle %.3f ms, L %.3f ms (measured %.3f ms); points of a unit: %s"
         % (t_cycle, L, D.calibration(DEV).measured(L), occ[0]))
    result = {"legs": {}, "blind": [], "moved": 0}
    sd = _TEMPLATES[29][1]
    result["moved"] = sum(int(not torch.equal(v.cpu(), sd[k[2:]])) for k, v in base.items() if k.startswith("w/"))
    for role in ("comm", "aux"):
        for a, b in ((role, "caller"), ("caller", role)):
            ok = D.sighted(streams[a], streams[b]) and D.ordered(streams[a], streams[b])
            _say("pair delayed=%s other=%s: %s" % (a, b, "sighted" if ok else "BLIND"))
            if not ok:
                result["blind"].append("%s/%s (%s)" % (a, b, _probe_says(a, b)[1]))
    for role, point in D.DP_LEGS:
        state, inj = leg(lambda net, opt: D.Injector(lambda: D.sleep_ms(streams[role], L), point, occ, 0)
                         .wrap_training(net, opt))
        diff = _differences(base, state)
        result["legs"]["%s@%s" % (role, point)] = {"fired": len(inj.fired), "differ": diff}
        _say("data parallel: %s delayed at %s: %d tensors differ" % (role, point, len(diff)))
    torch.save(result, os.path.join(out_dir, "delays_rccl1.pt"))
    torch.distributed.destroy_process_group()


def test_data_parallel_on_one_rccl_rank(tmp_path):
    """The data-parallel step on ONE rank of the real backend (tests/test_gpu_parallel.py: the all-reduces change no value, the
    communication stream, the bucket events and the split step run as on eight GPUs), in one child process: with ``comm``,
    ``aux`` or the caller's stream late behind ``forward`` and in front of the first ``optimizer.step`` the weights are the
    baseline's, bit for bit."""
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "rccl1", str(_free_port()), str(tmp_path)])
    try:
        assert p.wait(timeout=300) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    res = torch.load(os.path.join(str(tmp_path), "delays_rccl1.pt"))
    assert res["moved"] >= 30
    assert sorted(res["legs"]) == sorted("%s@%s" % leg for leg in D.DP_LEGS)
    for name, leg in res["legs"].items():
        assert leg["fired"] == 2, name     # once per cycle
        assert not leg["differ"], (name, leg["differ"][:3])
    if res["blind"]:
        pytest.skip("data parallel: the legs passed, but blind pair(s) %s could not have shown a missing wait" % res["blind"])


# ---------------------------------------------------------------------------------------------- inference passes of the nets
@pytest.mark.parametrize("role", D.NET_LEGS["vgg_fwd_aux"])
def test_vgg_forward_with_side_convs_on_the_auxiliary_stream(role):
    """``forward`` at N = 2 with ``fwd_aux`` on, the caller's stream or ``aux`` late in front of every call, three calls on
    different inputs: the five maps equal those of ``fwd_aux`` off."""
    streams = _loop_streams()
    _loop_pair(role, "aux" if role == "caller" else "caller", streams)
    net, _ = _fresh_net(23)
    net.eval()
    xs = [O.synthetic_frame(2, 40, 70, seed=810 + i)[0].to(DEV) for i in range(3)]

    def run(fwd_aux, delay):
        net.options = dataclasses.replace(net.options, fwd_aux=fwd_aux)
        outs = []
        with torch.no_grad():
            for x in xs:
                if delay:
                    D.sleep_ms(streams[role], delay)
                outs.append([o.clone() for o in net.forward(x)])
        torch.cuda.synchronize()
        return outs

    ref = run(False, 0)
    run(True, 0)
    plain, t_cycle = D.timed(lambda: run(True, 0), DEV, len(xs))
    L = D.delay_length(t_cycle)
    _say("vgg forward, fwd_aux: t_cycle %.3f ms, L %.3f ms (measured %.3f ms)" % (t_cycle, L, D.calibration(DEV).measured(L)))
    late = run(True, L)
    for got in (plain, late):
        for a, b in zip(got, ref):
            assert len(a) == len(b) == 5 and all(torch.equal(p, q) for p, q in zip(a, b))
    assert not torch.equal(ref[0][-1], ref[1][-1])


@pytest.mark.parametrize("role", D.NET_LEGS["resnet_aux"])
def test_resnet_forward_with_side_convs_on_a_second_stream(role):
    """ResNet-18 at 64x96 with ``EngineOptions.resnet_aux``: the caller's stream or the plan's own second stream late, two calls
    in a row on different inputs (the second finds the first's work on the second stream: busy_ev): the outputs of
    ``resnet_aux`` off."""
    from networks.osvos_resnet import OSVOS_RESNET
    from oracle import osvos_resnet_ref as R
    net = OSVOS_RESNET(pretrained=False, version=18, scale_down_exponent=1)
    net.load_state_dict(R.make_state_dict(18, 1, seed=3))
    net = net.to(DEV).eval()
    xs = [(50.0 * torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(5 + i))).to(DEV) for i in range(2)]
    default = net.options
    caller = torch.cuda.current_stream(torch.device(DEV))

    def run(aux, delay):
        net.options = dataclasses.replace(default, resnet_aux=aux)
        outs = []
        with torch.no_grad():
            for k, x in enumerate(xs):
                if delay and k == 0:   # (once: the second call is queued while the stream still sleeps)
                    D.sleep_ms(caller if role == "caller" else net._plan.aux, delay)
                outs.append([o.clone() for o in net(x)])
        torch.cuda.synchronize()
        return outs

    try:
        ref = run(False, 0)
        run(True, 0)
        assert net._plan.aux is not None

        def fresh():   # (the plan keeps whatever stream it finds in ``aux``: a fresh one per try, the earlier ones kept)
            net._plan.aux = torch.cuda.Stream(device=DEV)
            return net._plan.aux

        _sighted_instance(fresh, lambda st: [("plan.aux->caller", st, caller), ("caller->plan.aux", caller, st)],
                          "resnet plan.aux")
        plain, t_cycle = D.timed(lambda: run(True, 0), DEV, 1)
        L = D.delay_length(t_cycle)
        _say("resnet forward, resnet_aux: t_cycle %.3f ms, L %.3f ms (measured %.3f ms)"
             % (t_cycle, L, D.calibration(DEV).measured(L)))
        late = run(True, L)
    finally:
        net.options = default
    for got in (plain, late):
        for a, b in zip(got, ref):
            assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert not torch.equal(ref[0][-1], ref[1][-1])


# ---------------------------------------------------------------------------------------------- the segmenters
SH, SW, N_FRAMES = 48, 80, 12
_SEG_NETS = {}


def _seg_net(seed=2):
    if seed not in _SEG_NETS:
        from networks.osvos_vgg import OSVOS_VGG
        net = OSVOS_VGG(pretrained=0)
        net.load_state_dict(O.make_state_dict(seed))
        _SEG_NETS[seed] = net.to(DEV).eval()
    return _SEG_NETS[seed]


def _camera_frames():
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:SH, 0:SW]
    frames = []
    for k in range(N_FRAMES):   # distinct consecutive frames: a bright blob that moves over noise
        f = rng.integers(0, 120, (SH, SW, 3), dtype=np.uint8)
        blob = ((y - 20 - k) ** 2 + (x - 20 - 3 * k) ** 2) < 100
        f[blob] = 200 + rng.integers(0, 55, (int(blob.sum()), 3), dtype=np.uint8)
        frames.append(f)
    return frames


def _annotation():
    y, x = np.mgrid[0:SH, 0:SW]
    return (((y - 20) ** 2 + (x - 20) ** 2) < 100).astype(np.uint8)


def _make_segmenter(form, depth):
    from fosvos_hip.options import CleanOptions, RefineOptions, RoiOptions
    from fosvos_hip.stream import FrameSegmenter, ObjectSegmenter
    net = _seg_net()
    if form == "objects_png":
        return ObjectSegmenter([net, _seg_net(3)], SH, SW, depth=depth, overlay=False, encode="png", budget=64)
    kw = {"plain": {}, "device_frame": {}, "net_size": {"net_size": (24, 40)},
          "jpeg_second_copy": {"encode": "jpeg", "budget": 64},
          "clean_temporal": {"clean": CleanOptions(min_area=4, temporal_radius=6)},
          "roi": {"roi": RoiOptions(levels=4, min_pad=4), "net_size": (24, 40)},
          "refine": {"refine": RefineOptions(radius=2), "net_size": (24, 40)}}[form]
    return FrameSegmenter(net, SH, SW, depth=depth, **kw)


def _seg_streams(seg, net_stream):
    return {"net": net_stream, "up": seg._up, "down": seg._down}


def _seg_start(seg, form):
    """Every run starts from the same hand-over state: the seed / the window of an annotation."""
    if form == "clean_temporal":
        seg.seed(_annotation())
    elif form == "roi":
        seg.seed_window(_annotation())


def _seg_inputs(form, frames):
    if form == "device_frame":
        return [torch.from_numpy(f).to(DEV) for f in frames]
    return frames


def _as_bytes(out):
    return out if isinstance(out, bytes) else out.tobytes()


def _seg_run(seg, form, frames, net_stream, leg=None, L=0.0):
    """``segment()`` over the frames, with ``leg`` = (role, point) delayed once per submit..result unit."""
    _seg_start(seg, form)
    streams = _seg_streams(seg, net_stream)
    rec = D.Injector(unit_ends=("submit",)).wrap(seg, "submit", before="submit", after="submit/end") \
        .wrap(seg, "_compute", before="compute")
    if leg is None:
        inj = rec
    else:
        role, point = leg
        occ = [{"submit": 1, "compute": 1}] * len(frames)
        inj = D.Injector(lambda: D.sleep_ms(streams[role], L), point, occ, 0, unit_ends=("submit",)) \
            .wrap(seg, "submit", before="submit", after="submit/end").wrap(seg, "_compute", before="compute")
    with inj:
        outs = [_as_bytes(o) for o in seg.segment(_seg_inputs(form, frames))]
    torch.cuda.synchronize()
    assert inj.units == [{"submit": 1, "compute": 1}] * len(frames)
    assert leg is None or len(inj.fired) == len(frames)
    return outs


_SEG_REF = {}


def _seg_reference(form, frames):
    """``apply()`` frame by frame on a segmenter of its own, once per form."""
    if form not in _SEG_REF:
        seg = _make_segmenter(form, 1)
        _seg_start(seg, form)
        _SEG_REF[form] = [_as_bytes(seg.apply(f)) for f in _seg_inputs(form, frames)]
        torch.cuda.synchronize()
        if form in ("jpeg_second_copy", "objects_png"):
            assert seg.second_copies == len(frames)   # every file is longer than the budget: the second copy on _rest
        seg.close()
        distinct = len(set(_SEG_REF[form]))   # distinct outputs: a stale slot would show
        _say("segmenter %s: %d distinct outputs of %d frames" % (form, distinct, len(frames)))
        assert distinct == len(frames) or (form == "objects_png" and distinct >= 2)  # (label maps carry no frame bytes)
    return _SEG_REF[form]


def _segmenter_pairs(net_stream):
    def pairs(seg):
        return [("up->net", seg._up, net_stream), ("net->down", net_stream, seg._down), ("down->net", seg._down, net_stream)]
    return pairs


@pytest.mark.parametrize("depth", D.SEGMENTER_DEPTHS)
@pytest.mark.parametrize("form", D.SEGMENTER_FORMS)
def test_segmenter_with_one_stream_late(form, depth):
    """Twelve distinct 48x80 frames through a segmenter of every form, depth 1, 2 and 3: with the net's stream, ``_up`` or
    ``_down`` late once per frame the outputs (files where there are files) are byte for byte those of the undelayed
    ``segment()`` and of ``apply()`` frame by frame."""
    frames = _camera_frames()
    ref = _seg_reference(form, frames)
    net_stream = torch.cuda.current_stream(torch.device(DEV))
    what = "segmenter %s depth %d" % (form, depth)
    seg, kept = _sighted_instance(lambda: _make_segmenter(form, depth), _segmenter_pairs(net_stream), what)
    try:
        _seg_run(seg, form, frames, net_stream)
        base, t_cycle = D.timed(lambda: _seg_run(seg, form, frames, net_stream), DEV, len(frames))
        L = D.delay_length(t_cycle)
        _say("%s: t_cycle %.3f ms, L %.3f ms (measured %.3f ms)" % (what, t_cycle, L, D.calibration(DEV).measured(L)))
        assert base == ref, what
        for leg in D.SEGMENTER_LEGS:
            got = _seg_run(seg, form, frames, net_stream, leg, L)
            bad = [i for i, (a, b) in enumerate(zip(got, ref)) if a != b]
            assert not bad, "%s: %s delayed at %s: frames %s differ" % (what, leg[0], leg[1], bad)
    finally:
        for s in kept:
            s.close()
        torch.cuda.synchronize()


def test_segmenter_on_a_stream_of_the_callers_choice():
    """The net's stream is the current stream at ``submit``: one leg with a non-default current stream, itself the late one."""
    frames = _camera_frames()
    ref = _seg_reference("plain", frames)
    kept_streams = []

    def make():
        st = torch.cuda.Stream(device=DEV)
        kept_streams.append(st)
        seg = _make_segmenter("plain", 2)
        seg._net_stream = st
        return seg

    seg, kept = _sighted_instance(make, lambda s: _segmenter_pairs(s._net_stream)(s), "segmenter on a caller's stream")
    st = seg._net_stream
    try:
        st.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
        with torch.cuda.stream(st):
            base, t_cycle = D.timed(lambda: _seg_run(seg, "plain", frames, st), DEV, len(frames))
            L = D.delay_length(t_cycle)
            assert base == ref
            for leg in D.SEGMENTER_LEGS:
                assert _seg_run(seg, "plain", frames, st, leg, L) == ref, leg
    finally:
        for s in kept:
            s.close()
        torch.cuda.synchronize()


def test_mutation_segmenter_a_missing_upload_wait_is_seen():
    """The harness has teeth here too: with the wait of the net's stream on ``slot.moved`` suppressed for one FrameSegmenter
    and ``_up`` late in front of every ``submit``, the net reads the slot's frame before the upload has written it (what the
    slot held: an earlier frame, valid memory), and the outputs differ."""
    frames = _camera_frames()
    ref = _seg_reference("plain", frames)
    net_stream = torch.cuda.current_stream(torch.device(DEV))
    seg, kept = _sighted_instance(lambda: _make_segmenter("plain", 2), _segmenter_pairs(net_stream), "mutated segmenter")
    real = torch.cuda.Stream.wait_event
    try:
        base, t_cycle = D.timed(lambda: _seg_run(seg, "plain", frames, net_stream), DEV, len(frames))
        assert base == ref
        L = D.delay_length(t_cycle)
        moved = {id(slot.moved) for slot in seg._free}
        assert len(moved) == 2
        skipped = []

        def wait_event(self, event):
            if id(event) in moved and self.cuda_stream == net_stream.cuda_stream:
                skipped.append(1)
                return None
            return real(self, event)

        torch.cuda.Stream.wait_event = wait_event
        try:
            got = _seg_run(seg, "plain", frames, net_stream, ("up", "submit"), L)
        finally:
            torch.cuda.Stream.wait_event = real
        bad = [i for i, (a, b) in enumerate(zip(got, ref)) if a != b]
        _say("mutation main.wait_event(slot.moved) suppressed (%d times), _up delayed at submit: frames %s differ"
             % (len(skipped), bad))
        assert len(skipped) == len(frames)
        assert bad
        # ... and the same segmenter with the wait back in place is right again
        assert _seg_run(seg, "plain", frames, net_stream, ("up", "submit"), L) == ref
    finally:
        torch.cuda.Stream.wait_event = real
        for s in kept:
            s.close()
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the decoding loader
def _davis_tree(root, count, seq="blob"):
    """Twelve small JPEG files made by PIL, as a DAVIS tree with the first frame's annotation."""
    from PIL import Image
    for sub in ("ImageSets", "JPEGImages", "Annotations"):
        (root / sub / "480p" / (seq if sub != "ImageSets" else "")).mkdir(parents=True)
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:SH, 0:SW]
    lines = []
    for k in range(count):
        img = (2 * x + 3 * y + 16 * k)[..., None] % 256 + rng.integers(-20, 21, (SH, SW, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(str(root / "JPEGImages" / "480p" / seq / ("%05d.jpg" % k)),
                                                                    "JPEG", quality=92, subsampling=2)
        lines.append("/JPEGImages/480p/%s/%05d.jpg /Annotations/480p/%s/%05d.png" % (seq, k, seq, k))
    for name in ("trainval.txt", "val.txt", "train.txt"):
        (root / "ImageSets" / "480p" / name).write_text("\n".join(lines) + "\n")
    Image.fromarray(_annotation() * 255).save(str(root / "Annotations" / "480p" / seq / "00000.png"))
    return root


def test_decoding_loader_with_one_stream_late(tmp_path):
    """Twelve JPEG files, four a launch: three windows alternate between the loader's two streams.  With the window's stream
    late in front of its ``_launch``, or the consumer's stream late while every yielded image is cloned (a block recycled too
    early would show), the minibatches are bit for bit the undelayed loader's."""
    from dataloaders.device_decode import DeviceDecodeLoader
    from util import io_helper
    root = _davis_tree(tmp_path / "davis", 12)
    dataset = io_helper.get_data_loader_test(root, 1, "blob", device_decode=True).dataset
    consumer = torch.cuda.current_stream(torch.device(DEV))

    def pairs(ld):
        out = []
        for i, st in enumerate(ld._streams):
            out += [("decode%d->consumer" % i, st, consumer), ("consumer->decode%d" % i, consumer, st)]
        return out

    loader, kept = _sighted_instance(lambda: DeviceDecodeLoader(dataset, files_per_launch=4), pairs, "decoding loader")

    def run(leg=None, L=0.0):
        loader._windows = 0
        inj = D.Injector(unit_ends=("launch",)).wrap(loader, "_launch", before="launch", after="launch/end")
        if leg == "decode":
            inj = D.Injector(lambda: D.sleep_ms(loader._streams[loader._windows % 2], L), "launch", [{"launch": 1}] * 3, 0,
                             unit_ends=("launch",)).wrap(loader, "_launch", before="launch", after="launch/end")
        images, names = [], []
        with inj:
            for i, batch in enumerate(loader):
                if leg == "consumer" and i % 4 == 0:   # once per window; every image of it is cloned behind the sleep
                    D.sleep_ms(consumer, L)
                images.append(batch["image"].clone())
                names += list(batch["fname"])
                del batch
        torch.cuda.synchronize()
        assert inj.units == [{"launch": 1}] * 3 and loader.decoded == 12 and loader.fallbacks == 0
        assert leg != "decode" or len(inj.fired) == 3
        return [im.cpu() for im in images], names

    run()
    (base, names), t_cycle = D.timed(run, DEV, 3)
    L = D.delay_length(t_cycle)
    _say("decoding loader: t_cycle %.3f ms, L %.3f ms (measured %.3f ms)" % (t_cycle, L, D.calibration(DEV).measured(L)))
    assert len(base) == 12 and len({im.numpy().tobytes() for im in base}) == 12
    host = [b["image"] for b in io_helper.get_data_loader_test(root, 1, "blob")]
    assert all(torch.equal(a, b) for a, b in zip(base, host))
    for role, _ in D.LOADER_LEGS:
        got, got_names = run(role, L)
        assert got_names == names
        bad = [i for i, (a, b) in enumerate(zip(got, base)) if not torch.equal(a, b)]
        assert not bad, "decoding loader: %s delayed: images %s differ" % (role, bad)
    del kept


if __name__ == "__main__":
    assert sys.argv[1] == "rccl1"
    _worker_one_rccl_rank(int(sys.argv[2]), sys.argv[3])
