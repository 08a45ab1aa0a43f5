"""The host logic of tests/stream_delays.py, without a GPU: the Injector on a CPU run of the shipped ``train_online._train``
(the stand-in net and loss of tests/test_parallel_train_cpu.py), a recorder in place of the sleep; the rotation of the
occurrence; the restoring of every wrapped attribute; the scenario tables."""
import pytest
import torch

import stream_delays as D
import test_parallel_train_cpu as T


@pytest.fixture(autouse=True)
def _cpu_minibatches(monkeypatch):
    import train_online
    from util import gpu_handler
    monkeypatch.setattr(gpu_handler, "cast_cuda_if_possible", T._inputs_on_the_cpu)
    # (the stand-in loss and the single-process mode for the test only: both names are what they were afterwards)
    monkeypatch.setattr(train_online, "class_balanced_cross_entropy_loss", T._cbce)
    monkeypatch.setattr(train_online, "data_parallel", False)


def _run(injector_of, epochs=3, avg=4, group=1):
    """`train_online._train` on the CPU stand-in: ``epochs`` cycles of ``avg`` one-frame passes."""
    import train_online
    from fosvos_hip.options import LoopOptions
    net = T.TinyOSVOS()
    opt = T._sgd(net)
    inj = injector_of(net, opt)
    with inj:
        train_online._train(T._Prov(net), T._frames(avg), opt, T._Writer(), "tiny", 0, epochs, avg, 10 ** 9,
                            options=LoopOptions(microbatch_group=group))
    return net, opt, inj


def test_every_point_of_a_cpu_run_is_counted():
    """Three cycles of four one-frame passes: every cycle holds four forwards (each a point in front of and one behind the
    call), one join and one plain optimizer step, which closes the unit; the loop's last join (its ``finally``) is alone in
    the open unit behind them.  The loss is not wrapped: the name the loop tests by identity is the one the test set."""
    import train_online
    net, opt, inj = _run(lambda net, opt: D.Injector().wrap_training(net, opt))
    assert train_online.class_balanced_cross_entropy_loss is T._cbce
    cycle = {"forward:before": 4, "forward:after": 4, "join": 1, "step:plain": 1}
    assert inj.counts == [cycle, cycle, cycle, {"join": 1}]
    assert inj.units == inj.counts and inj.fired == []
    # a batched cycle: one forward
    _, _, one = _run(lambda net, opt: D.Injector().wrap_training(net, opt), group=5)
    assert one.counts[:3] == [{"forward:before": 1, "forward:after": 1, "join": 1, "step:plain": 1}] * 3


def test_the_points_a_native_module_adds():
    """``wait_grad_bucket`` and ``prepack_weights`` are points where the module has them, and ``optimizer.step`` is three
    points by its tag."""
    class Net:
        def forward(self, x):
            return x

        def join_gradients(self):
            pass

        def wait_grad_bucket(self, b):
            return b

        def prepack_weights(self, prefixes=None):
            return prefixes

    class Opt:
        def step(self, only=None, tag=None, zero_grad=True):
            return tag

    net, opt = Net(), Opt()
    with D.Injector().wrap_training(net, opt) as inj:
        assert net.forward(3) == 3 and net.wait_grad_bucket(2) == 2 and net.prepack_weights(("a",)) == ("a",)
        assert opt.step(only=[], tag="early") == "early"
        net.join_gradients()
        assert opt.step(only=[], tag="late") == "late"
        assert opt.step() is None
    assert inj.counts == [{"forward:before": 1, "forward:after": 1, "bucket": 1, "prepack": 1, "step:early": 1, "join": 1,
                           "step:late": 1}, {"step:plain": 1}, {}]
    assert inj.units == inj.counts[:2]


@pytest.mark.parametrize("point,per_unit", [("forward:before", 4), ("forward:after", 4), ("join", 1), ("step:plain", 1)])
def test_the_occurrence_rotates_over_the_units(point, per_unit):
    """A leg fires once per unit, at occurrence (unit + offset) % n; three units and four occurrences need the offsets 0 and
    3, and with both legs every occurrence has been hit."""
    _, _, rec = _run(lambda net, opt: D.Injector().wrap_training(net, opt))
    occ = rec.units
    offs = D.offsets(occ, point)
    assert offs == ([0, 3] if per_unit == 4 else [0])
    fired = []
    for off in offs:
        calls = []
        _, _, inj = _run(lambda net, opt: D.Injector(lambda: calls.append(1), point, occ, off).wrap_training(net, opt))
        # at most once per unit (the open unit behind the last step holds the loop's closing join: once more for "join")
        assert len(calls) == len(inj.fired) == 3 + (point == "join")
        assert [u for u, _, _ in inj.fired] == list(range(len(inj.fired)))
        assert all(name == point and k == (u + off) % occ[u][point] for u, name, k in inj.fired)
        assert inj.counts == rec.counts   # the recorder and the firing leg saw the same program
        fired.append(inj.fired)
    assert D.covered(occ, point, fired)
    assert not D.covered(occ, point, fired[:1]) or per_unit == 1
    assert D.offsets(occ, "prepack") == [] and D.covered(occ, "prepack", [])


def test_the_delayed_run_computes_what_the_plain_run_does():
    """Wrapping changes no value: the weights of a wrapped, firing run are the unwrapped run's."""
    ref = T._run_online(T._frames(4), 4, False)
    _, _, rec = _run(lambda net, opt: D.Injector().wrap_training(net, opt), epochs=1)
    net, _, _ = _run(lambda net, opt: D.Injector(lambda: None, "forward:after", rec.units).wrap_training(net, opt), epochs=1,
                     group=5)
    for k, v in ref.state_dict().items():
        assert torch.equal(v, net.state_dict()[k]), k


def test_attributes_are_restored():
    """After a normal exit and after an exception every wrapped attribute is what it was: a method of the class is again the
    class's (nothing left in the instance), an instance attribute and a module attribute are the objects they were."""
    net = T.TinyOSVOS()
    opt = T._sgd(net)
    own = lambda: None                                              # noqa: E731 - an attribute of the instance itself
    net.join_gradients = own
    import types
    mod = types.ModuleType("m")
    mod.fn = own

    def check():
        assert "forward" not in net.__dict__ and net.forward.__func__ is T.TinyOSVOS.forward
        assert "step" not in opt.__dict__ and net.__dict__["join_gradients"] is own and mod.fn is own

    inj = D.Injector().wrap_training(net, opt).wrap(mod, "fn", before="launch")
    check()                                                         # nothing is patched before the context is entered
    with inj:
        assert "forward" in net.__dict__ and "step" in opt.__dict__ and mod.fn is not own
        mod.fn()
    check()
    assert inj.counts[0] == {"launch": 1}
    with pytest.raises(RuntimeError, match="inside"):
        with D.Injector().wrap_training(net, opt).wrap(mod, "fn", before="launch"):
            raise RuntimeError("inside")
    check()
    # an exception out of a wrapped call, and out of the action itself
    with pytest.raises(RuntimeError, match="loader failed"):
        _failing(net, opt)
    check()

    def boom():
        raise ValueError("action")
    with pytest.raises(ValueError, match="action"):
        with D.Injector(boom, "launch", [{"launch": 1}]).wrap(mod, "fn", before="launch"):
            mod.fn()
    check()
    with pytest.raises(TypeError):
        D.Injector().wrap(net, "compute_side_outputs", before="compute")
    with pytest.raises(ValueError):
        D.Injector(lambda: None, "no such point", [])
    with pytest.raises(ValueError):
        D.Injector(None, "join", [])


def _failing(net, opt):
    import train_online
    with D.Injector().wrap_training(net, opt):
        train_online._train(T._Prov(net), T._FailingLoader(T._frames(4)), opt, T._Writer(), "tiny", 0, 1, 2, 10 ** 9)


def test_units_of_a_segmenter_and_a_loader():
    """``submit`` ends a segmenter's unit and ``_launch`` the loader's, both when the call returns."""
    class Seg:
        def submit(self, f):
            self._compute(f)

        def _compute(self, f):
            pass

    seg = Seg()
    inj = D.Injector(unit_ends=("submit",)).wrap(seg, "submit", before="submit", after="submit/end") \
        .wrap(seg, "_compute", before="compute")
    with inj:
        for f in range(3):
            seg.submit(f)
    assert inj.units == [{"submit": 1, "compute": 1}] * 3
    calls = []
    with D.Injector(lambda: calls.append(1), "compute", inj.units, unit_ends=("submit",)) \
            .wrap(seg, "submit", before="submit", after="submit/end").wrap(seg, "_compute", before="compute") as fire:
        for f in range(3):
            seg.submit(f)
    assert len(calls) == 3 and fire.fired == [(0, "compute", 0), (1, "compute", 0), (2, "compute", 0)]


def test_the_delay_length():
    assert D.delay_length(0.1) == 2.0 and D.delay_length(0.5) == 2.0 and D.delay_length(4.0) == 12.0


def test_scenario_tables_list_every_role_and_point():
    legs = [leg for table in D.SCENARIOS.values() for leg in table]
    assert {role for role, _ in legs} == set(D.STREAM_ROLES)
    assert {point for _, point in legs} == set(D.POINTS) - {"bucket"}   # (counted, never a place of a delay: the early step is)
    assert all(point in D.POINTS for _, point in legs)
    assert set(D.LOOP_STREAMS) == {"caller", "aux", "pass", "comm"}
    assert set(D.ONLINE_CONFIGS) == {"one_pass", "two_pairs", "two_singles", "cycle_over_two_windows"}
    for sizes, avg, fields in D.ONLINE_CONFIGS.values():
        assert len(sizes) == avg
        from fosvos_hip.options import LoopOptions
        LoopOptions(**fields)
    assert len(D.SEGMENTER_FORMS) == 8 and D.SEGMENTER_DEPTHS == (1, 2, 3)
