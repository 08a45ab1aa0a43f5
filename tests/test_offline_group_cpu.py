"""CPU checks of the offline loop's batched accumulation cycle (``train_offline._train(..., microbatch_group=N)``): the
flag, the pure planning functions (window boundaries, shape buckets, group cuts), and - with a CPU stand-in network and loss
bound as in tests/test_parallel_train_cpu.py - that the default runs today's calls and a grouped run the planned passes."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_parallel_train_cpu import TinyOSVOS, _Prov, _Writer, _cbce, _inputs_on_the_cpu, _sgd  # noqa: E402


@pytest.fixture(autouse=True)
def _cpu_minibatches(monkeypatch):
    from util import gpu_handler
    monkeypatch.setattr(gpu_handler, "cast_cuda_if_possible", _inputs_on_the_cpu)


# ------------------------------------------------------------------------------------------ the flag
def test_microbatch_group_flag_is_offline_only():
    from util import args_helper
    assert args_helper.parse_args(is_online=False, argv=[]).microbatch_group == 1
    assert args_helper.parse_args(is_online=False, argv=["--microbatch-group", "5"]).microbatch_group == 5
    assert not hasattr(args_helper.parse_args(is_online=True, argv=[]), "microbatch_group")
    with pytest.raises(SystemExit):
        args_helper.parse_args(is_online=True, argv=["--microbatch-group", "5"])
    for bad in ("0", "-3", "two"):
        with pytest.raises(SystemExit):
            args_helper.parse_args(is_online=False, argv=["--microbatch-group", bad])
    with pytest.raises(SystemExit):  # that mode splits a batch with the class counts of the whole batch
        args_helper.parse_args(is_online=False, argv=["--microbatch-group", "2", "--data-parallel"])


def test_offline_main_hands_the_group_to_train(monkeypatch, tmp_path):
    """main() sets the module global, train_and_test passes it to `_train` as the keyword."""
    import train_offline
    from util import io_helper
    seen = {}

    def fake_train(*a, **k):
        seen["group"] = k.get("microbatch_group")
        return {}

    class _P:
        name = "vgg16"

        def load_network_train(self):
            pass

        def get_optimizer(self):
            return None

    real_train_and_test = train_offline.train_and_test

    def spying_train_and_test(prov, settings):
        seen["global"] = train_offline.microbatch_group
        real_train_and_test(_P(), settings)

    monkeypatch.setattr(train_offline, "_train", fake_train)
    monkeypatch.setattr(train_offline, "train_and_test", spying_train_and_test)
    monkeypatch.setattr(train_offline, "_get_summary_writer", lambda: _Writer())
    monkeypatch.setattr(io_helper, "write_settings", lambda *a, **k: None)
    monkeypatch.setattr(io_helper, "get_data_loader_train", lambda *a, **k: [])
    monkeypatch.setattr(io_helper, "get_data_loader_test", lambda *a, **k: [])
    monkeypatch.setattr(train_offline.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_offline, "microbatch_group", 1)
    monkeypatch.setattr(train_offline, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_offline, "save_dir_results", tmp_path / "results")
    train_offline.main(["--microbatch-group", "4", "--no-testing", "--synthetic"])
    assert seen == {"global": 4, "group": 4}
    train_offline.main(["--no-testing", "--synthetic"])
    assert seen == {"global": 1, "group": 1}


# ------------------------------------------------------------------------------------------ planning
A, B, C = (1, 3, 48, 86), (1, 3, 64, 108), (1, 3, 24, 36)
ODD = (1, 3, 61, 107)      # H x W = 6527: the per-frame kernels read 16-byte vectors
PAIR = (2, 3, 48, 86)      # a minibatch of two frames: class counts over the whole tensor


def test_plan_passes_buckets_by_shape_in_order_of_first_appearance():
    from accumulation import plan_passes
    assert plan_passes([A, B, A, C, B], 5) == [([0, 2], True), ([1, 4], True), ([3], True)]
    assert plan_passes([B, A, A, B], 5) == [([0, 3], True), ([1, 2], True)]
    assert plan_passes([A], 5) == [([0], True)]
    assert plan_passes([], 5) == []
    # torch.Size is what the loop passes
    assert plan_passes([torch.Size(A), torch.Size(A)], 2) == [([0, 1], True)]


def test_plan_passes_cuts_a_bucket_into_groups():
    from accumulation import plan_passes
    assert plan_passes([A] * 7, 3) == [([0, 1, 2], True), ([3, 4, 5], True), ([6], True)]
    assert plan_passes([A, B] * 3, 2) == [([0, 2], True), ([4], True), ([1, 3], True), ([5], True)]
    assert plan_passes([A] * 3, 1) == [([0], True), ([1], True), ([2], True)]


def test_plan_passes_keeps_batches_and_odd_frames_alone():
    from accumulation import plan_passes
    got = plan_passes([A, PAIR, A, ODD, ODD, PAIR], 5)
    assert got == [([0, 2], True), ([1], False), ([3], False), ([4], False), ([5], False)]
    # every minibatch runs exactly once
    for shapes, group in (([A, PAIR, B, ODD, A, B, B, C], 2), ([ODD] * 3, 4), ([PAIR, PAIR], 5)):
        passes = plan_passes(shapes, group)
        assert sorted(i for idx, _ in passes for i in idx) == list(range(len(shapes)))
        assert all(len(idx) <= group for idx, _ in passes)
        assert all(len({shapes[i] for i in idx}) == 1 for idx, _ in passes)


def _windows(n_minibatches, n_epochs, accum, max_window, counter=0):
    """The windows the loop forms: (epoch, first index, length) - a replica of the loop's collection around window_closes."""
    from accumulation import window_closes
    out = []
    for epoch in range(n_epochs):
        n = 0
        for index in range(n_minibatches):
            n += 1
            if window_closes(n, counter, accum, max_window, index == n_minibatches - 1):
                out.append((epoch, index + 1 - n, n))
                counter = (counter + n) % accum
                n = 0
        assert n == 0  # the end of the epoch closed the last window
    return out


def test_windows_end_with_the_cycle_the_epoch_and_the_window_length():
    # 12 minibatches per epoch, a step every 5: the cycles straddle the epoch end, the windows do not
    assert _windows(12, 2, 5, 16) == [(0, 0, 5), (0, 5, 5), (0, 10, 2), (1, 0, 3), (1, 3, 5), (1, 8, 4)]
    # the window length caps a window inside a cycle; what is left of the cycle caps the next one
    assert _windows(10, 1, 10, 4) == [(0, 0, 4), (0, 4, 4), (0, 8, 2)]
    assert _windows(7, 1, 3, 2) == [(0, 0, 2), (0, 2, 1), (0, 3, 2), (0, 5, 1), (0, 6, 1)]
    # a cycle that opened in an earlier epoch: its rest closes the first window
    assert _windows(4, 1, 5, 16, counter=3) == [(0, 0, 2), (0, 2, 2)]
    assert _windows(3, 1, 1, 16) == [(0, 0, 1), (0, 1, 1), (0, 2, 1)]


# ------------------------------------------------------------------------------------------ the loop on CPU stand-ins
def _frames(shapes, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [{"image": torch.randn(n, 3, h, w, generator=g), "gt": (torch.rand(n, 1, h, w, generator=g) > 0.7).float()}
            for n, h, w in shapes]


def _run(monkeypatch, loader, avg, n_epochs=2, loss=_cbce, **kw):
    import train_offline
    monkeypatch.setattr(train_offline, "class_balanced_cross_entropy_loss", loss)
    monkeypatch.setattr(train_offline, "data_parallel", False)
    net = TinyOSVOS()
    shapes = []
    forward = net.forward
    net.forward = lambda x: (shapes.append(tuple(x.shape)), forward(x))[1]
    ret = train_offline._train(_Prov(net), loader, None, _sgd(net), _Writer(), 0, n_epochs, avg, 10 ** 9, False, 5, **kw)
    del net.forward
    return net, ret, shapes


def test_default_group_calls_the_loss_exactly_as_today(monkeypatch):
    """microbatch_group = 1 (and no keyword at all): one pass per minibatch, through the module-level loss - five calls per
    minibatch with its whole tensors, size_average=False, no batch counts - and the weights of a run without the keyword."""
    import train_offline
    calls = []

    def spy(output, label, size_average=True, batch_counts=None):
        calls.append((tuple(output.shape), tuple(label.shape), size_average, batch_counts))
        return _cbce(output, label, size_average=size_average, batch_counts=batch_counts)

    loader = _frames([(1, 10, 12), (1, 8, 10), (2, 10, 12), (1, 10, 12)])
    net0, ret0, shapes0 = _run(monkeypatch, loader, 3, loss=spy)
    calls0 = list(calls)
    del calls[:]
    net1, ret1, shapes1 = _run(monkeypatch, loader, 3, loss=spy, microbatch_group=1)
    assert calls == calls0 and len(calls) == 2 * 4 * 5
    expect = [s for mb in loader for s in [tuple(mb["gt"].shape)] * 5] * 2
    assert [c[0] for c in calls] == expect and [c[1] for c in calls] == expect
    assert all(c[2] is False and c[3] is None for c in calls)
    assert shapes0 == shapes1 == [tuple(mb["image"].shape) for mb in loader] * 2
    assert ret0["iterations"] == ret0["passes"] == ret1["passes"] == 8
    assert set(ret1) == {"loss_train", "loss_test", "losses_train", "iterations", "passes", "seconds"}
    assert ret0["losses_train"] == ret1["losses_train"]
    for k, v in net0.state_dict().items():
        assert torch.equal(v, net1.state_dict()[k]), k
    assert train_offline.microbatch_group == 1


def test_grouped_loop_runs_the_planned_passes(monkeypatch):
    """Seven minibatches per epoch, a step every 3, group 2: the passes are the plan's - by shape inside a window, never
    across a step or the epoch end - and the update and the epoch log equal the one-by-one run's to fp32 rounding."""
    a, b, pair, odd = (1, 10, 12), (1, 8, 10), (2, 10, 12), (1, 5, 7)
    loader = _frames([a, b, a, a, pair, odd, b])
    net1, ret1, shapes1 = _run(monkeypatch, loader, 3)
    net2, ret2, shapes2 = _run(monkeypatch, loader, 3, microbatch_group=2)
    A2, A1, B1, P, O = (2, 3, 10, 12), (1, 3, 10, 12), (1, 3, 8, 10), (2, 3, 10, 12), (1, 3, 5, 7)
    # epoch 0: windows [a b a] [a pair odd] [b]; epoch 1 (the cycle has one iteration in it): [a b] [a a pair] [odd b]
    assert shapes2 == [A2, B1, A1, P, O, B1,
                       A1, B1, A2, P, O, B1]
    assert ret2["iterations"] == ret1["iterations"] == 14 and ret1["passes"] == 14 and ret2["passes"] == 12
    assert len(ret2["losses_train"]) == 2 and len(ret2["losses_train"][0]) == 5
    assert torch.allclose(torch.tensor(ret2["losses_train"]), torch.tensor(ret1["losses_train"]), rtol=1e-5)
    moved = 0
    init = TinyOSVOS().state_dict()
    for k, v in net1.state_dict().items():
        assert torch.allclose(v, net2.state_dict()[k], rtol=1e-5, atol=1e-7), k
        moved += int(not torch.equal(v, init[k]))
    assert moved >= 20


def test_grouped_loop_rejects_data_parallel_and_bad_groups(monkeypatch):
    import train_offline
    monkeypatch.setattr(train_offline, "class_balanced_cross_entropy_loss", _cbce)
    net = TinyOSVOS()
    args = (_Prov(net), _frames([(1, 10, 12)]), None, _sgd(net), _Writer(), 0, 1, 2, 10 ** 9, False, 5)
    monkeypatch.setattr(train_offline, "data_parallel", True)
    with pytest.raises(ValueError, match="data_parallel"):
        train_offline._train(*args, microbatch_group=2)
    monkeypatch.setattr(train_offline, "data_parallel", False)
    with pytest.raises(ValueError):
        train_offline._train(*args, microbatch_group=0)
    assert net.defer_wgrad_join is False


def test_a_failing_grouped_loop_restores_the_module(monkeypatch):
    from test_parallel_train_cpu import _FailingLoader
    import train_offline
    monkeypatch.setattr(train_offline, "class_balanced_cross_entropy_loss", _cbce)
    monkeypatch.setattr(train_offline, "data_parallel", False)
    net = TinyOSVOS()
    with pytest.raises(RuntimeError, match="loader failed"):
        train_offline._train(_Prov(net), _FailingLoader(_frames([(1, 10, 12)] * 4)), None, _sgd(net), _Writer(), 0, 2, 2,
                             10 ** 9, False, 5, microbatch_group=2)
    assert net.compute_side_outputs is True and net.defer_wgrad_join is False
