"""CPU checks of the accumulation-cycle layer both training loops stand on (``fosvos_amd/accumulation.py``): the online loop's
grouping (``plan_passes(..., odd_alone=False)``) against a replica of the bucketing that loop used to do itself, the windows
the online loop forms around ``window_closes``, the cycle counter, and the module state a loop sets and gives back."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_offline_group_cpu import A, B, C, ODD, PAIR  # noqa: E402


# ------------------------------------------------------------------------------------------ the online loop's grouping
def _inline_bucketing(shapes, max_group):
    """What ``train_online._train`` computed inline before it used plan_passes, on (index, shape) items: index lists."""
    window = [(i, tuple(s)) for i, s in enumerate(shapes)]
    buckets = {}
    for item in window:
        shape = item[1]
        buckets.setdefault(shape if shape[0] == 1 else ('batch', id(item)), []).append(item)
    groups = [items[i:i + max_group] for items in buckets.values() for i in range(0, len(items), max_group)]
    return [[item[0] for item in group] for group in groups]


def test_plan_passes_without_odd_alone_is_the_online_grouping():
    from accumulation import plan_passes
    # only a minibatch of several frames runs alone; an H x W that is no multiple of 4 still buckets
    assert [idx for idx, _ in plan_passes([A, PAIR, A, ODD, ODD, B], 5, odd_alone=False)] == [[0, 2], [1], [3, 4], [5]]
    assert plan_passes([A, PAIR, A, ODD, ODD, B], 5, odd_alone=False) == [([0, 2], True), ([1], False), ([3, 4], True),
                                                                          ([5], True)]
    assert [idx for idx, _ in plan_passes([A] * 7, 3, odd_alone=False)] == [[0, 1, 2], [3, 4, 5], [6]]
    assert plan_passes([], 3, odd_alone=False) == []
    for shapes, group in (([A, B, A, C, B], 5), ([B, A, A, B], 2), ([A, PAIR, B, ODD, A, B, B, C], 2), ([ODD] * 5, 2),
                          ([PAIR, PAIR, A], 5), ([A, B] * 3, 1), ([ODD, PAIR, ODD, A, PAIR, A, ODD], 3)):
        assert [idx for idx, _ in plan_passes(shapes, group, odd_alone=False)] == _inline_bucketing(shapes, group), shapes
    # the default is the offline loop's rule: odd frames alone
    assert plan_passes([ODD, ODD], 5) == [([0], False), ([1], False)] == plan_passes([ODD, ODD], 5, odd_alone=True)


# ------------------------------------------------------------------------------------------ the online loop's windows
def _online_windows(n_minibatches, n_epochs, accum, max_window, snapshot_every_n):
    """The windows the online loop forms: (epoch of the last minibatch, length, iterations of the cycle in front, ended at an
    epoch's end) - a replica of the loop's collection around window_closes; a window may cross an epoch's end."""
    from accumulation import window_closes
    out, counter, n = [], 0, 0
    for epoch in range(n_epochs):
        for index in range(n_minibatches):
            n += 1
            end_of_epoch = index == n_minibatches - 1
            if window_closes(n, counter, accum, max_window, end_of_epoch and epoch % snapshot_every_n == snapshot_every_n - 1):
                out.append((epoch, n, counter, end_of_epoch))
                counter = (counter + n) % accum
                n = 0
    return out, n


def test_online_windows_end_with_the_cycle_the_window_length_and_a_snapshot():
    accum, max_window, every, n_mb, n_epochs = 5, 4, 2, 7, 6
    windows, left = _online_windows(n_mb, n_epochs, accum, max_window, every)
    assert sum(n for _, n, _, _ in windows) + left == n_mb * n_epochs
    for epoch, n, counter, at_epoch_end in windows:
        assert 1 <= n <= max_window
        assert counter + n <= accum                      # never across a cycle's end
        closes_cycle = counter + n == accum
        if at_epoch_end and not closes_cycle and n < max_window:
            assert epoch % every == every - 1            # an epoch's end alone ends a window only where a snapshot is due
    # every snapshot epoch's end does end a window ...
    ends = {epoch for epoch, _, _, at_epoch_end in windows if at_epoch_end}
    assert {e for e in range(n_epochs) if e % every == every - 1} <= ends
    # ... and some other epoch's end lies inside one (windows do cross the end of an epoch without a snapshot)
    assert set(range(n_epochs)) - ends
    # the first windows, by hand: 4 + 1 close the cycle; the 2 left of epoch 0 do not end with it (no snapshot) and take the
    # first 2 of epoch 1; in epoch 3 the snapshot alone ends a window of 3 in an open cycle
    assert windows[:5] == [(0, 4, 0, False), (0, 1, 4, False), (1, 4, 0, False), (1, 1, 4, False), (1, 4, 0, True)]
    assert (3, 3, 0, True) in windows


# ------------------------------------------------------------------------------------------ the cycle counter
def test_cycle_counts_passes_that_do_not_divide_it():
    from accumulation import Cycle
    cycle = Cycle(5)
    assert (cycle.counter, cycle.iterations, cycle.passes, cycle.grads_stale) == (0, 0, 0, False)
    seen = []
    for k in (2, 2, 1, 3, 2):
        closes = cycle.closes(k)
        due = cycle.advance(k)
        assert due is closes
        seen.append((due, cycle.counter))
    # 2 + 2 + 1 = 5: the step is due and the counter is 0 again; 3 + 2 = 5 closes the second cycle
    assert seen == [(False, 2), (False, 4), (True, 0), (False, 3), (True, 0)]
    assert cycle.iterations == 10 and cycle.passes == 5
    assert not cycle.closes(4) and cycle.closes(5) and Cycle(1).closes(1)


# ------------------------------------------------------------------------------------------ the module state
class _Module:
    def __init__(self, reserve):
        self.joins = 0
        self.accumulate_grads_in_place = False
        if reserve is not None:
            self.reserve_arena_frames = reserve

    def join_gradients(self):
        self.joins += 1


@pytest.mark.parametrize("defer_join", [True, False])
def test_loop_state_gives_the_module_back_whatever_was_raised(defer_join):
    import dataclasses
    from accumulation import loop_state
    from fosvos_hip.engine import PassFlags
    from fosvos_hip.options import LoopOptions
    net, flags = _Module(reserve=2), PassFlags()
    with pytest.raises(RuntimeError, match="inside"):
        with loop_state(net, flags, LoopOptions(defer_join=defer_join), True, reserve_frames=5):
            assert net.accumulate_grads_in_place is True and net.reserve_arena_frames == 5
            assert flags.defer_wgrad_join is defer_join and flags.compact_stage1 is True
            assert net.joins == (0 if defer_join else 1)     # the join in front of the loop where nothing is deferred
            flags.publish_grad_buckets = flags.forward_one_stream = True   # what the loops set on the way
            raise RuntimeError("inside")
    for field in dataclasses.fields(flags):
        assert getattr(flags, field.name) is False, field.name
    assert net.reserve_arena_frames == 2
    assert net.joins == (1 if defer_join else 2)
    # a module without a reservation gets none, and None leaves one alone
    bare = _Module(reserve=None)
    with loop_state(bare, PassFlags(), LoopOptions(), False, reserve_frames=5):
        assert not hasattr(bare, "reserve_arena_frames")
    with loop_state(net, flags, LoopOptions(), False):
        assert net.reserve_arena_frames == 2 and flags.compact_stage1 is False
    assert net.reserve_arena_frames == 2


def test_gather_reads_the_cast_at_call_time(monkeypatch):
    import torch
    from accumulation import gather
    from util import gpu_handler
    seen = []
    monkeypatch.setattr(gpu_handler, "cast_cuda_if_possible", lambda ts, verbose=False: (seen.append(len(ts)), ts)[1])
    a = {"image": torch.zeros(1, 3, 4, 4), "gt": torch.ones(1, 1, 4, 4)}
    b = {"image": torch.ones(1, 3, 4, 4), "gt": torch.zeros(1, 1, 4, 4)}
    image, gt = gather([a])
    assert image is a["image"] and gt is a["gt"]            # one minibatch: its own tensors, no copy
    image, gt = gather([a, b])
    assert tuple(image.shape) == (2, 3, 4, 4) and torch.equal(image[1:], b["image"]) and torch.equal(gt[:1], a["gt"])
    assert seen == [2, 2]
