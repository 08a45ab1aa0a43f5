"""What train_online._train and train_offline._train share of an accumulation CYCLE (the iterations between two optimizer
steps: constant weights, a gradient that is a sum): its WINDOWS (the consecutive minibatches a loop looks at together), their
PASSES (one forward / loss / backward each), the counting, the plain optimizer step, the module state."""
import contextlib

import torch

from util import gpu_handler


def window_closes(n_window: int, counter_gradient: int, accum: int, max_window: int, boundary: bool) -> bool:
    """Whether the minibatches collected so far (``n_window`` of them, ``counter_gradient`` iterations of the accumulation
    cycle already run in front of them) are run now: a window holds at most ``max_window`` minibatches, never crosses an
    optimizer step and never a ``boundary`` - offline the end of an epoch (the side-loss weight, the epoch log and the snapshot
    change there), online that of an epoch whose snapshot is due.  A CYCLE may straddle either, as in the reference."""
    return ((counter_gradient + n_window) % accum == 0) or n_window >= max_window or boundary


def plan_passes(shapes, group: int, odd_alone: bool = True):
    """The passes of one window.  shapes: the image shapes (N, C, H, W) of its minibatches in draw order.  Returns a list of
    (indices, batched) in the order the passes run: one-frame minibatches are bucketed by shape, buckets in order of first
    appearance and frames in draw order, each bucket cut into passes of at most ``group`` frames (batched = True: the frames
    run concatenated, every frame with the class weights of its own label).  A minibatch that holds several frames is a
    pass of its own at its place (the reference balances its classes over the whole batch tensor): batched = False.  So is,
    with ``odd_alone`` (the offline loop), a frame whose H x W is no multiple of 4: the per-frame loss kernels read 16-byte
    vectors; the online loop's one-map loss takes such frames one call each (ops.cbce_loss_frames) and buckets them.
    The cycle's gradient is a sum over its minibatches, so the order of the passes changes only the order of fp32 additions
    - and a loader that yields the same frames already sorted by shape runs the IDENTICAL passes (tested bit for bit)."""
    buckets = {}
    for i, shape in enumerate(shapes):
        shape = tuple(int(v) for v in shape)
        alone = shape[0] != 1 or (odd_alone and (shape[-2] * shape[-1]) % 4 != 0)
        buckets.setdefault(('alone', i) if alone else shape, []).append(i)
    # (a minibatch that runs alone is a bucket of one index: cut into groups it is what it was)
    return [(idx[j:j + group], key[0] != 'alone') for key, idx in buckets.items() for j in range(0, len(idx), group)]


def gather(items):
    """(image, gt) of one pass over the minibatches ``items``, on the device where there is one."""
    if len(items) == 1:
        inputs, gts = items[0]['image'], items[0]['gt']
    else:
        inputs = torch.cat([m['image'] for m in items])
        gts = torch.cat([m['gt'] for m in items])
    return gpu_handler.cast_cuda_if_possible([inputs, gts])


class Cycle:
    """Where a loop stands in its accumulation cycle of ``length`` iterations: ``counter`` iterations of the open cycle have
    run; ``iterations`` and ``passes`` count the whole `_train` call."""

    def __init__(self, length: int) -> None:
        self.length, self.counter, self.iterations, self.passes = length, 0, 0, 0
        self.grads_stale = False  # the last optimizer step left its gradients in the buffer (LoopOptions.grad_overwrite)

    def closes(self, k: int) -> bool:
        """Whether a pass of ``k`` more iterations is the cycle's last."""
        return (self.counter + k) % self.length == 0

    def advance(self, k: int) -> bool:
        """A pass of ``k`` iterations has been queued; True = the optimizer step is due (the counter is 0 again)."""
        due = self.closes(k)
        self.counter = 0 if due else self.counter + k
        self.iterations += k
        self.passes += 1
        return due


def close_plain(net, sync, optimizer, flat, zero: bool = True) -> None:
    """The optimizer step behind a cycle's last pass, as one step over all parameters."""
    net.join_gradients()
    sync.finish()  # the bucketed all-reduce begun right behind the cycle's last backward pass
    optimizer.step()
    if zero:
        flat.zero()


@contextlib.contextmanager
def loop_state(net, flags, options, compact_stage1: bool, reserve_frames=None):
    """What a loop sets on the module and its engine.PassFlags for the length of its passes; whatever happens inside, the
    caller's module gets back the flags it came with (all off) and its ``reserve_arena_frames`` (read only when a new arena
    is allocated).  reserve_frames: the most frames a pass will hold (never more than a cycle), or None = as it is."""
    reserved = getattr(net, 'reserve_arena_frames', None)
    net.accumulate_grads_in_place = True  # the loops only ever call loss.backward()
    if reserve_frames is not None and reserved is not None:
        net.reserve_arena_frames = reserve_frames
    if not options.defer_join:
        net.join_gradients()
    # weights are constant inside an accumulation cycle: let the next forward overlap the wgrad tail of this backward
    flags.defer_wgrad_join = options.defer_join
    try:
        flags.compact_stage1 = bool(compact_stage1)  # (the loops read nothing of a pass's arena)
        yield
    finally:
        net.join_gradients()
        flags.defer_wgrad_join = False
        flags.publish_grad_buckets = False
        flags.forward_one_stream = False
        flags.compact_stage1 = False
        if reserved is not None:
            net.reserve_arena_frames = reserved
