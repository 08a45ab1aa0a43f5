"""Parent-network (offline) training (reference: src/train_offline.py).

Same entry points and loop semantics (src/train_offline.py:77-110): five deeply-supervised losses,
``loss = (1 - epoch / n_epochs) * sum(side losses) + fused loss``, ``loss /= avg_grad_every_n``,
backward, step every ``avg_grad_every_n``-th iteration; snapshots every ``snapshot_every_n`` epochs.

Opt-in (``--microbatch-group N``, ``_train(..., microbatch_group=N)``): the one-frame minibatches of an accumulation cycle
run as shape-bucketed batched passes of up to N frames, as the online loop's do (accumulation.window_closes / plan_passes).
"""
import timeit
from pathlib import Path
from typing import Optional

import torch
from torch import optim

from config.mypath import Path as P
from fosvos_hip.engine import PassFlags
from fosvos_hip.options import LoopOptions
from layers.osvos_layers import (class_balanced_cross_entropy_loss, class_balanced_cross_entropy_loss_frames_multi,
                                 stage_frames_loss_multi)
from util import gpu_handler, io_helper, experiment_helper, args_helper
from util.logger import get_logger
from util.network_provider import NetworkProvider, provider_mapping
from util.settings import OfflineSettings
import accumulation
import parallel

log = get_logger(__file__)
_hip_cbce = class_balanced_cross_entropy_loss  # tests may rebind the module-level name to a CPU stand-in

save_dir_models = Path('models')
save_dir_results = Path('results')
db_root_dir = None
synthetic_size = None
data_parallel = False
resident_train_set = False
rotate = None               # --augment-rotate (and --rotate-range / --zoom-range / --rotate-renormalize): a RotateOptions
microbatch_group = 1        # --microbatch-group: frames per batched pass of an accumulation cycle (1 = the reference's order)


def train_and_test(net_provider: NetworkProvider, settings: OfflineSettings) -> None:
    io_helper.write_settings(save_dir_models, net_provider.name, settings, variant_offline=settings.variant_offline)
    if settings.is_training:
        net_provider.load_network_train()
        shard = (parallel.rank(), parallel.world_size()) if data_parallel else None
        data_loader_train = io_helper.get_data_loader_train(db_root_dir, settings.batch_size_train,
                                                            synthetic=synthetic_size, shard=shard,
                                                            resident_set=resident_train_set,
                                                            **({} if rotate is None else {'rotate': rotate}))
        data_loader_test = io_helper.get_data_loader_test(db_root_dir, settings.batch_size_test,
                                                          synthetic=synthetic_size)
        optimizer = net_provider.get_optimizer()
        summary_writer = _get_summary_writer()
        _train(net_provider, data_loader_train, data_loader_test, optimizer, summary_writer, settings.start_epoch,
               settings.n_epochs, settings.avg_grad_every_n, settings.snapshot_every_n,
               settings.is_testing_while_training, settings.test_every_n, microbatch_group=microbatch_group)

    if settings.is_testing:
        if not settings.is_training:
            net_provider.load_network_test()
        data_loader = io_helper.get_data_loader_test(db_root_dir, settings.batch_size_test, synthetic=synthetic_size)
        save_dir = io_helper.results_dir(save_dir_results, net_provider.name, 'offline', settings.variant_offline)
        experiment_helper.test(net_provider, data_loader, save_dir, settings.is_visualizing_results,
                               settings.eval_speeds)


def _get_summary_writer():
    return io_helper.get_summary_writer(save_dir_models, comment='-offline')


def _losses(net, minibatch):
    inputs, gts = accumulation.gather([minibatch])
    outputs = net.forward(inputs)
    # Data parallel: this minibatch is one rank's shard of the step's batch.  The reference balances the classes over the
    # whole batch tensor (src/layers/osvos_layers.py:28-39), so the two counts are summed over the ranks first (one
    # 16-byte all-reduce, shared by the five losses); the ranks' losses then add up to the single-process value.
    counts = parallel.batch_label_counts(gts) if data_parallel else None
    return [class_balanced_cross_entropy_loss(o, gts, size_average=False, batch_counts=counts) for o in outputs]


def _losses_frames(outputs, gts, map_scale, ones, staged=None):
    """[k,5] per-frame losses of a batched pass and the seed of its backward pass.  On the GPU one fused op whose kernel writes
    every map's gradient times its map_scale (the seed is then `ones` [>= k, 5], announced and passed through untouched);
    elsewhere (the CPU stand-ins of the tests) the module-level loss per frame and map, seeded with the scales."""
    k = gts.shape[0]
    if gts.is_cuda and class_balanced_cross_entropy_loss is _hip_cbce:
        return class_balanced_cross_entropy_loss_frames_multi(outputs, gts, map_scale, size_average=False,
                                                              backward_seed=(ones, 1.0), staged=staged), ones[:k]
    losses = torch.stack([torch.stack([class_balanced_cross_entropy_loss(o[i:i + 1], gts[i:i + 1], size_average=False)
                                       for o in outputs]) for i in range(k)])
    return losses, torch.tensor(map_scale, dtype=losses.dtype, device=losses.device).expand(k, -1)


def _train(net_provider: NetworkProvider, data_loader_train, data_loader_test, optimizer: optim.SGD, summary_writer,
           start_epoch: int, n_epochs: int, avg_grad_every_n: int, snapshot_every_n: int,
           is_testing_while_training: bool, test_every_n: int, *, options: Optional[LoopOptions] = None,
           microbatch_group: int = 1, compact_stage1: bool = True) -> dict:
    """compact_stage1: the loop's training passes run with PassFlags.compact_stage1 (the same bits either way; False is the
    A/B and test switch).
    options: the loop's switches (fosvos_hip.options.LoopOptions); None = from the environment as it is now.
    microbatch_group: 1 = the reference's loop, one minibatch per pass.  N > 1: the one-frame minibatches of an accumulation
    cycle run as batched passes of up to N frames of one shape (``options.group_window`` minibatches are looked at together;
    ``options.microbatch_group`` is the online loop's and is not read here).  The weights are constant inside a cycle and its
    gradient is a sum, so only the order of fp32 additions changes; every frame keeps the class weights of its own label."""
    if options is None:
        options = LoopOptions.from_env()
    microbatch_group = int(microbatch_group)
    if microbatch_group < 1:
        raise ValueError('microbatch_group must be at least 1, got {}'.format(microbatch_group))
    if microbatch_group > 1 and data_parallel:
        raise ValueError('microbatch_group > 1 with data_parallel: that mode splits every BATCH over the ranks with class '
                         'counts of the whole batch; a grouped pass keeps the counts per frame')
    log.info('Start of offline training')
    net = net_provider.network
    flags = getattr(net, 'pass_flags', None) or PassFlags()  # (a module without the native engine: a throw-away set)
    world = parallel.world_size() if data_parallel else 1
    # Data parallel here splits the BATCH, not the accumulation: every rank runs all
    # avg_grad_every_n iterations of a cycle on its own shard of each iteration's batch (global batch = world x
    # batch_size_train), the class counts of the loss are summed over the ranks per iteration (_losses) and the gradients
    # once per optimizer step - the update of a single process running the whole batch.
    local_accum = avg_grad_every_n
    # gradients live in one flat fp32 buffer: the wgrad kernels accumulate straight into it, zeroing is one memset,
    # and under data parallelism it is the single all-reduce payload
    flat = parallel.FlatGrads.attach_module(net)
    sync = parallel.GradSync(net, flat, options)
    device = next(net.parameters()).device

    n_samples_train = len(data_loader_train)
    loss_train, loss_test, losses_train = [], [], []
    cycle = accumulation.Cycle(local_accum)
    max_window = max(microbatch_group, options.group_window)
    ones = torch.ones((microbatch_group, 5), device=device) if microbatch_group > 1 else None  # seed of a batched backward pass

    def log_epoch(epoch, running, n_images, start_time):
        if world > 1:  # every rank holds its shards' part of the batch losses: the logged value is their sum
            torch.distributed.all_reduce(running, op=torch.distributed.ReduceOp.SUM)
        vals = (running / n_samples_train).tolist()  # one device->host sync per epoch
        loss_train.append(vals[-1])
        losses_train.append(vals)  # all five deeply supervised losses of the epoch
        summary_writer.add_scalar('data/total_loss_epoch', vals[-1], epoch)
        log.info('[Epoch: %d, numImages: %5d]' % (epoch, n_images))
        for l in range(len(vals)):
            log.info('Loss %d: %f' % (l, vals[l]))
        log.info('Execution time: ' + str(timeit.default_timer() - start_time))

    def run_unbatched(minibatch, epoch, running, log_at=None):
        """The reference's pass over one minibatch, class counts over its whole tensor; `running` takes its five losses.
        log_at: (images so far, the epoch's start time) where the epoch's log goes between the loss and the backward pass."""
        losses = _losses(net, minibatch)
        running += torch.stack([l.detach() for l in losses])
        loss = (1 - epoch / n_epochs) * sum(losses[:-1]) + losses[-1]
        if log_at is not None:
            log_epoch(epoch, running, *log_at)
        # `loss /= nAveGrad; loss.backward()` of the reference, as a backward pass seeded with 1/nAveGrad (same
        # gradient, three fewer tiny kernels: see train_online._train)
        last_of_cycle = world > 1 and cycle.closes(1)
        if last_of_cycle:
            sync.arm()
        loss.backward(torch.full_like(loss.detach(), 1.0 / avg_grad_every_n))
        if last_of_cycle:
            sync.begin()
        if cycle.advance(1):
            accumulation.close_plain(net, sync, optimizer, flat)

    def run_window(window, epoch, running):
        """The minibatches of `window` (inside one accumulation cycle and one epoch, draw order) as the passes of
        accumulation.plan_passes; `running` takes the five loss sums of every frame."""
        w = 1 - epoch / n_epochs
        map_scale = [w / avg_grad_every_n] * 4 + [1.0 / avg_grad_every_n]
        for idx, batched in accumulation.plan_passes([mb['image'].shape for mb in window], microbatch_group):
            if not batched:
                run_unbatched(window[idx[0]], epoch, running)
                continue
            inputs, gts = accumulation.gather([window[i] for i in idx])
            # the loss in three places, as in the online loop: the class counts in front of the forward pass (they need
            # no logits), ONE launch for the five maps' gradients between the passes, the values behind the backward pass
            staged = None
            if options.stage_loss and gts.is_cuda and class_balanced_cross_entropy_loss is _hip_cbce:
                staged = stage_frames_loss_multi(gts.contiguous().float(), 5)
                if staged is not None:
                    gts = staged.label
            outputs = net.forward(inputs)
            losses, seed = _losses_frames(outputs, gts, map_scale, ones, staged)
            losses.backward(seed)
            if staged is not None:
                staged.finish()
            running += losses.detach().sum(0)  # (queued behind finish(): no host sync)
            if cycle.advance(len(idx)):
                accumulation.close_plain(net, sync, optimizer, flat)

    time_all_start = timeit.default_timer()
    with accumulation.loop_state(net, flags, options, compact_stage1,
                                 min(microbatch_group, avg_grad_every_n) if microbatch_group > 1 else None):
        for epoch in range(start_epoch, n_epochs):
            start_time = timeit.default_timer()
            # a DistributedSampler (data-parallel loader) draws the same permutation every epoch unless it is told the
            # epoch; the reference's shuffle=True loader draws a new order per epoch (src/util/io_helper.py:62-70)
            sampler = getattr(data_loader_train, 'sampler', None)
            if hasattr(sampler, 'set_epoch'):
                sampler.set_epoch(epoch)
            running = torch.zeros(5, device=device)
            window = []
            for index, minibatch in enumerate(data_loader_train):
                end_of_epoch = index % n_samples_train == n_samples_train - 1
                if microbatch_group == 1:
                    # the epoch's log in front of its last backward pass: the one .tolist() sync per epoch lands while that
                    # pass and the optimizer step are still to be queued
                    run_unbatched(minibatch, epoch, running, (index + 1, start_time) if end_of_epoch else None)
                    continue
                window.append(minibatch)
                if accumulation.window_closes(len(window), cycle.counter, local_accum, max_window, end_of_epoch):
                    run_window(window, epoch, running)
                    window = []
                if end_of_epoch:
                    log_epoch(epoch, running, index + 1, start_time)
            if window:  # (a loader that ended before its own length)
                run_window(window, epoch, running)

            if (epoch % snapshot_every_n) == snapshot_every_n - 1 and epoch != 0 and parallel.rank() == 0:
                net_provider.save_model(epoch)

            if is_testing_while_training and epoch % test_every_n == (test_every_n - 1):
                with torch.no_grad():
                    running_t = torch.zeros(5, device=device)
                    for index, minibatch in enumerate(data_loader_test):
                        running_t += torch.stack(_losses(net, minibatch))
                    vals = (running_t / max(len(data_loader_test), 1)).tolist()
                loss_test.append(vals[-1])
                summary_writer.add_scalar('data/test_loss_epoch', vals[-1], epoch)
                for l in range(len(vals)):
                    log.info('***Testing *** Loss %d: %f' % (l, vals[l]))
        summary_writer.close()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return {'loss_train': loss_train, 'loss_test': loss_test, 'losses_train': losses_train, 'iterations': cycle.iterations,
            'passes': cycle.passes, 'seconds': timeit.default_timer() - time_all_start}


def main(argv=None):
    global db_root_dir, synthetic_size, data_parallel, resident_train_set, microbatch_group, rotate
    args = args_helper.parse_args(is_online=False, argv=argv)
    if args.network != 'vgg16':
        raise SystemExit('only --network vgg16 is implemented on the HIP path (ResNet family: SURVEY.md §8 f4)')
    data_parallel = bool(args.data_parallel) and parallel.init_distributed()
    gpu_handler.select_gpu(args.gpu_id)
    db_root_dir = P.db_root_dir()
    synthetic_size = (args.height, args.width) if args.synthetic else None
    resident_train_set = bool(args.resident_train_set)
    microbatch_group = args.microbatch_group
    rotate = args.rotate
    save_dir_models.mkdir(parents=True, exist_ok=True)
    save_dir_results.mkdir(parents=True, exist_ok=True)

    settings = OfflineSettings(is_training=args.is_training, is_testing=args.is_testing, start_epoch=0,
                               n_epochs=args.n_epochs or 240, avg_grad_every_n=args.avg_grad_every_n or 10,
                               snapshot_every_n=40, is_testing_while_training=False, test_every_n=5,
                               batch_size_train=1, batch_size_test=1, is_visualizing_network=False,
                               is_visualizing_results=False, is_loading_vgg_caffe=False,
                               variant_offline=args.variant_offline, eval_speeds=args.eval_speeds)
    provider_class = provider_mapping[('offline', args.network)]
    net_provider = provider_class(args.network, save_dir_models, settings, variant_offline=args.variant_offline)
    if args.synthetic:
        # no ImageNet weights offline (pretrained=1 needs torchvision + network): start from the reference's
        # random init instead and say so
        log.warning('--synthetic: starting from OSVOS_VGG(pretrained=0) random init')
        net_provider.load_network_train = lambda: net_provider.init_network(pretrained=0)
    train_and_test(net_provider, settings)


if __name__ == '__main__':
    main()
