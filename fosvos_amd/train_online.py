"""One-shot online fine-tuning (reference: src/train_online.py).

Same entry points - ``train_and_test(net_provider, seq_name, settings)`` and ``_train(...)`` with the
reference's positional arguments - and the same loop semantics (src/train_online.py:70-107): forward,
class-balanced BCE on ``outputs[-1]`` with ``size_average=False``, ``loss /= avg_grad_every_n``,
backward, ``optimizer.step(); optimizer.zero_grad()`` every ``avg_grad_every_n``-th iteration.  The
arithmetic runs on the HIP kernels; the loss is accumulated on the device and only read back at the
reference's logging points, so the loop does not synchronise every iteration.

Run:  python train_online.py --synthetic --n-epochs 100        (one GPU)
      torchrun --nproc-per-node 8 train_online.py --synthetic --data-parallel --avg-grad-every-n 8
      python train_online.py --synthetic --multi-object --objects 3 --score   (one net per object: train_and_test_objects)
      python train_online.py --synthetic --adapt-steps 1 --score    (online adaptation in the test pass: test_adaptive)
"""
import timeit
from pathlib import Path
from typing import Optional

import numpy as np
import torch
from torch import optim

from config.mypath import Path as P
from fosvos_hip.engine import PassFlags
from fosvos_hip.options import LoopOptions
from layers.osvos_layers import class_balanced_cross_entropy_loss, class_balanced_cross_entropy_loss_frames, stage_frames_loss
from util import gpu_handler, io_helper, experiment_helper, args_helper
from util.logger import get_logger
from util.network_provider import NetworkProvider, provider_mapping
from util.settings import OnlineSettings
import accumulation
import parallel

log = get_logger(__file__)
_hip_cbce = class_balanced_cross_entropy_loss  # tests may rebind the module-level name to a CPU stand-in

# run-wide locations; the reference keeps these as module globals set in __main__
save_dir_models = Path('models')
save_dir_results = Path('results')
path_stem = 'vgg16/online'
db_root_dir = None
synthetic_size = None       # (H, W) when --synthetic
data_parallel = False
score = False               # --score: the test pass computes J and F on the device (experiment_helper.test_scored)
fast_test = False           # --fast-test: grouped forward passes, PNG files encoded on the device (experiment_helper.test_fast)
png_fitted = False          # --png-fitted (with --fast-test): Huffman codes fitted to each segment of the PNG files
device_decode = False       # --device-decode: the test pass's JPEG frames are decoded on the device (dataloaders/device_decode.py)
multi_object = False        # --multi-object: one net per object, merged and scored on the device (train_and_test_objects)
clean = None                # --clean-min-area / --clean-largest / --clean-temporal (with --fast-test): a CleanOptions
rotate = None               # --augment-rotate (and its options): a RotateOptions; the one-shot loaders rotate and zoom the sample
lucid = None                # --augment-lucid (and --lucid-*): a LucidOptions; the one-shot loaders move the object against its background
adapt = None                # --adapt-steps (and --adapt-*): an AdaptOptions; the test pass is experiment_helper.test_adaptive
ensemble = None             # --ensemble-flip / --ensemble-scales (with --fast-test or --multi-object): an EnsembleOptions
crf = None                  # --crf (and --crf-*; with --fast-test or --multi-object): a CrfOptions
crf_joint = False           # --crf-joint (with --crf and --multi-object): ONE joint CRF over the labels in test_objects
motion = None               # --clean-motion (and --motion-*; with --clean-temporal): a MotionOptions
synthetic_objects = 2       # --objects: the objects of the synthetic sequence under --multi-object
scored_sequences = []       # the score of every sequence of this run, in order

sequences_val = ['blackswan', 'bmx-trees', 'breakdance', 'camel', 'car-roundabout', 'car-shadow', 'cows',
                 'dance-twirl', 'dog', 'drift-chicane', 'drift-straight', 'goat', 'horsejump-high', 'kite-surf',
                 'libby', 'motocross-jump', 'paragliding-launch', 'parkour', 'scooter-black', 'soapbox']


def _train_annotation(data_loader) -> Optional[np.ndarray]:
    """``gt >= 0.5`` of the one-shot training sample at the frame's own size (uint8 [H,W]), or None where the loader does
    not hold exactly one untransformed sample."""
    dataset = getattr(data_loader, 'dataset', None)
    if dataset is None or len(dataset) != 1 or getattr(dataset, 'transform', None) is not None:
        return None
    gt = np.squeeze(np.asarray(dataset[0]['gt'], dtype=np.float32))
    return (gt >= 0.5).astype(np.uint8) if gt.ndim == 2 else None


def _clean_seed(train_seed, annotations, data_loader, seq_name: str) -> Optional[np.ndarray]:
    """The first seed of --clean-temporal: the training sample's annotation when this call trained, else the first test
    frame's annotation when --score gives one, else None."""
    if train_seed is not None:
        return train_seed
    if annotations is not None and len(data_loader.dataset):
        first = data_loader.dataset[0]
        ann = annotations(first.get('seq_name', seq_name), first['fname'])
        if ann is not None:
            return (np.asarray(ann) != 0).astype(np.uint8)
    log.info('Clean {0}: no annotation to start the temporal gate from, the first frame is not gated'.format(seq_name))
    return None


def _augment_kwargs() -> dict:
    """``rotate`` / ``lucid`` for a training loader, each passed only when set (absent: the call is what it was)."""
    return {name: v for name, v in (('rotate', rotate), ('lucid', lucid)) if v is not None}


def _train_loader(seq_name: str, settings: OnlineSettings):
    """The training loader of a sequence run."""
    return io_helper.get_data_loader_train(db_root_dir, settings.batch_size_train, seq_name, synthetic=synthetic_size,
                                           **_augment_kwargs())


def _first_sample(data_loader) -> dict:
    """The one-shot training frame as it is, neither flipped nor rescaled: ``image`` [1,3,H,W] and ``gt`` [1,1,H,W], what
    online adaptation keeps training on beside each new frame."""
    variants = getattr(data_loader, 'variants', None)
    if variants is not None and 1 in list(data_loader.scales):  # the resident loader: its unflipped variant at scale 1
        sample = variants[(False, list(data_loader.scales).index(1))]
        return {'image': sample['image'], 'gt': sample['gt']}
    dataset = data_loader.dataset
    if len(dataset) < 1:
        raise ValueError('online adaptation needs the training frame: the training loader is empty')
    if getattr(dataset, 'transform', None) is None:
        sample = dataset[0]
        if not torch.is_tensor(sample['image']):
            from dataloaders import custom_transforms
            sample = custom_transforms.ToTensor()(sample)
        return {'image': sample['image'][None], 'gt': sample['gt'][None]}
    raise ValueError('online adaptation needs the training frame as it is; this training loader only yields augmented ones')


def _report_score(result: Optional[dict], save_dir: Path, seq_name: str) -> None:
    """A sequence's score (None: the pass had no annotations, nothing happens) goes to the log, to
    ``<save_dir>/<seq_name>/scores.yml`` and into ``scored_sequences``."""
    if result is None:
        return
    log.info('Score {0}: {1}'.format(seq_name, experiment_helper.format_score(result)))
    (Path(save_dir) / seq_name).mkdir(parents=True, exist_ok=True)
    experiment_helper.write_scores(Path(save_dir) / seq_name / 'scores.yml', result)
    scored_sequences.append(result)


def _log_mean_score(scored, over: str) -> None:
    """The run's mean J and F over ``scored`` (each with 'J_stats' and 'F_stats'), as one log line."""
    j_mean = sum(r['J_stats']['mean'] for r in scored) / len(scored)
    f_mean = sum(r['F_stats']['mean'] for r in scored) / len(scored)
    log.info('Score over {0}: J mean {1:.4f}, F mean {2:.4f}, J&F {3:.4f}'.format(over, j_mean, f_mean, (j_mean + f_mean) / 2))


def train_and_test(net_provider: NetworkProvider, seq_name: str, settings: OnlineSettings) -> None:
    train_seed = None
    first_sample = None
    io_helper.write_settings(save_dir_models, net_provider.name, settings, variant_offline=settings.variant_offline,
                             variant_online=settings.variant_online)
    summary_writer = _get_summary_writer(path_stem)

    if settings.is_training:
        net_provider.load_network_train()
        data_loader = _train_loader(seq_name, settings)
        optimizer = net_provider.get_optimizer()
        _train(net_provider, data_loader, optimizer, summary_writer, seq_name, settings.start_epoch, settings.n_epochs,
               settings.avg_grad_every_n, settings.snapshot_every_n)
        if clean is not None and clean.chain:
            train_seed = _train_annotation(data_loader)
        if adapt is not None:
            first_sample = _first_sample(data_loader)

    if settings.is_testing:
        if not settings.is_training:
            net_provider.load_network_test(sequence=seq_name)
        data_loader = io_helper.get_data_loader_test(db_root_dir, settings.batch_size_test, seq_name,
                                                     synthetic=synthetic_size, device_decode=device_decode)
        save_dir = io_helper.results_dir(save_dir_results, net_provider.name, 'online', settings.variant_offline,
                                         settings.variant_online)
        if adapt is not None:
            if first_sample is None:  # this call did not train: the training loader still holds the annotated frame
                first_sample = _first_sample(_train_loader(seq_name, settings))
            annotations = io_helper.get_annotations(db_root_dir, data_loader, synthetic_size) if score else None
            result = experiment_helper.test_adaptive(net_provider, data_loader, save_dir, first_sample, adapt, annotations,
                                                     seq_name=seq_name, png_huffman='fitted' if png_fitted else 'fixed')
            _report_score(result, save_dir, seq_name)
            return
        if fast_test:
            annotations = io_helper.get_annotations(db_root_dir, data_loader, synthetic_size) if score else None
            cleaning = {}
            if clean is not None:  # (absent: the call is what it was)
                cleaning['clean'] = clean
                if clean.chain:
                    cleaning['clean_seed'] = _clean_seed(train_seed, annotations, data_loader, seq_name)
            if ensemble is not None:  # (absent: the call is what it was)
                cleaning['ensemble'] = ensemble
            if crf is not None:  # (absent: the call is what it was)
                cleaning['crf'] = crf
            if motion is not None:  # (absent: the call is what it was)
                cleaning['motion'] = motion
            result = experiment_helper.test_fast(net_provider, data_loader, save_dir, annotations, seq_name=seq_name,
                                                 png_huffman='fitted' if png_fitted else 'fixed', **cleaning)
            _report_score(result, save_dir, seq_name)
            return
        if score:
            result = experiment_helper.test_scored(net_provider, data_loader, save_dir,
                                                   io_helper.get_annotations(db_root_dir, data_loader, synthetic_size),
                                                   seq_name=seq_name)
            _report_score(result, save_dir, seq_name)
            return
        experiment_helper.test(net_provider, data_loader, save_dir, settings.is_visualizing_results,
                               settings.eval_speeds, seq_name=seq_name)


def _object_loaders(seq_name: str, object_id: int, settings: OnlineSettings, n_objects: int):
    """(train loader, test loader or None, annotations) of one object of a multi-object sequence."""
    if synthetic_size is not None:
        from dataloaders.synthetic import SyntheticObjectsSequence
        from torch.utils.data import DataLoader
        h, w = synthetic_size
        train = DataLoader(SyntheticObjectsSequence(seq_name, h, w, n_frames=1, n_objects=n_objects, object_id=object_id),
                           batch_size=settings.batch_size_train, shuffle=True, num_workers=0)
        test = DataLoader(SyntheticObjectsSequence(seq_name, h, w, n_frames=4, n_objects=n_objects),
                          batch_size=settings.batch_size_test, shuffle=False, num_workers=0)
        return train, test, test.dataset.annotation
    from dataloaders import custom_transforms
    from dataloaders.davis_2017 import DAVIS2017, Davis2017Annotations
    from dataloaders.resident import ResidentOneShotLoader
    from torch.utils.data import DataLoader
    train = ResidentOneShotLoader(DAVIS2017(mode='train', db_root_dir=str(db_root_dir), seq_name=seq_name,
                                            object_id=object_id, transform=None),
                                  **_augment_kwargs())
    test = DataLoader(DAVIS2017(mode='test', db_root_dir=str(db_root_dir), seq_name=seq_name, object_id=object_id,
                                transform=custom_transforms.ToTensor()),
                      batch_size=settings.batch_size_test, shuffle=False, num_workers=2)
    return train, test, Davis2017Annotations(db_root_dir)


def train_and_test_objects(make_provider, seq_name: str, settings: OnlineSettings) -> Optional[dict]:
    """A sequence of K objects: for k = 1..K a fresh provider (``make_provider()``) loads the parent weights and `_train`
    fine-tunes it on object k against everything else, snapshots named ``<seq>_<k>`` through the provider's ``sequence``
    argument; the K nets stay on the device and ``experiment_helper.test_objects`` runs them all on every frame.  The train
    loop itself is `_train`, untouched."""
    if synthetic_size is not None:
        n_objects = synthetic_objects
    else:
        from dataloaders.davis_2017 import n_objects as count_objects
        n_objects = count_objects(db_root_dir, seq_name)
    if not 1 <= n_objects <= 16:
        raise SystemExit('sequence {}: {} objects, outside [1, 16]'.format(seq_name, n_objects))
    summary_writer = _get_summary_writer(path_stem)
    providers, test_loader, annotations = [], None, None
    for k in range(1, n_objects + 1):
        provider = make_provider()
        io_helper.write_settings(save_dir_models, provider.name, settings, variant_offline=settings.variant_offline,
                                 variant_online=settings.variant_online)
        train_loader, test_loader, annotations = _object_loaders(seq_name, k, settings, n_objects)
        name_k = '{0}_{1}'.format(seq_name, k)
        if settings.is_training:
            provider.load_network_train()
            _train(provider, train_loader, provider.get_optimizer(), summary_writer, name_k, settings.start_epoch,
                   settings.n_epochs, settings.avg_grad_every_n, settings.snapshot_every_n)
        elif settings.is_testing:
            provider.load_network_test(sequence=name_k)
        providers.append(provider)
    if not settings.is_testing:
        return None
    save_dir = io_helper.results_dir(save_dir_results, providers[0].name, 'online', settings.variant_offline,
                                     settings.variant_online)
    result = experiment_helper.test_objects(providers, test_loader, save_dir, annotations if score else None,
                                            seq_name=seq_name, png_huffman='fitted' if png_fitted else 'fixed',
                                            **({} if ensemble is None else {'ensemble': ensemble}),
                                            **({} if crf is None else {'crf': crf}),
                                            **({'crf_joint': True} if crf_joint else {}))
    _report_score(result, save_dir, seq_name)
    return result


def _losses_per_frame(fused, gts, backward_seed=None, staged=None):
    """[k] per-frame losses of a batched pass; one fused op on the GPU, the reference's function per slice elsewhere.
    staged: the loss was started beside the forward pass (osvos_layers.stage_frames_loss): its values are written by
    staged.finish(), which the caller queues behind the backward pass."""
    if fused.is_cuda and class_balanced_cross_entropy_loss is _hip_cbce:
        return class_balanced_cross_entropy_loss_frames(fused, gts, size_average=False, backward_seed=backward_seed,
                                                        staged=staged)
    return torch.stack([class_balanced_cross_entropy_loss(fused[i:i + 1], gts[i:i + 1], size_average=False)
                        for i in range(fused.shape[0])])


class _Landed:
    """Stand-in for a recorded CUDA event when the loop runs on CPU tensors."""

    def query(self):
        return True

    def synchronize(self):
        pass


class _LossLog:
    """The loss log of one `_train` call.  The reference reads loss.item() every iteration and the running loss at 20 logging
    points per run (device->host syncs that drain the launch queue).  Here every pass sends its per-frame losses to pinned
    memory with ONE asynchronous copy and the host does the bookkeeping (running sum, logging points) once the copy has
    landed: no device-side accumulator kernels, no sync.  `loss_tr` fills in iteration order, a few passes behind the device.

    ring: pinned [slots, frames per pass] fp32 host tensor, or None for CPU tensors.  (Every slot is free at construction:
    the previous call ended with a device sync.)"""

    def __init__(self, ring, n_samples: int, log_every: int, seq_name: str, summary_writer) -> None:
        self.ring = ring
        self.ring_free = list(range(ring.shape[0])) if ring is not None else []
        self.n_samples, self.log_every, self.seq_name, self.summary_writer = n_samples, log_every, seq_name, summary_writer
        self.loss_tr = []
        self.running_host = 0.0
        self.pending = []  # per window: ([(epoch, minibatch index, host tensor, position)] in iteration order, events, ring slots)
        self.window = []   # (frames, host tensor, event, ring slot) of the passes of the window being run

    def flush(self, block: bool) -> None:
        while self.pending:
            items, landed, slots = self.pending[0]
            # every pass's copy has its own event: the passes of a window alternate between two streams, so the last
            # event alone says nothing about the copies queued on the other stream
            if block:
                for ev in landed:
                    ev.synchronize()
            elif not all(ev.query() for ev in landed):
                break
            self.pending.pop(0)
            for ep, mb, host_vals, i in items:  # iteration order of the reference's loop, whatever order the passes ran in
                self.running_host += float(host_vals[i])
                if ep % self.log_every == self.log_every - 1:
                    value = self.running_host / self.n_samples
                    self.running_host = 0.0
                    self.loss_tr.append(value)
                    log.info('[Epoch {0}: {1}, numImages: {2}]'.format(self.seq_name, ep + 1, mb + 1))
                    log.info('Loss {0}: {1}'.format(self.seq_name, value))
                    self.summary_writer.add_scalar('data/total_loss_epoch', value, ep)
            self.ring_free.extend(slots)

    def record(self, group, losses) -> None:
        """losses: [k] detached device tensor, frame by frame in the order of `group`."""
        frames = [(g[0], g[1]) for g in group]
        if self.ring is not None:
            if not self.ring_free:
                self.flush(True)
            if not self.ring_free:  # every slot is held by the window in flight: a plain (pageable, synchronous) copy instead
                self.window.append((frames, losses.to('cpu'), _Landed(), None))
                return
            slot = self.ring_free.pop()
            host_vals = self.ring[slot, :len(frames)]
            host_vals.copy_(losses, non_blocking=True)
            landed = torch.cuda.Event()
            landed.record()
        else:  # CPU tensors (the gloo tests of the data-parallel wiring): nothing to wait for
            slot, host_vals, landed = None, losses.clone(), _Landed()
        self.window.append((frames, host_vals, landed, slot))

    def close_window(self) -> None:
        """The passes of a window ran bucket by bucket; the bookkeeping (running loss, logging points) follows the
        reference's iteration order: one pending entry per window, sorted, waiting on the copies of ALL its passes."""
        if not self.window:
            return
        items = sorted(((ep, mb, host_vals, i) for frames, host_vals, _, _ in self.window
                        for i, (ep, mb) in enumerate(frames)), key=lambda t: (t[0], t[1]))
        slots = [slot for _, _, _, slot in self.window if slot is not None]
        self.pending.append((items, [landed for _, _, landed, _ in self.window], slots))
        self.window.clear()
        self.flush(False)


class _PassStreams:
    """The second stream (``side``, or None) of a cycle whose passes alternate between two (LoopOptions.pass_streams)."""

    def __init__(self, side, device) -> None:
        self.side, self.device = side, device
        self.used = False          # a pass of the current cycle ran on the side stream: the optimizer step waits for it
        self.last_on_side = False  # ... and it was the most recent pass

    def pick(self, i: int, n: int, multi: bool):
        """The stream of pass i of n of a window (None = the caller's).  The window's LAST pass (the one that may close the
        cycle) always runs on the caller's: the split optimizer step is queued there, behind that pass's data-gradient chain."""
        self.last_on_side = multi and (n - 1 - i) % 2 == 1
        self.used = self.used or self.last_on_side
        return self.side if self.last_on_side else None

    def wait(self) -> None:
        """The caller's stream waits for the passes of this cycle that ran on the second pass stream.  (The EARLY part of a
        split optimizer step does not need this for the EARLIER passes: the weight-gradient kernels of all passes share one
        stream, in order, and a pass's last weight-gradient kernels wait for the end of its data-gradient chain, so the
        bucket events of the cycle's last pass also say that every earlier pass has left the stages they cover.  The closing
        pass's OWN data-gradient chain is not covered by its bucket events - a stage's event is recorded behind the weight
        gradient of the stage's first conv, which is issued in front of that conv's data gradient - so the closing pass runs
        on the caller's stream, where the step queues behind it; see pick and _train's close_cycle.)"""
        if self.used:
            torch.cuda.current_stream(self.device).wait_stream(self.side)
            self.used = False


def _get_summary_writer(seq_name: str):
    return io_helper.get_summary_writer(Path('tensorboard') / path_stem)


def _train(net_provider: NetworkProvider, dataloader, optimizer: optim.SGD, summary_writer, seq_name: str,
           start_epoch: int, n_epochs: int, avg_grad_every_n: int, snapshot_every_n: int, *,
           options: Optional[LoopOptions] = None, compact_stage1: bool = True) -> dict:
    """options: the loop's switches (fosvos_hip.options.LoopOptions, where each is explained); None = from the environment
    as it is now.  compact_stage1: the loop's passes run with PassFlags.compact_stage1 (conv1_2 stores the pool's winner
    codes instead of its output; the same bits either way - False is the A/B and test switch)."""
    if options is None:
        options = LoopOptions.from_env()
    log.info('Start of Online Training, sequence: ' + seq_name)
    net = net_provider.network
    # the flags the passes read (engine.PassFlags): the module's own, or - a module that does not run on the native engine,
    # like the CPU stand-in of the data-parallel tests - a throw-away set nobody reads
    flags = getattr(net, 'pass_flags', None)
    native = flags is not None and all(callable(getattr(net, f, None)) for f in ('wait_grad_bucket', 'join_gradients'))
    if flags is None:
        flags = PassFlags()
    world = parallel.world_size() if data_parallel else 1
    dp_on = data_parallel and parallel.collectives_on()  # (world > 1, or the single-rank test hook)
    local_accum = parallel.split_accumulation(avg_grad_every_n, world)
    # gradients live in one flat fp32 buffer: the wgrad kernels accumulate straight into it, zeroing is one memset,
    # and under data parallelism it is the single all-reduce payload
    flat = parallel.FlatGrads.attach_module(net)
    sync = parallel.GradSync(net, flat, options)
    on_gpu = flat.flat.is_cuda and native

    # on the GPU the optimizer step is split by gradient bucket (see close_cycle; LoopOptions.split_step)
    # (slice indices of the flat buffer; flat.bucket_ids maps a slice to the native bucket its gradients are published as)
    early_buckets = [b for b, bid in enumerate(flat.bucket_ids) if bid < parallel.VGG_EARLY_BUCKETS]
    late_buckets = [b for b in range(len(flat.slices)) if b not in early_buckets]
    split_step = (on_gpu and bool(early_buckets) and bool(late_buckets)
                  and getattr(net, 'publishes_grad_buckets', True)  # the native backward pass records the bucket events
                  and hasattr(optimizer, '_tables') and options.split_step)
    early_params = [p for b in early_buckets for p in flat.bucket_params[b]]
    early_ids = {id(p) for p in early_params}
    late_params = [p for group in optimizer.param_groups for p in group['params'] if id(p) not in early_ids]
    early_prefixes = tuple(pre for b in early_buckets for pre in parallel.VGG_BUCKETS[flat.bucket_ids[b]])

    lazy_zero = on_gpu and options.grad_overwrite  # gradient buffers without zeroing (LoopOptions.grad_overwrite)
    side_stream = None  # a cycle of several passes on two alternating streams (LoopOptions.pass_streams)
    if flat.flat.is_cuda:
        from fosvos_hip import engine as _engine
        dev_index = flat.flat.device.index if flat.flat.device.index is not None else torch.cuda.current_device()
        # the library's auxiliary streams exist from here on, in their fixed creation order (engine.shared_stream)
        _engine.shared_stream(dev_index, "comm")
        if native and options.defer_join and options.pass_streams:
            side_stream = _engine.shared_stream(dev_index, "pass")
    device = next(net.parameters()).device
    streams = _PassStreams(side_stream, device)
    cycle = accumulation.Cycle(local_accum)
    log_every = max(n_epochs // 20, 1)  # the reference divides by n_epochs // 20, which is 0 below 20 epochs
    max_group = options.microbatch_group
    max_window = max(max_group, options.group_window)
    consts = flat.cache.get(('online', avg_grad_every_n, max_group, str(device)))
    if consts is None:  # (constants of the loop, kept with the gradient buffer: a short call should not re-create them)
        consts = flat.cache[('online', avg_grad_every_n, max_group, str(device))] = {
            'inv_avg': torch.ones((), device=device) / avg_grad_every_n,
            'inv_avg_k': torch.full((max_group,), 1.0 / avg_grad_every_n, device=device),  # backward seed of a batched pass
            'ring': torch.empty((64, max_group), dtype=torch.float32).pin_memory() if device.type == 'cuda' else None}
    inv_avg, inv_avg_k = consts['inv_avg'], consts['inv_avg_k']
    loss_log = _LossLog(consts['ring'], len(dataloader), log_every, seq_name, summary_writer)

    def run_pass(group) -> None:
        """One forward / loss / backward pass, on the current stream, over the micro-batches of `group` (iterations of the
        reference's loop with the same frame size, inside one accumulation cycle; consecutive or not - see run_window).  The
        weights do not change inside a cycle, so running k iterations as one batch of k frames leaves every frame's logits,
        loss (the class weights are still counted per frame) and gradient contribution what the one-by-one loop computes; only
        the order of the fp32 sums over frames differs.  What it buys on the GPU: k frames per kernel launch (the small stage-5
        layers fill the chip without split-K, fewer launch gaps) and one set of weight-gradient partial slabs per group
        instead of per frame."""
        k = len(group)
        inputs, gts = accumulation.gather([g[2] for g in group])

        # A batched pass spreads its loss over three places (LoopOptions.stage_loss): the class counts of the labels are taken
        # here, in front of the forward pass (they need no logits), the loss kernel proper sits between the passes, and the
        # loss VALUES - which only the log reads - are finished and copied to the host behind the backward pass.  Between the
        # passes the whole chip waits on a chain of small kernels: this takes two of them and the copy out of that chain.
        staged = None
        if k > 1 and options.stage_loss and gts.is_cuda and class_balanced_cross_entropy_loss is _hip_cbce:
            staged = stage_frames_loss(gts)

        outputs = net.forward(inputs)

        # (the seed of the backward pass below is announced to the loss: its kernel writes the gradient times 1 / nAveGrad
        # and the loss's own backward has nothing left to multiply)
        seeded = outputs[-1].is_cuda and class_balanced_cross_entropy_loss is _hip_cbce
        if k == 1:
            loss = (class_balanced_cross_entropy_loss(outputs[-1], gts, size_average=False,
                                                      backward_seed=(inv_avg, 1.0 / avg_grad_every_n))
                    if seeded else class_balanced_cross_entropy_loss(outputs[-1], gts, size_average=False))
            losses = loss.detach().reshape(1)
        else:
            # [k]; the sum over frames is taken by the backward seed
            loss = _losses_per_frame(outputs[-1], gts, (inv_avg_k, 1.0 / avg_grad_every_n) if seeded else None, staged)
            losses = loss.detach()
        if staged is None:
            loss_log.record(group, losses)

        # reference: `loss /= nAveGrad; loss.backward()` (src/train_online.py:92-93).  Seeding the backward pass with
        # 1/nAveGrad is the same gradient (the division's own backward produces exactly this factor) without the
        # three tiny kernels of the division, the ones-fill and its backward on the critical path
        closes_cycle = cycle.closes(k)
        last_of_cycle = dp_on and closes_cycle
        flags.last_pass_of_cycle = closes_cycle
        if last_of_cycle:
            sync.arm()
        if split_step and closes_cycle:
            flags.publish_grad_buckets = True
        loss.backward(inv_avg if k == 1 else inv_avg_k[:k])
        if last_of_cycle:
            sync.begin()
        if staged is not None:
            # the loss VALUES: one small kernel and the copy to the host, behind the backward pass.  (Queued on the
            # communication stream instead, behind an event, they cost 0.6 % - a third stream with work in flight - where on
            # this stream they cost nothing measurable: profiles/r04_lab_step_ab_head_loss.txt.)
            staged.finish()
            loss_log.record(group, losses)
        # (the reference also sums loss.item() into a per-epoch tensorboard scalar, src/train_online.py:94-104: one
        # device sync per frame; the per-pass asynchronous copy above carries the same information without it)

    def close_cycle() -> None:
        """The optimizer step behind the cycle's last pass, on the caller's stream."""
        if split_step:
            # Stages 5-3 hold 97 % of the parameters and their gradients are final well before the backward pass ends.
            # Their share of the optimizer step, the zeroing of their gradients and the repacking of their weights are
            # queued on the main stream right here - behind the data-gradient chain, while the weight-gradient stream
            # is still working through stages 3-1 - and only the small rest waits for that stream.
            # Data parallel: "final" means all-reduced - the early buckets' collectives were begun while the backward pass
            # was still running, and each is waited for on its own.
            flags.publish_grad_buckets = False
            if streams.last_on_side:
                # (_PassStreams.pick schedules a window's last pass on the caller's stream, so this is a guard: the early step
                # rewrites and repacks weights the closing pass's data-gradient chain on the other stream still reads)
                streams.wait()
            for b in early_buckets:
                if dp_on:
                    sync.wait_bucket(b)
                else:
                    net.wait_grad_bucket(flat.bucket_ids[b])
            optimizer.step(only=early_params, tag='early', zero_grad=not lazy_zero)  # (the step kernel zeroes what it read)
            net.prepack_weights(early_prefixes)
            streams.wait()
            net.join_gradients()
            sync.finish()
            optimizer.step(only=late_params, tag='late', zero_grad=not lazy_zero)
        else:
            streams.wait()
            accumulation.close_plain(net, sync, optimizer, flat, zero=not lazy_zero)
        cycle.grads_stale = lazy_zero

    def run_window(window) -> None:
        """The micro-batches the loop has collected (all inside one accumulation cycle, in iteration order) as the batched
        passes of accumulation.plan_passes: bucketed by frame shape, each bucket cut into groups of at most `max_group`
        frames; minibatches that are batches themselves (N > 1) run alone."""
        plan = accumulation.plan_passes([item[2]['image'].shape for item in window], max_group, odd_alone=False)
        groups = [[window[i] for i in idx] for idx, _ in plan]
        # (measured at 480x854, passes of 1 / 2 / 3+2 frames: +9.4 % / +2.0 % / -2.6 % - a pass of three or more frames does
        # better with its two forward chains side by side, which needs the auxiliary stream the previous pass's weight
        # gradients would still occupy)
        multi = streams.side is not None and not dp_on and len(groups) > 1 and max(len(g) for g in groups) <= 2
        if lazy_zero:
            # a window that opens a cycle: one pass that is the whole cycle writes its gradients; anything else adds - to
            # zeros (queued here, on the caller's stream, in front of everything the window's passes do on either stream)
            whole_cycle = cycle.counter == 0 and len(groups) == 1 and len(groups[0]) == local_accum
            flags.overwrite_grads = whole_cycle
            if cycle.counter == 0:
                if cycle.grads_stale and not whole_cycle:
                    flat.zero()
                cycle.grads_stale = False
        if multi:
            # both pass streams must see the last optimizer step and the repacked weight images: pack once here, on the
            # caller's stream, instead of inside the first forward pass (which the second stream would have to wait for)
            net.prepack_weights()
            streams.side.wait_stream(torch.cuda.current_stream(device))
        flags.forward_one_stream = multi
        for i, group in enumerate(groups):
            stream = streams.pick(i, len(groups), multi)
            if stream is not None:
                with torch.cuda.stream(stream):
                    run_pass(group)
            else:
                run_pass(group)
            if cycle.advance(len(group)):
                close_cycle()
        if multi:
            # the window's minibatches were allocated on the caller's stream and read on the other one: before they are
            # released (window = [] below; a window can end without a cycle close) the caller's stream waits for it
            streams.wait()
        loss_log.close_window()
        epoch, _idx, _mb, snapshot_due = window[-1]
        if snapshot_due and parallel.rank() == 0:  # (the window ended here: the snapshot holds exactly the updates up to its epoch)
            net_provider.save_model(epoch, sequence=seq_name)

    time_all_start = timeit.default_timer()
    try:
        with accumulation.loop_state(net, flags, options, compact_stage1, min(max_group, avg_grad_every_n) if native else None):
            net.compute_side_outputs = False  # the loss is on outputs[-1] only (src/train_online.py:80): skip the 4 side logit maps
            window = []  # pending (epoch, minibatch index, minibatch, snapshot due behind it) tuples, all of one accumulation cycle
            for epoch in range(start_epoch, n_epochs):
                n_mb = len(dataloader)
                for minibatch_index, minibatch in enumerate(dataloader):
                    snapshot_due = minibatch_index == n_mb - 1 and (epoch % snapshot_every_n) == snapshot_every_n - 1
                    window.append((epoch, minibatch_index, minibatch, snapshot_due))
                    if accumulation.window_closes(len(window), cycle.counter, local_accum, max_window, snapshot_due):
                        run_window(window)
                        window = []
            if window:
                run_window(window)
    finally:  # (behind loop_state's own: the gradients are joined by now)
        if lazy_zero:
            flags.overwrite_grads = False
            if cycle.grads_stale:  # leave the buffers as optimizer.zero_grad() would (src/train_online.py:100-104)
                flat.zero()
        net.compute_side_outputs = True
    time_enqueued = timeit.default_timer() - time_all_start  # how far ahead of the device the host loop ran
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    loss_log.flush(True)
    time_for_all = timeit.default_timer() - time_all_start
    n_images = len(dataloader)
    log.info('Train {0}: total time {1} sec'.format(seq_name, str(time_for_all)))
    log.info('Train {0}: {1} images'.format(seq_name, str(n_images)))
    log.info('Train {0}: time per sample {1} sec'.format(seq_name, str(time_for_all / max(n_images, 1))))
    return {'loss': loss_log.loss_tr, 'seconds': time_for_all, 'iterations': cycle.iterations,
            'seconds_host_enqueue': time_enqueued, 'comm_timing': sync.timing_summary() if sync.active and sync.timing else None}


def main(argv=None):
    global db_root_dir, synthetic_size, data_parallel, save_dir_models, save_dir_results, score, fast_test, png_fitted, device_decode
    global multi_object, synthetic_objects, clean, adapt, rotate, lucid, ensemble, crf, crf_joint, motion
    args = args_helper.parse_args(is_online=True, argv=argv)
    if args.score and args.eval_speeds:
        raise SystemExit('--score needs the PNG-writing test pass; --eval-speeds writes nothing')
    if args.fast_test and args.eval_speeds:
        raise SystemExit('--fast-test is the PNG-writing test pass; --eval-speeds writes nothing')
    score = bool(args.score)
    fast_test = bool(args.fast_test)
    png_fitted = bool(args.png_fitted)
    device_decode = bool(args.device_decode)
    multi_object = bool(args.multi_object)
    clean = None
    if args.clean_min_area is not None or args.clean_largest or args.clean_temporal is not None:
        from fosvos_hip.options import CleanOptions
        clean = CleanOptions(min_area=args.clean_min_area or 0, largest=bool(args.clean_largest),
                             temporal_radius=args.clean_temporal)
    adapt = args.adapt
    rotate = args.rotate
    lucid = args.lucid
    ensemble = args.ensemble
    crf = args.crf_options
    crf_joint = bool(args.crf_joint)
    motion = args.motion
    synthetic_objects = int(args.objects)
    del scored_sequences[:]
    if args.network != 'vgg16':
        raise SystemExit('only --network vgg16 is implemented on the HIP path (ResNet family: SURVEY.md §8 f4)')
    data_parallel = bool(args.data_parallel) and parallel.init_distributed()
    gpu_handler.select_gpu(args.gpu_id)

    db_root_dir = P.db_root_dir()
    synthetic_size = (args.height, args.width) if args.synthetic else None
    save_dir_models.mkdir(parents=True, exist_ok=True)
    save_dir_results.mkdir(parents=True, exist_ok=True)
    path_input_model = Path(args.parent_model) if args.parent_model else save_dir_models / 'vgg16_epoch-239.pth'
    path_output_model_base = save_dir_models / path_stem
    path_output_model_base.mkdir(parents=True, exist_ok=True)

    settings = OnlineSettings(is_training=args.is_training, is_testing=args.is_testing, start_epoch=0,
                              n_epochs=args.n_epochs or 10000, avg_grad_every_n=args.avg_grad_every_n or 5,
                              snapshot_every_n=args.n_epochs or 10000, is_testing_while_training=False, test_every_n=5,
                              batch_size_train=1, batch_size_test=1, is_visualizing_network=False,
                              is_visualizing_results=False, offline_epoch=240, variant_offline=args.variant_offline,
                              variant_online=args.variant_online, eval_speeds=args.eval_speeds)

    provider_class = provider_mapping[('online', args.network)]

    def make_provider():
        return provider_class(name=args.network, save_dir=(path_input_model, path_output_model_base), settings=settings,
                              variant_offline=args.variant_offline, variant_online=args.variant_online)

    net_provider = make_provider()
    if args.synthetic and not path_input_model.exists():
        # no parent checkpoint offline: write a seeded random-init one so the load path is exercised
        from networks.osvos_vgg import OSVOS_VGG
        torch.manual_seed(0)
        if parallel.rank() == 0:
            path_input_model.parent.mkdir(parents=True, exist_ok=True)
            torch.save(OSVOS_VGG(pretrained=0).state_dict(), str(path_input_model))
        if data_parallel:
            torch.distributed.barrier()

    if multi_object:
        if args.sequence_name is not None:
            sequences = [args.sequence_name]
        elif args.synthetic:
            sequences = ['synthetic']
        else:
            from dataloaders.davis_2017 import sequence_names
            sequences = parallel.shard_sequences(sequence_names(db_root_dir, 'val'), args.sequence_group,
                                                 args.sequence_group_size)
        for s in sequences:
            train_and_test_objects(make_provider, s, settings)
        if score and scored_sequences:
            # the run's mean is over OBJECTS: every object of every sequence counts once
            objects = [o for r in scored_sequences for o in r['objects']]
            _log_mean_score(objects, '{0} objects of {1} sequences'.format(len(objects), len(scored_sequences)))
        return
    if args.sequence_name is None:
        # replicas: the reference's -sg/-sgs sharding; under torchrun without --data-parallel the ranks shard
        group, group_size = args.sequence_group, args.sequence_group_size
        if group is None and not data_parallel and parallel.init_distributed():
            group, group_size = parallel.rank(), parallel.world_size()
        sequences = parallel.shard_sequences(sequences_val, group, group_size)
        [train_and_test(net_provider, s, settings) for s in sequences]
    else:
        train_and_test(net_provider, args.sequence_name, settings)
    if score and scored_sequences:
        _log_mean_score(scored_sequences, '{0} sequences'.format(len(scored_sequences)))


if __name__ == '__main__':
    main()
