"""Inference pass over a sequence (reference: src/util/experiment_helper.py:20-80): forward, sigmoid,
write probability PNGs; with ``eval_speeds`` time ``net.forward`` between device synchronisations
over 10 passes, dropping the first minibatch of each pass (the reference's protocol, :29-53,77-80;
no PNGs are written in that mode, as in the reference).

``test_scored`` (an extension: the reference leaves evaluation to an outside toolkit) is the same pass with the sigmoid,
the byte stretch and the DAVIS 2016 J / F counts computed on the device beside the logits (fosvos_prob_bytes,
fosvos_jf_counts); ``test`` itself keeps the reference's host path.

``test_fast`` (opt-in, ``--fast-test``) forwards the frames in groups, has the device encode the PNG files as well
(fosvos_png_encode, layout: util/png_layout.py) and leaves the host nothing to do but write them.

``test_objects`` (``--multi-object``) is ``test_fast`` for a sequence of several objects: K nets, one per object, forward every
group; the device merges their answers into label maps, encodes palette PNG files and counts J / F per object
(util/object_merge.py states the definitions).

``test_adaptive`` (``--adapt-steps N``) is the test pass with online adaptation: between a frame's two forward passes the net
takes fine-tune steps against pseudo-labels made from its own output on the device (util/online_adapt.py states them).

``test_fast`` and ``test_objects`` take ``ensemble=`` (``--ensemble-flip``, ``--ensemble-scales``): the net also sees every frame
mirrored and at other sizes, and the device averages its answers back on the frame's grid (util/test_ensemble.py states it).
They also take ``crf=`` (``--crf``): a local CRF on the frame's colours refines the logits on the device before anything else
reads them (util/mask_crf.py states it); ``test_objects`` with ``crf_joint=True`` (``--crf-joint``) runs ONE CRF over the labels
0..K in the place of a CRF per net and the label merge (util/label_crf.py states it).  ``test_fast`` takes ``motion=`` (``--clean-motion``) beside a temporal gate: the
gate's seed is carried along the motion of the picture, estimated by block matching on the device (util/block_motion.py
states it)."""
import timeit
from pathlib import Path
from typing import Callable, Optional

import numpy as np
import torch
from torch import cuda

from util import davis_measures, gpu_handler
from util.logger import get_logger

log = get_logger(__file__)

# what the last call of test() did: {'n_runs', 'n_forward', 'times' (seconds, the kept samples), 'accurate_images',
# 'time_per_sample'}.  The reference only logs these numbers (:70-80); tests and bench.py read them here.
last_eval = {}
# what the last call of test_scored() (or of test_fast() / test_objects() with annotations) returned
last_score = {}
# what the last call of test_fast() did: {'n_frames', 'n_groups', 'group_sizes', 'seconds', host seconds per stage:
# 'seconds_load' (waiting for the loader), 'seconds_issue' (upload, forward and encode calls), 'seconds_wait' (for the
# device and the copy), 'seconds_write' (files), 'png_bytes', 'png_huffman'}
last_fast = {}


def bytescale(data: np.ndarray) -> np.ndarray:
    """What ``scipy.misc.imsave`` did to a float image before writing it (reference: src/util/experiment_helper.py:64
    calls it on the sigmoid map; scipy 1.0/1.1 ``misc.pilutil``: imsave -> toimage -> bytescale with cmin = data.min(),
    cmax = data.max(), low = 0, high = 255): the map is stretched to ITS OWN value range, then rounded half up."""
    data = np.asarray(data, dtype=np.float64)
    cmin, cmax = float(data.min()), float(data.max())
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1.0
    scaled = (data - cmin) * (255.0 / cscale)
    return (scaled.clip(0, 255) + 0.5).astype(np.uint8)


def _save_png(path: Path, prob: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(bytescale(prob), mode='L').save(str(path))


def test(net_provider, data_loader, save_dir: Path, is_visualizing_results: bool, eval_speeds: bool,
         seq_name: Optional[str] = None):
    log.info('Testing Network')
    net = net_provider.network
    n_runs = 10 if eval_speeds else 1
    times = []
    n_forward = 0
    time_all_start = timeit.default_timer()
    with torch.no_grad():
        for _ in range(n_runs):
            for minibatch_index, minibatch in enumerate(data_loader):
                img, gt = minibatch['image'], minibatch['gt']
                minibatch_seq_name, fname = minibatch['seq_name'], minibatch['fname']
                inputs, gts = gpu_handler.cast_cuda_if_possible([img, gt])
                if eval_speeds:
                    cuda.synchronize()
                    time_image_start = timeit.default_timer()
                outputs = net.forward(inputs)
                n_forward += 1
                if eval_speeds:
                    cuda.synchronize()
                    if minibatch_index > 0:  # first allocate takes longer
                        times.append(timeit.default_timer() - time_image_start)
                else:
                    # reference :57-59: 1 / (1 + exp(-pred)) in numpy on the host
                    pred = outputs[-1].cpu().numpy()
                    probs = 1.0 / (1.0 + np.exp(-pred))
                    for index in range(inputs.size()[0]):
                        save_dir_seq = Path(save_dir) / minibatch_seq_name[index]
                        save_dir_seq.mkdir(parents=True, exist_ok=True)
                        _save_png(save_dir_seq / '{0}.png'.format(fname[index]), probs[index, 0])
    time_for_all = timeit.default_timer() - time_all_start
    n_images = len(data_loader)
    time_per_sample = time_for_all / max(n_images, 1)
    log.info('Test {0}: total test time {1} sec'.format(seq_name, str(time_for_all)))
    log.info('Test {0}: {1} images'.format(seq_name, str(n_images)))
    log.info('Test {0}: time per sample {1} sec'.format(seq_name, str(time_per_sample)))
    last_eval.clear()
    last_eval.update(n_runs=n_runs, n_forward=n_forward, times=list(times), accurate_images=(n_images - 1) * n_runs,
                     time_per_sample=time_per_sample)
    if eval_speeds and times:
        log.info('Test {0}: accurate {1} images'.format(seq_name, str((n_images - 1) * n_runs)))
        log.info('Test {0}: accurate total time {1} sec ({2} runs)'.format(seq_name, np.sum(times), n_runs))
        log.info('Test {0}: accurate time per sample {1} sec ({2} runs)'.format(seq_name, np.average(times), n_runs))
        return float(np.average(times))
    return None


def _frame_annotation(annotations: Callable, seq: str, fname: str, h: int, w: int, ids: bool = False) -> Optional[np.ndarray]:
    """uint8 [H,W] of one frame, or None: 1 = object, or with ``ids`` the object ids as they come."""
    ann = annotations(seq, fname)
    if ann is None:
        return None
    ann = np.asarray(ann)
    if ann.shape != (h, w):
        raise ValueError('annotation of {}/{} is {}, the logits are {}'.format(seq, fname, ann.shape, (h, w)))
    return ann.astype(np.uint8) if ids else (ann != 0).astype(np.uint8)


class _Frames:
    """The frames a test pass has seen so far: their sequences, their names and whether each has an annotation."""

    def __init__(self, data_loader, save_dir: Path) -> None:
        self.n_frames, self.save_dir = len(data_loader.dataset), Path(save_dir)
        self.seqs, self.fnames, self.scored = [], [], []

    def __len__(self) -> int:
        return len(self.fnames)

    def add(self, minibatches, h: int, w: int, annotations: Optional[Callable], ids: bool = False):
        """Takes a group's minibatches in.  Returns the index of its first frame, its annotations as one uint8 [n,H,W] (a
        frame without one: zeros, and not scored; None without ``annotations``) and the paths of its files."""
        first = len(self.fnames)
        n = sum(len(minibatch['fname']) for minibatch in minibatches)
        if first + n > self.n_frames:
            raise RuntimeError('the loader yields more frames than its dataset holds ({})'.format(self.n_frames))
        gt = np.zeros((n, h, w), dtype=np.uint8) if annotations is not None else None
        for minibatch in minibatches:
            for seq, fname in zip(minibatch['seq_name'], minibatch['fname']):
                ann = _frame_annotation(annotations, seq, fname, h, w, ids) if annotations is not None else None
                if ann is not None:
                    gt[len(self.fnames) - first] = ann
                self.seqs.append(seq)
                self.fnames.append(fname)
                self.scored.append(ann is not None)
        paths = [self.save_dir / self.seqs[k] / '{0}.png'.format(self.fnames[k]) for k in range(first, first + n)]
        return first, gt, paths

    def score_head(self, seq_name: Optional[str], radius) -> dict:
        """The keys every score dict starts with."""
        return {'seq_name': seq_name if seq_name is not None else (self.seqs[0] if self.seqs else None),
                'radius': radius, 'fnames': list(self.fnames), 'scored': [bool(k) for k in self.scored]}


class _Counters:
    """Integer counters per frame, [n_frames, *tail]: an int64 array the host branches fill, or - made at its first use - an
    int32 device tensor whose rows the kernels fill and which comes back in ONE read at the end of the pass."""

    def __init__(self, n_frames: int, *tail: int) -> None:
        self.host, self.dev = np.zeros((n_frames,) + tail, dtype=np.int64), None

    def rows(self, first: int, n: int, device) -> torch.Tensor:
        if self.dev is None:
            self.dev = torch.zeros(self.host.shape, dtype=torch.int32, device=device)
        return self.dev[first:first + n]

    def read(self, n_seen: int) -> np.ndarray:
        if self.dev is not None:
            self.host, self.dev = self.dev.cpu().numpy().astype(np.int64), None
        return self.host[:n_seen]


def _sequence_score(frames: _Frames, counts: np.ndarray, radius, seconds: float, seq_name: Optional[str], **extra) -> dict:
    """The score dict of one object's sequence from its [n,6] J / F counts (``test_scored`` states the keys)."""
    j, f = davis_measures.jf_from_counts(counts) if len(frames) else (np.zeros(0), np.zeros(0))
    keep = np.asarray(frames.scored, dtype=bool)
    j_stats = davis_measures.sequence_statistics(j[keep])
    f_stats = davis_measures.sequence_statistics(f[keep])
    return {**frames.score_head(seq_name, radius),
            'counts': [[int(v) for v in row] if k else None for row, k in zip(counts, keep)],
            'J': [float(v) if k else None for v, k in zip(j, keep)],
            'F': [float(v) if k else None for v, k in zip(f, keep)],
            'J_stats': j_stats, 'F_stats': f_stats, 'J&F': (j_stats['mean'] + f_stats['mean']) / 2,
            'seconds': seconds, **extra}


class _Slot:
    """Device bytes laid out as [n files at capacity | n int32 lengths] - the lengths sit behind the files in the same buffer,
    so that one copy brings both - and their pinned twin on the host."""

    def __init__(self, n: int, cap: int, device) -> None:
        self.n, self.cap = n, cap
        self.dev = torch.empty(n * cap + 4 * n, dtype=torch.uint8, device=device)
        self.host = torch.empty(n * cap + 4 * n, dtype=torch.uint8).pin_memory()
        self.files, self.lengths = self.dev[:n * cap].view(n, cap), self.dev[n * cap:].view(torch.int32)

    def send(self, paths):
        """The ONE copy of a group, at capacity, and the event that says it has landed: the group's pending item."""
        self.host.copy_(self.dev, non_blocking=True)
        landed = torch.cuda.Event()
        landed.record()
        return self, landed, paths


class _FileSlots:
    """The files of a pass.  The device encodes a group's files into one of two slots, so the host can write a group's files
    one group later, while the device works on the next."""

    def __init__(self) -> None:
        self.slots, self.turn, self.png_bytes = {}, 0, 0

    def take(self, n: int, h: int, w: int, capacity: int, device) -> _Slot:
        key = (self.turn, n, h, w, capacity + -capacity % 4)
        self.turn ^= 1
        if key not in self.slots:
            self.slots[key] = _Slot(n, key[-1], device)
        return self.slots[key]

    def write(self, paths, blobs) -> None:
        for path, blob in zip(paths, blobs):
            path.parent.mkdir(parents=True, exist_ok=True)
            with open(str(path), 'wb') as fh:
                fh.write(blob)
            self.png_bytes += len(blob)

    def retire(self, item, stage: Optional[dict] = None) -> None:
        """Waits for a sent group to have landed and writes its files; ``stage`` receives the seconds of either."""
        slot, landed, paths = item
        t0 = timeit.default_timer()
        landed.synchronize()
        t1 = timeit.default_timer()
        n, cap = slot.n, slot.cap
        lengths = slot.host[n * cap:].view(torch.int32).tolist()
        data = slot.host.numpy()
        self.write(paths, [data[k * cap:k * cap + lengths[k]].data for k in range(n)])
        if stage is not None:
            stage['wait'] += t1 - t0
            stage['write'] += timeit.default_timer() - t1


def _forward_logits(net, inputs: torch.Tensor, forward_batch: int) -> torch.Tensor:
    """The fused logits of a batch, fp32 [n,1,H,W], forwarded ``forward_batch`` frames a call."""
    n = int(inputs.shape[0])
    if n <= forward_batch:
        return net.forward(inputs)[-1].detach().float().contiguous()
    return torch.cat([net.forward(inputs[k:k + forward_batch])[-1].detach().float() for k in range(0, n, forward_batch)])


def _check_ensemble(who: str, ensemble) -> None:
    if ensemble is not None:
        from fosvos_hip.options import EnsembleOptions
        if not isinstance(ensemble, EnsembleOptions):
            raise ValueError('{}: ensemble must be a fosvos_hip.options.EnsembleOptions or None, got {!r}'.format(who, ensemble))


def _ensemble_inputs(inputs: torch.Tensor, ensemble) -> list:
    """The views of a group's frames, one tensor per view of ``ensemble.views()``: ONE ``ops.ensemble_views`` call on the
    device (the unflipped view of the frame's size is ``inputs`` itself), ``test_ensemble.make_views`` for CPU tensors."""
    if inputs.is_cuda:
        from fosvos_hip import ops
        return ops.ensemble_views(inputs, ensemble.views())
    from util import test_ensemble
    return [torch.from_numpy(v) for v in test_ensemble.make_views(inputs.numpy(), ensemble.views())]


def _ensemble_logits(net, inputs: torch.Tensor, forward_batch: int, ensemble, views: Optional[list] = None) -> torch.Tensor:
    """``_forward_logits`` behind a test-time ensemble (``ensemble``: an EnsembleOptions; None: ``_forward_logits`` itself,
    nothing else is called).  The net forwards every view of the group in view order - ``views``: what ``_ensemble_inputs``
    made, where several nets share it; None: made here - and ONE ``ops.ensemble_merge`` averages its V answers back on the
    frame's grid (CPU tensors: ``test_ensemble.merge``).  No host synchronisation."""
    if ensemble is None:
        return _forward_logits(net, inputs, forward_batch)
    if views is None:
        views = _ensemble_inputs(inputs, ensemble)
    maps = [_forward_logits(net, view, forward_batch) for view in views]
    h, w = int(inputs.shape[2]), int(inputs.shape[3])
    if maps[0].is_cuda:
        from fosvos_hip import ops
        return ops.ensemble_merge(maps, ensemble.views(), (h, w))
    from util import test_ensemble
    return torch.from_numpy(test_ensemble.merge([m.numpy() for m in maps], ensemble.views(), h, w))


def _check_crf(who: str, crf) -> None:
    if crf is not None:
        from fosvos_hip.options import CrfOptions
        if not isinstance(crf, CrfOptions):
            raise ValueError('{}: crf must be a fosvos_hip.options.CrfOptions or None, got {!r}'.format(who, crf))


def _crf_logits(inputs: torch.Tensor, logits: torch.Tensor, crf) -> torch.Tensor:
    """A group's logits fp32 [n,1,H,W] refined by the CRF on the group's uploaded frames ``inputs`` (``crf``: a CrfOptions): ONE
    ``ops.crf_refine`` on the device, ``mask_crf.refine`` frame by frame for CPU tensors.  No host synchronisation."""
    if logits.is_cuda:
        from fosvos_hip import ops
        return ops.crf_refine(inputs.float().contiguous(), logits, crf)
    from util import mask_crf
    return torch.from_numpy(mask_crf.refine_batch(inputs.float().cpu().contiguous().numpy(), logits.numpy(), crf))


def _crf_joint_labels(inputs: torch.Tensor, logits, crf):
    """A group's label maps uint8 [n,H,W] from the K nets' logits fp32 [n,1,H,W] by the joint CRF on the group's uploaded
    frames ``inputs``: ONE ``ops.crf_labels`` on the device (a tensor), ``label_crf.refine_labels_batch`` for CPU logits (an
    array; the frames come to the host if they were uploaded).  No host synchronisation on the device path."""
    if logits[0].is_cuda:
        from fosvos_hip import ops
        return ops.crf_labels(inputs.float().contiguous(), logits, crf)
    from util import label_crf
    return label_crf.refine_labels_batch(inputs.float().cpu().contiguous().numpy(), [x.numpy() for x in logits], crf)[0]


def _check_motion(who: str, motion, clean) -> None:
    if motion is not None:
        from fosvos_hip.options import MotionOptions
        if not isinstance(motion, MotionOptions):
            raise ValueError('{}: motion must be a fosvos_hip.options.MotionOptions or None, got {!r}'.format(who, motion))
        if clean is None or getattr(clean, 'temporal_radius', None) is None:
            raise ValueError('{}: motion carries the seed of the temporal gate along the picture\'s motion: it needs '
                             'clean=CleanOptions(temporal_radius=...)'.format(who))


class _MotionBuffers:
    """What the motion-compensated gate keeps on the device per frame size: the luma planes of a group behind the last plane
    of the group before ([group + 1, H, W]; plane 0 is that last plane), the fields and costs of the group's pairs and the
    warped seed.  Allocated at the first group of a size."""

    def __init__(self, group: int, h: int, w: int, block: int, device) -> None:
        hb, wb = -(-h // block), -(-w // block)
        self.luma = torch.empty((group + 1, h, w), dtype=torch.uint8, device=device)
        self.field = torch.empty((group, hb, wb, 2), dtype=torch.int8, device=device)
        self.cost = torch.empty((group, hb, wb), dtype=torch.int32, device=device)
        self.warped = torch.empty((1, h, w), dtype=torch.uint8, device=device)


def _motion_clean(ops, inputs: torch.Tensor, logits: torch.Tensor, seed_dev, kept: torch.Tensor, buffers: _MotionBuffers,
                  continued: bool, clean, motion) -> None:
    """A group's chain with its seed carried along the motion: ONE ``motion_luma`` of the group's uploaded frames, ONE
    ``motion_estimate`` over its consecutive pairs - the pair across the group boundary included when the chain is
    ``continued``: plane 0 of ``buffers.luma`` then holds the last plane of the group before and ``seed_dev`` what that frame
    kept -, and per frame ``motion_warp`` of the seed and ``clean_components`` on that one frame, in place.  The very first
    frame of a chain is gated by ``seed_dev`` unwarped (None: not gated).  No host synchronisation."""
    n = int(logits.shape[0])
    planes = buffers.luma
    ops.motion_luma(inputs.float().contiguous(), out=planes[1:n + 1])
    lo = 0 if continued else 1          # the first plane that is a pair's previous frame
    pairs = n - lo
    if pairs > 0:
        ops.motion_estimate(planes[lo:n], planes[lo + 1:n + 1], motion, field=buffers.field[:pairs], cost=buffers.cost[:pairs])
    for t in range(n):
        seed = seed_dev if t == 0 else kept[t - 1:t]
        if t > 0 or continued:
            pair = t - lo
            seed = ops.motion_warp(seed, buffers.field[pair:pair + 1], motion.block, out=buffers.warped)
        ops.clean_components(logits[t:t + 1], seed, clean.temporal_radius, clean.min_area, clean.largest, chain=True,
                             fill=clean.fill, out=logits[t:t + 1], kept=kept[t:t + 1])
    planes[0].copy_(planes[n])          # the next group's boundary pair: a copy in stream order, no host


def _check_png_huffman(who: str, png_huffman: str) -> None:
    from util import png_layout
    if png_huffman not in png_layout.HUFFMAN_MODES:
        raise ValueError('{}: png_huffman must be one of {}, got {!r}'.format(who, png_layout.HUFFMAN_MODES, png_huffman))


def _check_batching(who: str, group: int, forward_batch: int) -> None:
    if group < 1 or forward_batch < 1:
        raise ValueError('{}: group and forward_batch must be at least 1, got {} and {}'.format(who, group, forward_batch))


def test_scored(net_provider, data_loader, save_dir: Path, annotations: Callable, write_png: bool = True,
                seq_name: Optional[str] = None) -> dict:
    """The test pass with its score.  Per minibatch: forward; on the device ``ops.prob_bytes`` (the PNG bytes: 1 B a
    pixel comes back instead of the 4 B of the logits) and ``ops.jf_counts`` into the minibatch's rows of one
    [n_frames,6] counter tensor, which is read back ONCE after the last frame.  The files are the ones ``test`` writes,
    ``<save_dir>/<seq>/<fname>.png``; their bytes come from the sigmoid in fp64 where ``test`` takes it in fp32, so a byte
    may differ by one where the stretched value sits on a rounding boundary.
    ``annotations(seq_name, fname)`` -> uint8 [H,W] (non-zero = object) or None (the frame gets its PNG but no score).
    CPU logits take the host path: ``bytescale`` of the fp64 sigmoid and ``davis_measures.jf_counts_numpy``.
    Returns (and keeps in ``last_score``) per-frame J, F and counts, ``sequence_statistics`` of J and F over the scored
    frames and 'J&F' = (J mean + F mean) / 2."""
    from PIL import Image
    log.info('Testing Network (scored)')
    net = net_provider.network
    frames = _Frames(data_loader, save_dir)
    counts, radius = _Counters(frames.n_frames, 6), None
    time_all_start = timeit.default_timer()
    with torch.no_grad():
        for minibatch in data_loader:
            inputs, = gpu_handler.cast_cuda_if_possible([minibatch['image']])
            logits = net.forward(inputs)[-1].detach().float().contiguous()
            n, h, w = int(logits.shape[0]), int(logits.shape[2]), int(logits.shape[3])
            radius = davis_measures.default_radius(h, w)
            first, gt, paths = frames.add([minibatch], h, w, annotations)
            if logits.is_cuda:
                from fosvos_hip import ops
                ops.jf_counts(logits, torch.from_numpy(gt).to(logits.device), radius, out=counts.rows(first, n, logits.device))
                png = ops.prob_bytes(logits).cpu().numpy() if write_png else None
            else:
                x = logits[:, 0].numpy().astype(np.float64)
                for index in range(n):
                    counts.host[first + index] = davis_measures.jf_counts_numpy(x[index] >= 0, gt[index], radius)
                png = np.stack([bytescale(1.0 / (1.0 + np.exp(-x[index]))) for index in range(n)]) if write_png else None
            if write_png:
                for index in range(n):
                    paths[index].parent.mkdir(parents=True, exist_ok=True)
                    Image.fromarray(png[index], mode='L').save(str(paths[index]))
    counts_host = counts.read(len(frames))
    time_for_all = timeit.default_timer() - time_all_start
    score = _sequence_score(frames, counts_host, radius, time_for_all, seq_name)
    log.info('Test {0}: {1} images, {2} scored, total test time {3} sec'.format(seq_name, len(frames), sum(frames.scored),
                                                                               time_for_all))
    last_score.clear()
    last_score.update(score)
    return score


def _frame_groups(data_loader, group: int):
    """The loader's minibatches, consecutive ones of one frame shape joined while they hold at most ``group`` frames."""
    held, n_held = [], 0
    for minibatch in data_loader:
        n = int(minibatch['image'].shape[0])
        if held and (n_held + n > group or minibatch['image'].shape[1:] != held[0]['image'].shape[1:]):
            yield held
            held, n_held = [], 0
        held.append(minibatch)
        n_held += n
    if held:
        yield held


def test_fast(net_provider, data_loader, save_dir: Path, annotations: Optional[Callable] = None, group: int = 5,
              seq_name: Optional[str] = None, forward_batch: int = 2, png_huffman: str = 'fixed', clean=None,
              clean_seed: Optional[np.ndarray] = None, ensemble=None, crf=None, motion=None) -> Optional[dict]:
    """The test pass with the PNG files made on the device.  Up to ``group`` consecutive frames of one shape are uploaded
    as one batch and forwarded ``forward_batch`` frames a call into one logit tensor.  Two frames a call is the largest
    batch whose frames the engine computes exactly as it computes a frame alone (a batch runs as two chains of ceil(N/2)
    and floor(N/2) frames, and a chain's tile plans and K splits depend on its frame count): the files hold the pixels of
    the one-frame-a-call passes ``test`` and ``test_scored``, where a five-frame forward rounds its bf16 activations
    differently and moves bytes by tens of steps on steep maps (``forward_batch=group`` selects that).
    ``ops.prob_bytes`` and ``ops.png_encode`` turn the group's logits into complete PNG files (layout:
    util/png_layout.py - the pixels ``test_scored`` writes, in a larger file of many IDAT chunks), ONE copy per group brings
    the file buffer and the lengths to pinned host memory, and the host writes ``<save_dir>/<seq>/<fname>.png`` with plain
    ``write`` calls - for the previous group, after the next group's forward pass has been issued.  The copy moves the
    buffer at its capacity (the layout's size bound, about the stored size): the lengths are only known on the device, and
    asking for them first would put a host synchronisation in front of every group's copy.
    ``annotations`` (as for ``test_scored``): the J / F counts are taken on the device as well and the score dict of
    ``test_scored`` is returned (and kept in ``last_score``); without it the pass returns None.
    CPU logits take the host path: ``bytescale`` of the fp64 sigmoid, ``png_layout.encode``.
    ``png_huffman='fitted'`` (``--png-fitted``): segments may be dynamic-Huffman blocks with a code fitted to them - the
    same pixels in smaller files (never larger, segment by segment).
    ``clean`` (a ``fosvos_hip.options.CleanOptions``; None: nothing changes): each group's logits go through ONE
    ``ops.clean_components``, in place, before the counts and the bytes are taken (util/mask_components.py states the rules;
    CPU logits: ``mask_components.clean_sequence``).  With ``clean.temporal_radius`` the group is a chain: its first frame is
    gated by what the last frame of the group before kept - carried on the device - and the very first frame by
    ``clean_seed`` (uint8 or bool [H,W], non-zero = object; None: not gated).  The score dict then holds the options under
    'clean'.
    ``ensemble`` (a ``fosvos_hip.options.EnsembleOptions``; None: nothing changes): the test-time ensemble.  ONE
    ``ops.ensemble_views`` makes the group's mirrored and rescaled views, the net forwards them view by view
    (``forward_batch`` frames a call, as above) and ONE ``ops.ensemble_merge`` averages the answers back on the frame's grid
    (util/test_ensemble.py states both; CPU tensors take it).  Cleaning, counts and bytes work on the merged logits; no host
    synchronisation is added.  The score dict and ``last_fast`` then hold the options under 'ensemble'.
    ``crf`` (a ``fosvos_hip.options.CrfOptions``; None: nothing changes): each group's logits - the merged ones behind an
    ensemble - go through ONE ``ops.crf_refine`` whose guide is the group's uploaded frames, before the cleaning, the counts
    and the bytes (util/mask_crf.py states it; CPU tensors: ``mask_crf.refine``).  No host synchronisation is added.  The
    score dict and ``last_fast`` then hold the options under 'crf'.
    ``motion`` (a ``fosvos_hip.options.MotionOptions``; None: nothing changes; it needs ``clean.temporal_radius``): the
    temporal gate follows the picture.  Per group ONE ``ops.motion_luma`` of the uploaded frames and ONE
    ``ops.motion_estimate`` over the consecutive pairs - the pair across the group boundary uses the last luma plane of the
    group before, kept on the device -, then frame by frame ``ops.motion_warp`` of what the frame before kept and
    ``ops.clean_components`` on that one frame with the warped mask as its seed (util/block_motion.py: ``gate_sequence``
    states it and is the CPU tensors' path).  The sequence's first frame is gated by ``clean_seed`` unwarped; a change of the
    frame size starts the chain again.  It sits where cleaning sits, behind the ensemble's merge and the CRF; no host
    synchronisation is added.  The score dict and ``last_fast`` then hold the options under 'motion'."""
    from util import png_layout
    _check_png_huffman('test_fast', png_huffman)
    _check_batching('test_fast', group, forward_batch)
    _check_ensemble('test_fast', ensemble)
    _check_crf('test_fast', crf)
    _check_motion('test_fast', motion, clean)
    if clean is None and clean_seed is not None:
        raise ValueError('test_fast: clean_seed is the first seed of clean=CleanOptions(temporal_radius=...)')
    if clean is not None:
        from fosvos_hip.options import CleanOptions
        if not isinstance(clean, CleanOptions):
            raise ValueError('test_fast: clean must be a fosvos_hip.options.CleanOptions or None, got {!r}'.format(clean))
        if clean_seed is not None and not clean.chain:
            raise ValueError('test_fast: clean_seed is the first seed of the temporal gate: set clean.temporal_radius')
        if clean_seed is not None:
            clean_seed = np.asarray(clean_seed)
            if clean_seed.ndim != 2 or clean_seed.dtype not in (np.uint8, np.bool_):
                raise ValueError('test_fast: clean_seed must be a uint8 or bool [H,W] mask, got {} {}'.format(
                    clean_seed.dtype, clean_seed.shape))
            clean_seed = np.ascontiguousarray((clean_seed != 0).astype(np.uint8))
    seed_host = clean_seed   # the chain's seed for the next group: host form (CPU logits) ...
    seed_dev = None          # ... and device form, uint8 [1,H,W]
    kept_dev = {}            # (n, h, w) -> the group's kept masks
    motion_dev = {}          # (h, w) -> the _MotionBuffers of that frame size
    motion_size = None       # the frame size whose last luma plane the device holds (motion): the chain can continue
    motion_host = None       # (luma plane, kept mask) of the last frame, host form (motion, CPU logits)
    log.info('Testing Network (fast)')
    net = net_provider.network
    frames = _Frames(data_loader, save_dir)
    counts, radius = _Counters(frames.n_frames, 6), None
    files = _FileSlots()
    pending = None   # the sent group whose files are not written yet
    stage = {'load': 0.0, 'issue': 0.0, 'wait': 0.0, 'write': 0.0}
    group_sizes = []
    time_all_start = timeit.default_timer()
    with torch.no_grad():
        groups = iter(_frame_groups(data_loader, group))
        while True:
            t0 = timeit.default_timer()
            minibatches = next(groups, None)
            stage['load'] += timeit.default_timer() - t0
            if minibatches is None:
                break
            t0 = timeit.default_timer()
            images = minibatches[0]['image'] if len(minibatches) == 1 else torch.cat([m['image'] for m in minibatches])
            inputs, = gpu_handler.cast_cuda_if_possible([images])
            n = int(inputs.shape[0])
            logits = _ensemble_logits(net, inputs, forward_batch, ensemble)
            if crf is not None:
                logits = _crf_logits(inputs, logits, crf)
            h, w = int(logits.shape[2]), int(logits.shape[3])
            first, gt, paths = frames.add(minibatches, h, w, annotations)
            group_sizes.append(n)
            radius = davis_measures.default_radius(h, w)
            if clean is not None and seed_host is not None and seed_host.shape != (h, w):
                if first == 0:
                    raise ValueError('test_fast: clean_seed is {}, the logits are {}'.format(seed_host.shape, (h, w)))
                seed_host = seed_dev = None  # the frames changed their size: the chain starts again, ungated
            if logits.is_cuda:
                from fosvos_hip import ops
                if clean is not None:
                    if clean.chain:
                        if seed_dev is not None and tuple(seed_dev.shape) != (1, h, w):
                            seed_dev = None
                        if seed_dev is None and first == 0 and seed_host is not None:
                            seed_dev = torch.from_numpy(seed_host[None]).to(logits.device)
                        if (n, h, w) not in kept_dev:
                            kept_dev[(n, h, w)] = torch.empty((n, h, w), dtype=torch.uint8, device=logits.device)
                        kept = kept_dev[(n, h, w)]
                        if motion is None:
                            ops.clean_components(logits, seed_dev, clean.temporal_radius, clean.min_area, clean.largest,
                                                 chain=True, fill=clean.fill, out=logits, kept=kept)
                        else:
                            if (h, w) not in motion_dev:
                                motion_dev[(h, w)] = _MotionBuffers(group, h, w, motion.block, logits.device)
                            _motion_clean(ops, inputs, logits, seed_dev, kept, motion_dev[(h, w)],
                                          motion_size == (h, w) and seed_dev is not None, clean, motion)
                            motion_size = (h, w)
                        # what the group's last frame kept gates the next group's first: a copy in stream order, no host
                        if seed_dev is None:
                            seed_dev = torch.empty((1, h, w), dtype=torch.uint8, device=logits.device)
                        seed_dev.copy_(kept[n - 1:n])
                    else:
                        ops.clean_components(logits, None, 0, clean.min_area, clean.largest, fill=clean.fill, out=logits)
                if annotations is not None:
                    ops.jf_counts(logits, torch.from_numpy(gt).to(logits.device), radius,
                                  out=counts.rows(first, n, logits.device))
                slot = files.take(n, h, w, ops.png_capacity(h, w), logits.device)
                ops.png_encode(ops.prob_bytes(logits), out=slot.files, lengths=slot.lengths, huffman=png_huffman)
                sent = slot.send(paths)
                stage['issue'] += timeit.default_timer() - t0
                if pending is not None:
                    files.retire(pending, stage)  # the previous group's files, while the device works on this group
                pending = sent
            else:
                x = logits[:, 0].numpy()
                if motion is not None:
                    from util import block_motion
                    if motion_host is not None and motion_host[0].shape != (h, w):
                        motion_host = None  # the frames changed their size: the chain starts again
                    frames_host = inputs.float().contiguous().numpy()
                    x, kept = block_motion.gate_sequence(
                        frames_host, np.ascontiguousarray(x, dtype=np.float32), seed_host if motion_host is None else None,
                        clean, motion, *(motion_host or (None, None)))
                    motion_host = (block_motion.luma(frames_host[n - 1]), kept[n - 1])
                    seed_host = None  # used: every later frame is gated by what the frame before kept
                elif clean is not None:
                    from util import mask_components
                    x, kept = mask_components.clean_sequence(
                        np.ascontiguousarray(x, dtype=np.float32), seed_host if clean.chain else None,
                        clean.temporal_radius if clean.chain else 0, clean.min_area, clean.largest, chain=clean.chain,
                        fill=clean.fill)
                    seed_host = kept[n - 1].astype(np.uint8) if clean.chain else None
                x = x.astype(np.float64)
                blobs = []
                for index in range(n):
                    if annotations is not None:
                        counts.host[first + index] = davis_measures.jf_counts_numpy(x[index] >= 0, gt[index], radius)
                    blobs.append(png_layout.encode(bytescale(1.0 / (1.0 + np.exp(-x[index]))), huffman=png_huffman))
                stage['issue'] += timeit.default_timer() - t0
                t0 = timeit.default_timer()
                files.write(paths, blobs)
                stage['write'] += timeit.default_timer() - t0
        if pending is not None:
            files.retire(pending, stage)
    counts_host = counts.read(len(frames))
    time_for_all = timeit.default_timer() - time_all_start
    cleaned = {'clean': clean.as_dict()} if clean is not None else {}
    if ensemble is not None:
        cleaned['ensemble'] = ensemble.as_dict()
    if crf is not None:
        cleaned['crf'] = crf.as_dict()
    if motion is not None:
        cleaned['motion'] = motion.as_dict()
    last_fast.clear()
    last_fast.update(n_frames=len(frames), n_groups=len(group_sizes), group_sizes=group_sizes, seconds=time_for_all,
                     seconds_load=stage['load'], seconds_issue=stage['issue'], seconds_wait=stage['wait'],
                     seconds_write=stage['write'], png_bytes=files.png_bytes, png_huffman=png_huffman, **cleaned)
    log.info('Test {0}: {1} images in {2} groups, total test time {3} sec'.format(seq_name, len(frames), len(group_sizes),
                                                                                 time_for_all))
    if annotations is None:
        return None
    score = _sequence_score(frames, counts_host, radius, time_for_all, seq_name, **cleaned)
    last_score.clear()
    last_score.update(score)
    return score


def _first_sample_tensors(first_sample):
    """(image [1,3,H,W], gt [1,1,H,W]) float32 of the annotated training frame, as the loaders' minibatches hold them."""
    image, gt = torch.as_tensor(first_sample['image']).float(), torch.as_tensor(first_sample['gt']).float()
    if image.dim() == 3:
        image = image[None]
    while gt.dim() < 4:
        gt = gt[None]
    if image.dim() != 4 or image.shape[0] != 1 or gt.dim() != 4 or tuple(gt.shape[:2]) != (1, 1) \
            or tuple(gt.shape[2:]) != tuple(image.shape[2:]):
        raise ValueError('test_adaptive: first_sample holds one frame, image [1,3,H,W] and gt [1,1,H,W]; got {} and {}'.format(
            tuple(image.shape), tuple(gt.shape)))
    return image.contiguous(), gt.contiguous()


def adapt_accumulate(net, first_image, first_gt, x, label, void, weights, with_first: bool = True, no_void=None) -> None:
    """One accumulation of online adaptation on the device: adds ``weights[0] * grad L(first_image, first_gt) + weights[1] *
    grad L(x, label, void)`` (``size_average=False``; ``weights``: float32 [2] on the device) to the ``.grad`` of the net's
    parameters.  Where both frames have one size and H W is a multiple of 4 it is ONE 2-frame pass through the per-frame
    loss - ``void`` zero for the first frame (``no_void``: that map, made here when None), the backward seed ``weights`` -,
    else two passes.  ``with_first`` False: the first frame is not forwarded at all.  No host synchronisation."""
    from layers.osvos_layers import (class_balanced_cross_entropy_loss as cbce,
                                     class_balanced_cross_entropy_loss_frames as cbce_frames)
    h, w = int(x.shape[2]), int(x.shape[3])
    with torch.enable_grad():
        if with_first and (h * w) % 4 == 0 and tuple(first_image.shape) == tuple(x.shape):
            if no_void is None:
                no_void = torch.zeros_like(void)
            out = net.forward(torch.cat([first_image, x]))[-1]
            losses = cbce_frames(out, torch.cat([first_gt, label]), size_average=False, void_pixels=torch.cat([no_void, void]))
            losses.backward(weights)
            return
        if with_first:
            cbce(net.forward(first_image)[-1], first_gt, size_average=False).backward(weights[0])
        cbce(net.forward(x)[-1], label, size_average=False, void_pixels=void).backward(weights[1])


def test_adaptive(net_provider, data_loader, save_dir: Path, first_sample, adapt, annotations: Optional[Callable] = None,
                  seq_name: Optional[str] = None, png_huffman: str = 'fixed', trace: Optional[list] = None) -> Optional[dict]:
    """The test pass with online adaptation (as in OnAVOS): while the sequence is segmented the net keeps taking fine-tune
    steps on each new frame against pseudo-labels made from its own output (util/online_adapt.py states them).
    ``adapt``: a ``fosvos_hip.options.AdaptOptions``.  ``first_sample``: the training frame's ``image`` and ``gt``.  Frames
    come one at a time, in order (a loader batch of more than one frame is refused).  The chain's first ``last_mask`` is
    ``first_sample['gt'] >= 0.5``; the optimizer is a fresh ``net_provider.get_optimizer(learning_rate=adapt.learning_rate)``.
    Per frame x:
      1. ``logits0 = net.forward(x)[-1]`` under ``no_grad``
      2. ``ops.adapt_labels(logits0, last_mask, adapt.pos_logit, adapt.neg_distance, adapt.erode)`` -> label, void, counts
      3. ``adapt.steps`` times: zero the gradients, accumulate ``first_weight * grad L(first frame, gt) + frame_weight *
         grad L(x, label, void)`` with ``size_average=False``, ``optimizer.step()``.  Where the first frame has x's size and
         H W is a multiple of 4 this is ONE 2-frame pass through the per-frame loss (``void`` zero for the first frame,
         backward seed ``[first_weight, frame_weight]``), else two passes; with ``first_weight == 0`` the first frame is
         not forwarded at all
      4. ``logits1 = net.forward(x)[-1]`` under ``no_grad``
      5. ``logits1`` through ``test_fast``'s device path: ``prob_bytes``, ``png_encode``, ``jf_counts`` into one counter
         tensor read back once, the files written one frame behind
      6. ``last_mask = logits1 >= 0``
    Nothing in the per-frame work synchronises with the host.  The class counts of ``adapt_labels`` land in a [n_frames,3]
    tensor copied once at the end; they go into ``last_fast`` and the score dict under 'adapt', beside the options.
    ``steps == 0`` performs no training call and constructs no optimizer: the files are ``test_fast``'s.
    THE NET LEAVES THE PASS ADAPTED: its weights are the ones after the last frame's last step (restoring them is not built;
    the caller reloads the snapshot where it needs the one-shot net again).
    ``trace`` (a list, or None) receives per frame a dict of the tensors the loop used, cloned: 'logits0', 'last_mask',
    'label', 'void' and 'logits1'.
    CPU logits (the stand-in nets of the CPU tests) take the numpy definitions and ``online_adapt.cbce_void_torch``, the way
    ``test_fast`` has a host branch.  Returns the score dict of ``test_fast`` with ``annotations``, else None."""
    from fosvos_hip.options import AdaptOptions
    from util import online_adapt, png_layout
    if not isinstance(adapt, AdaptOptions):
        raise ValueError('test_adaptive: adapt must be a fosvos_hip.options.AdaptOptions, got {!r}'.format(adapt))
    _check_png_huffman('test_adaptive', png_huffman)
    if trace is not None and not isinstance(trace, list):
        raise ValueError('test_adaptive: trace must be a list or None')
    first_image, first_gt = _first_sample_tensors(first_sample)
    log.info('Testing Network (adaptive, {} steps a frame)'.format(adapt.steps))
    net = net_provider.network
    optimizer = net_provider.get_optimizer(learning_rate=adapt.learning_rate) if adapt.steps > 0 else None
    pos_logit = adapt.pos_logit
    frames = _Frames(data_loader, save_dir)
    counts, radius = _Counters(frames.n_frames, 6), None
    adapt_counts = _Counters(frames.n_frames, 3)
    files = _FileSlots()
    pending = None   # the sent frame whose file is not written yet
    buffers = {}     # (h, w) -> (label, void) of the device labelling
    on_device = {}   # the first frame, its labels and the pass's constants on the logits' device, made at the first frame
    last_mask = None

    def train_steps(x, label, void):
        """Step 3 on the device."""
        for _ in range(adapt.steps):
            optimizer.zero_grad(set_to_none=False)
            adapt_accumulate(net, on_device['image'], on_device['gt'], x, label, void, on_device['weights'],
                             with_first=adapt.first_weight > 0, no_void=on_device['no_void'])
            optimizer.step()

    def train_steps_host(x, label, void):
        """Step 3 for CPU logits: the same sum of two losses as one torch-autograd expression per frame."""
        label_t, void_t = torch.from_numpy(label)[None, None], torch.from_numpy(void)[None, None]
        with torch.enable_grad():
            for _ in range(adapt.steps):
                optimizer.zero_grad(set_to_none=False)
                if adapt.first_weight > 0:
                    out = net.forward(first_image)[-1]
                    (adapt.first_weight * online_adapt.cbce_void_torch(out, first_gt.to(out.device), None, False)).backward()
                out = net.forward(x)[-1]
                (adapt.frame_weight * online_adapt.cbce_void_torch(out, label_t.to(out.device), void_t.to(out.device),
                                                                   False)).backward()
                optimizer.step()

    time_all_start = timeit.default_timer()
    for minibatch in data_loader:
        inputs, = gpu_handler.cast_cuda_if_possible([minibatch['image']])
        if int(inputs.shape[0]) != 1:
            raise ValueError('test_adaptive: frames come one at a time (the chain of masks and steps is sequential); the '
                             'loader yields batches of {}'.format(int(inputs.shape[0])))
        with torch.no_grad():
            logits0 = net.forward(inputs)[-1].detach().float().contiguous()
        h, w = int(logits0.shape[2]), int(logits0.shape[3])
        radius = davis_measures.default_radius(h, w)
        first, gt, paths = frames.add([minibatch], h, w, annotations)
        if first == 0 and tuple(first_gt.shape[2:]) != (h, w):
            raise ValueError('test_adaptive: first_sample is {}, the logits are {}'.format(tuple(first_gt.shape[2:]), (h, w)))
        if logits0.is_cuda:
            from fosvos_hip import ops
            device = logits0.device
            if not on_device:
                on_device['image'], on_device['gt'] = first_image.to(device), first_gt.to(device)
                on_device['weights'] = torch.tensor([adapt.first_weight, adapt.frame_weight], dtype=torch.float32,
                                                    device=device)
                on_device['no_void'] = torch.zeros((1, 1, h, w), dtype=torch.uint8, device=device)
                last_mask = (on_device['gt'][:, 0] >= 0.5).to(torch.uint8)
            if tuple(last_mask.shape) != (1, h, w):
                raise ValueError('test_adaptive: the frames changed their size from {} to {}'.format(
                    tuple(last_mask.shape[1:]), (h, w)))
            if (h, w) not in buffers:
                buffers[(h, w)] = (torch.empty((1, 1, h, w), dtype=torch.float32, device=device),
                                   torch.empty((1, 1, h, w), dtype=torch.uint8, device=device))
            label, void = buffers[(h, w)]
            ops.adapt_labels(logits0, last_mask, pos_logit, adapt.neg_distance, adapt.erode, label=label, void=void,
                             counts=adapt_counts.rows(first, 1, device))
            if adapt.steps > 0:
                train_steps(inputs, label, void)
                with torch.no_grad():
                    logits1 = net.forward(inputs)[-1].detach().float().contiguous()
            else:
                logits1 = logits0
            if trace is not None:
                trace.append({'logits0': logits0.clone(), 'last_mask': last_mask.clone(), 'label': label.clone(),
                              'void': void.clone(), 'logits1': logits1.clone()})
            with torch.no_grad():
                if annotations is not None:
                    ops.jf_counts(logits1, torch.from_numpy(gt).to(device), radius, out=counts.rows(first, 1, device))
                slot = files.take(1, h, w, ops.png_capacity(h, w), device)
                ops.png_encode(ops.prob_bytes(logits1), out=slot.files, lengths=slot.lengths, huffman=png_huffman)
                sent = slot.send(paths)
                last_mask = (logits1[:, 0] >= 0).to(torch.uint8)
            if pending is not None:
                files.retire(pending)  # the previous frame's file, while the device works on this frame
            pending = sent
        else:
            if last_mask is None:
                last_mask = (first_gt[0, 0].numpy() >= 0.5).astype(np.uint8)
            if last_mask.shape != (h, w):
                raise ValueError('test_adaptive: the frames changed their size from {} to {}'.format(last_mask.shape, (h, w)))
            x0 = np.ascontiguousarray(logits0[0, 0].numpy(), dtype=np.float32)
            label, void, adapt_counts.host[first] = online_adapt.adapt_labels(x0, last_mask, pos_logit, adapt.neg_distance,
                                                                              adapt.erode)
            if adapt.steps > 0:
                train_steps_host(inputs, label, void)
                with torch.no_grad():
                    logits1 = net.forward(inputs)[-1].detach().float().contiguous()
            else:
                logits1 = logits0
            if trace is not None:
                trace.append({'logits0': logits0.clone(), 'last_mask': torch.from_numpy(last_mask.copy())[None],
                              'label': torch.from_numpy(label.copy())[None, None],
                              'void': torch.from_numpy(void.copy())[None, None], 'logits1': logits1.clone()})
            x1 = logits1[0, 0].numpy().astype(np.float64)
            if frames.scored[first]:
                counts.host[first] = davis_measures.jf_counts_numpy(x1 >= 0, gt[0], radius)
            files.write(paths, [png_layout.encode(bytescale(1.0 / (1.0 + np.exp(-x1))), huffman=png_huffman)])
            last_mask = (logits1[0, 0].numpy() >= 0).astype(np.uint8)
    if pending is not None:
        files.retire(pending)
    counts_host, adapt_host = counts.read(len(frames)), adapt_counts.read(len(frames))
    time_for_all = timeit.default_timer() - time_all_start
    adapt_report = dict(adapt.as_dict(), counts=[[int(v) for v in row] for row in adapt_host])
    last_fast.clear()
    last_fast.update(n_frames=len(frames), n_groups=len(frames), group_sizes=[1] * len(frames), seconds=time_for_all,
                     png_bytes=files.png_bytes, png_huffman=png_huffman, adapt=adapt_report)
    log.info('Test {0}: {1} images adapted with {2} steps each, total test time {3} sec'.format(seq_name, len(frames),
                                                                                              adapt.steps, time_for_all))
    if annotations is None:
        return None
    score = _sequence_score(frames, counts_host, radius, time_for_all, seq_name, adapt=adapt_report)
    last_score.clear()
    last_score.update(score)
    return score


def test_objects(net_providers, data_loader, save_dir: Path, annotations: Optional[Callable] = None, group: int = 5,
                 seq_name: Optional[str] = None, forward_batch: int = 2, png_huffman: str = 'fixed',
                 palette=None, ensemble=None, crf=None, crf_joint: bool = False) -> Optional[dict]:
    """The test pass of a sequence with several objects: ``net_providers[k - 1]`` holds the net fine-tuned on object k
    against everything else.  ``test_fast``'s structure - groups of up to ``group`` frames uploaded once, ``forward_batch``
    frames a forward call, two buffer slots, ONE copy per group of files plus lengths, the host writing the previous group's
    files while the device works on this one - with every one of the K nets forwarding the same uploaded batch.  On the
    device ``ops.merge_objects`` gives each pixel to the object whose net answers highest, or to the background where no
    logit is >= 0 (util/object_merge.merge_labels), ``ops.png_encode_indexed`` turns the label maps into palette PNG files
    (util/png_layout.encode_indexed; ``palette``: uint8 [256,3], None = the DAVIS palette) written as
    ``<save_dir>/<seq>/<fname>.png``, and ``ops.jf_counts_labels`` takes J / F counts per object into one [n_frames,K,6]
    counter tensor read back once.  ``annotations(seq_name, fname)`` -> uint8 [H,W] object ids or None; without
    ``annotations`` the pass returns None.  CPU logits take the numpy path (``merge_labels``, ``encode_indexed``,
    ``jf_counts_labels_numpy``).
    The score dict (kept in ``last_score``): 'seq_name', 'radius', 'fnames', 'scored', 'n_objects', 'objects' - per object
    {'object_id', 'counts', 'J', 'F', 'J_stats', 'F_stats'} as ``test_scored`` forms them -, 'J_stats' / 'F_stats' - each
    statistic averaged over the objects -, 'J&F' and 'seconds'.  Toolkit parity unpinned, as for the single-object J / F.
    ``ensemble`` (an EnsembleOptions; None: nothing changes): the test-time ensemble of ``test_fast``.  The group's views are
    made ONCE and shared among the K nets; each net forwards them in view order and has its V answers merged
    (``ops.ensemble_merge``) before ``ops.merge_objects`` sees them.  The score dict then holds the options under
    'ensemble'.
    ``crf`` (a CrfOptions; None: nothing changes): the CRF of ``test_fast``, per net: each net's logits - merged behind an
    ensemble - go through ONE ``ops.crf_refine`` on the group's uploaded frames before ``ops.merge_objects`` sees them.  The
    score dict then holds the options under 'crf'.
    ``crf_joint`` (needs ``crf``; False: nothing changes): per group the K nets' logits - merged behind an ensemble - go through
    ONE ``ops.crf_labels`` on the group's uploaded frames, a joint CRF over the labels 0..K (util/label_crf.py states it; CPU
    tensors: ``label_crf.refine_labels_batch``), in the place of the K ``crf_refine`` calls AND of ``merge_objects``.  No host
    synchronisation is added.  The score dict then holds 'crf' and 'crf_joint': True."""
    from util import object_merge, png_layout
    _check_png_huffman('test_objects', png_huffman)
    _check_batching('test_objects', group, forward_batch)
    _check_ensemble('test_objects', ensemble)
    _check_crf('test_objects', crf)
    if not isinstance(crf_joint, bool):
        raise ValueError('test_objects: crf_joint must be a bool, got {!r}'.format(crf_joint))
    if crf_joint and crf is None:
        raise ValueError('test_objects: crf_joint is the joint form of the CRF: it needs crf (a CrfOptions)')
    nets = [p.network for p in net_providers]
    n_obj = len(nets)
    if not 1 <= n_obj <= object_merge.MAX_OBJECTS:
        raise ValueError('test_objects: {} nets, outside [1, {}]'.format(n_obj, object_merge.MAX_OBJECTS))
    log.info('Testing Network ({} objects)'.format(n_obj))
    frames = _Frames(data_loader, save_dir)
    counts, radius = _Counters(frames.n_frames, n_obj, 6), None
    palette_dev, palette_host = None, (None if palette is None else np.asarray(palette, dtype=np.uint8))
    files = _FileSlots()
    pending = None   # the sent group whose files are not written yet
    n_groups = 0
    time_all_start = timeit.default_timer()
    with torch.no_grad():
        for minibatches in _frame_groups(data_loader, group):
            images = minibatches[0]['image'] if len(minibatches) == 1 else torch.cat([m['image'] for m in minibatches])
            inputs, = gpu_handler.cast_cuda_if_possible([images])
            n = int(inputs.shape[0])
            views = None if ensemble is None else _ensemble_inputs(inputs, ensemble)  # made once, shared among the nets
            # every net forwards the same uploaded batch
            logits = [_ensemble_logits(net, inputs, forward_batch, ensemble, views) for net in nets]
            if crf is not None and not crf_joint:
                logits = [_crf_logits(inputs, x, crf) for x in logits]
            h, w = int(logits[0].shape[2]), int(logits[0].shape[3])
            first, gt, paths = frames.add(minibatches, h, w, annotations, ids=True)
            n_groups += 1
            radius = davis_measures.default_radius(h, w)
            if logits[0].is_cuda:
                from fosvos_hip import ops
                device = logits[0].device
                if palette_host is not None and palette_dev is None:
                    palette_dev = torch.from_numpy(palette_host).to(device)
                labels = _crf_joint_labels(inputs, logits, crf) if crf_joint else ops.merge_objects(logits)
                if annotations is not None:
                    ops.jf_counts_labels(labels, torch.from_numpy(gt).to(device), n_obj, radius,
                                         out=counts.rows(first, n, device))
                slot = files.take(n, h, w, ops.png_indexed_capacity(h, w), device)
                ops.png_encode_indexed(labels, palette_dev, out=slot.files, lengths=slot.lengths, huffman=png_huffman)
                sent = slot.send(paths)
                if pending is not None:
                    files.retire(pending)  # the previous group's files, while the device works on this group
                pending = sent
            else:
                labels = _crf_joint_labels(inputs, logits, crf) if crf_joint else \
                    object_merge.merge_labels([x[:, 0].numpy() for x in logits])
                blobs = []
                for index in range(n):
                    if annotations is not None:
                        counts.host[first + index] = object_merge.jf_counts_labels_numpy(labels[index], gt[index], n_obj,
                                                                                         radius)
                    blobs.append(png_layout.encode_indexed(labels[index], palette_host, huffman=png_huffman))
                files.write(paths, blobs)
        if pending is not None:
            files.retire(pending)
    counts_host = counts.read(len(frames))
    time_for_all = timeit.default_timer() - time_all_start
    log.info('Test {0}: {1} images of {2} objects in {3} groups, {4} PNG bytes, total test time {5} sec'.format(
        seq_name, len(frames), n_obj, n_groups, files.png_bytes, time_for_all))
    if annotations is None:
        return None
    keep = np.asarray(frames.scored, dtype=bool)
    objects = [object_merge.object_score(counts_host[:, k], keep, k + 1) for k in range(n_obj)]
    j_stats = object_merge.mean_statistics([o['J_stats'] for o in objects])
    f_stats = object_merge.mean_statistics([o['F_stats'] for o in objects])
    score = {**frames.score_head(seq_name, radius), 'n_objects': n_obj, 'objects': objects, 'J_stats': j_stats,
             'F_stats': f_stats, 'J&F': (j_stats['mean'] + f_stats['mean']) / 2, 'seconds': time_for_all}
    if ensemble is not None:
        score['ensemble'] = ensemble.as_dict()
    if crf is not None:
        score['crf'] = crf.as_dict()
    if crf_joint:
        score['crf_joint'] = True
    last_score.clear()
    last_score.update(score)
    return score


def format_score(score: dict) -> str:
    js, fs = score['J_stats'], score['F_stats']
    objects = ' (mean over {} objects)'.format(score['n_objects']) if 'n_objects' in score else ''
    return ('J mean {:.4f} recall {:.4f} decay {:.4f}, F mean {:.4f} recall {:.4f} decay {:.4f}, J&F {:.4f}{}'
            .format(js['mean'], js['recall'], js['decay'], fs['mean'], fs['recall'], fs['decay'], score['J&F'], objects))


def write_scores(path: Path, score: dict) -> None:
    """The per-frame values and the statistics of one sequence as YAML (plain lists, numbers and None)."""
    import yaml
    with open(str(path), 'w') as fh:
        yaml.safe_dump(dict(score), fh, default_flow_style=False)
