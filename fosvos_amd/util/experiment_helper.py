"""Inference pass over a sequence (reference: src/util/experiment_helper.py:20-80): forward, sigmoid,
write probability PNGs; with ``eval_speeds`` time ``net.forward`` between device synchronisations
over 10 passes, dropping the first minibatch of each pass (the reference's protocol, :29-53,77-80;
no PNGs are written in that mode, as in the reference).

``test_scored`` (an extension: the reference leaves evaluation to an outside toolkit) is the same pass with the sigmoid,
the byte stretch and the DAVIS 2016 J / F counts computed on the device beside the logits (fosvos_prob_bytes,
fosvos_jf_counts); ``test`` itself keeps the reference's host path."""
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
# what the last call of test_scored() returned
last_score = {}


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


def _frame_annotation(annotations: Callable, seq: str, fname: str, h: int, w: int) -> Optional[np.ndarray]:
    ann = annotations(seq, fname)
    if ann is None:
        return None
    ann = np.asarray(ann)
    if ann.shape != (h, w):
        raise ValueError('annotation of {}/{} is {}, the logits are {}'.format(seq, fname, ann.shape, (h, w)))
    return (ann != 0).astype(np.uint8)


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
    n_frames = len(data_loader.dataset)
    fnames, seqs, scored = [], [], []
    counts_dev, counts_host, radius = None, np.zeros((n_frames, 6), dtype=np.int64), None
    time_all_start = timeit.default_timer()
    with torch.no_grad():
        for minibatch in data_loader:
            inputs, = gpu_handler.cast_cuda_if_possible([minibatch['image']])
            logits = net.forward(inputs)[-1].detach().float().contiguous()
            n, h, w = int(logits.shape[0]), int(logits.shape[2]), int(logits.shape[3])
            first = len(fnames)
            if first + n > n_frames:
                raise RuntimeError('the loader yields more frames than its dataset holds ({})'.format(n_frames))
            radius = davis_measures.default_radius(h, w)
            gt = np.zeros((n, h, w), dtype=np.uint8)
            for index in range(n):
                seq, fname = minibatch['seq_name'][index], minibatch['fname'][index]
                ann = _frame_annotation(annotations, seq, fname, h, w)
                if ann is not None:
                    gt[index] = ann
                seqs.append(seq)
                fnames.append(fname)
                scored.append(ann is not None)
            if logits.is_cuda:
                from fosvos_hip import ops
                if counts_dev is None:
                    counts_dev = torch.zeros((n_frames, 6), dtype=torch.int32, device=logits.device)
                ops.jf_counts(logits, torch.from_numpy(gt).to(logits.device), radius, out=counts_dev[first:first + n])
                png = ops.prob_bytes(logits).cpu().numpy() if write_png else None
            else:
                x = logits[:, 0].numpy().astype(np.float64)
                for index in range(n):
                    counts_host[first + index] = davis_measures.jf_counts_numpy(x[index] >= 0, gt[index], radius)
                png = np.stack([bytescale(1.0 / (1.0 + np.exp(-x[index]))) for index in range(n)]) if write_png else None
            if write_png:
                for index in range(n):
                    save_dir_seq = Path(save_dir) / seqs[first + index]
                    save_dir_seq.mkdir(parents=True, exist_ok=True)
                    Image.fromarray(png[index], mode='L').save(str(save_dir_seq / '{0}.png'.format(fnames[first + index])))
    if counts_dev is not None:
        counts_host = counts_dev.cpu().numpy().astype(np.int64)
    time_for_all = timeit.default_timer() - time_all_start
    counts_host = counts_host[:len(fnames)]
    j, f = davis_measures.jf_from_counts(counts_host) if len(fnames) else (np.zeros(0), np.zeros(0))
    keep = np.asarray(scored, dtype=bool)
    j_stats = davis_measures.sequence_statistics(j[keep])
    f_stats = davis_measures.sequence_statistics(f[keep])
    score = {'seq_name': seq_name if seq_name is not None else (seqs[0] if seqs else None),
             'radius': radius, 'fnames': list(fnames), 'scored': [bool(k) for k in keep],
             'counts': [[int(v) for v in row] if k else None for row, k in zip(counts_host, keep)],
             'J': [float(v) if k else None for v, k in zip(j, keep)],
             'F': [float(v) if k else None for v, k in zip(f, keep)],
             'J_stats': j_stats, 'F_stats': f_stats, 'J&F': (j_stats['mean'] + f_stats['mean']) / 2,
             'seconds': time_for_all}
    log.info('Test {0}: {1} images, {2} scored, total test time {3} sec'.format(seq_name, len(fnames), int(keep.sum()),
                                                                               time_for_all))
    last_score.clear()
    last_score.update(score)
    return score


def format_score(score: dict) -> str:
    js, fs = score['J_stats'], score['F_stats']
    return ('J mean {:.4f} recall {:.4f} decay {:.4f}, F mean {:.4f} recall {:.4f} decay {:.4f}, J&F {:.4f}'
            .format(js['mean'], js['recall'], js['decay'], fs['mean'], fs['recall'], fs['decay'], score['J&F']))


def write_scores(path: Path, score: dict) -> None:
    """The per-frame values and the statistics of one sequence as YAML (plain lists, numbers and None)."""
    import yaml
    with open(str(path), 'w') as fh:
        yaml.safe_dump(dict(score), fh, default_flow_style=False)
