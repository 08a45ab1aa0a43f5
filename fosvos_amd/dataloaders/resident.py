"""The one-shot training sample, resident on the device.

In a sequence run the reference's training loader holds exactly ONE sample - frame 00000 and its mask
(src/dataloaders/davis_2016.py:72-83) - behind ``DataLoader(db_train, batch_size=1, shuffle=True, num_workers=1)``
(src/util/io_helper.py:62-70): every iteration starts a worker process, decodes the JPEG and the PNG, draws a flip
(src/dataloaders/custom_transforms.py:96-111) and one of three scales (:63-93), resamples, and copies the result to the
device: several milliseconds per iteration in front of a 0.8 ms training step.  The augmentation has only
2 flips x 3 scales = SIX outcomes, all determined by that one sample.

``ResidentOneShotLoader`` decodes the sample once, builds the six variants once with the SAME transform code, keeps them
on the device, and per epoch draws the variant with the reference pipeline's random numbers in the reference pipeline's
order, so that it yields, tensor for tensor, what the per-iteration DataLoader yields under the same torch seed:

  * creating the loader's iterator draws the workers' base seed from torch's default generator
    (``torch.empty((), dtype=torch.int64).random_()``);
  * worker 0 seeds Python's ``random`` with ``base_seed + 0``; fetching the sample then calls
    ``random.random()`` (flip if < 0.5) and ``random.randint(0, 2)`` (index into the scales), in that order;
  * the shuffling sampler draws one more int64 from the default generator when its first index is asked for.

``ResidentTrainSetLoader`` does the same for the whole offline training set, which has far too many samples to keep six
fp32 variants of each: it keeps every decoded frame and mask as uint8 on the device and runs flip + rescale per draw in
one HIP launch (fosvos_hip.ops.augment_sample, bit for bit custom_transforms.resize), with the same random numbers
(the per-index draws of the shuffled order come from the sampler, the flip / scale draws from worker 0's ``random``).
"""
import random
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import RandomSampler
from torch.utils.data.distributed import DistributedSampler

from dataloaders import custom_transforms
from util.logger import get_logger

log = get_logger(__file__)


class ResidentOneShotLoader(object):
    """Drop-in for the training DataLoader of a one-sample dataset: ``len() == 1``, each ``iter()`` yields one minibatch
    dict (``image`` [1,3,h,w], ``gt`` [1,1,h,w] on ``device``, ``seq_name`` / ``fname`` lists as default_collate builds them)."""

    def __init__(self, dataset, device: Optional[torch.device] = None, scales: Sequence[float] = (0.5, 0.8, 1)):
        if len(dataset) != 1:
            raise ValueError("ResidentOneShotLoader holds the single sample of a one-shot sequence run, got %d samples"
                             % len(dataset))
        if dataset.transform is not None:
            raise ValueError("pass the dataset without its transform: the loader applies flip / rescale / ToTensor itself")
        self.dataset = dataset
        self.scales = list(scales)
        self.device = device if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        base = dataset[0]  # decoded once
        self._meta = {k: [base[k]] for k in ("seq_name", "fname") if k in base}
        to_tensor = custom_transforms.ToTensor()
        self.variants: Dict[tuple, Dict[str, torch.Tensor]] = {}
        for flip in (False, True):
            for si, sc in enumerate(self.scales):
                sample = {"image": base["image"], "gt": base["gt"]}
                if flip:  # custom_transforms.RandomHorizontalFlip with the draw fixed
                    sample = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in sample.items()}
                sample = {k: custom_transforms.resize(v, sc, sc) for k, v in sample.items()}  # custom_transforms.Resize
                sample = to_tensor(sample)
                self.variants[(flip, si)] = {k: v.unsqueeze(0).to(self.device) for k, v in sample.items()}
        self.draws: List[tuple] = []  # (flip, scale index) of every epoch so far

    def __len__(self) -> int:
        return 1

    def __iter__(self):
        # _BaseDataLoaderIter.__init__: the workers' base seed, from torch's default generator
        base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        rng = random.Random(base_seed + 0)        # worker 0: random.seed(base_seed + worker_id)
        flip = rng.random() < 0.5                 # RandomHorizontalFlip.__call__
        si = rng.randint(0, len(self.scales) - 1)  # Resize.__call__
        torch.empty((), dtype=torch.int64).random_()  # RandomSampler.__iter__: its own seed, drawn at the first index
        self.draws.append((flip, si))
        batch = dict(self.variants[(flip, si)])
        batch.update(self._meta)
        yield batch


_ALIGN = 16  # byte alignment of every frame / mask inside the resident buffers


class ResidentTrainSetLoader(object):
    """Drop-in for the offline training DataLoader (src/util/io_helper.py:62-70: batch 1, shuffled, flip + rescale) over
    a whole DAVIS2016 training split.  Every sample is decoded ONCE (the dataset's own read / ``inputRes`` path, on a pool
    of at most 16 host threads); the uint8 frames and masks stay on ``device`` with the resampling tables of every
    (source size, scale); each iteration replays the DataLoader's draws and launches one kernel, with no host->device
    copy and no device->host sync.  It yields what ``default_collate`` builds (``image`` [1,3,h,w], ``gt`` [1,1,h,w],
    ``seq_name`` / ``fname`` one-element lists), tensor for tensor what the DataLoader yields under the same torch seed.

    shard = (rank, world): the DataLoader over a DistributedSampler(shuffle=True) of the data-parallel factory
    (``sampler.set_epoch`` picks the epoch's order, as ``train_offline._train`` does).  On a CPU ``device`` the numpy
    transforms run on the cached decoded arrays instead of the kernel (the same values; that path needs no GPU)."""

    def __init__(self, dataset, device: Optional[torch.device] = None, shard: Optional[Tuple[int, int]] = None,
                 batch_size: int = 1, scales: Sequence[float] = (0.5, 0.8, 1), threads: int = 16):
        if batch_size != 1:
            raise ValueError("ResidentTrainSetLoader yields batches of one sample (frames of different scales cannot be "
                             "collated), got batch_size=%d" % batch_size)
        if dataset.transform is not None:
            raise ValueError("pass the dataset without its transform: the loader applies flip / rescale / ToTensor itself")
        n = len(dataset)
        self.dataset = dataset
        self.scales = list(scales)
        self.device = torch.device(device) if device is not None else \
            torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if shard is None:
            self.sampler = RandomSampler(range(n))  # what DataLoader(shuffle=True) builds
        else:
            self.sampler = DistributedSampler(range(n), num_replicas=shard[1], rank=shard[0], shuffle=True)
        self._meta = [([dataset.seq_list[i]], [dataset.fname_list[i]]) for i in range(n)]

        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=max(1, min(int(threads), 16, n))) as pool:
            raw = list(pool.map(dataset.read_raw, range(n)))
        raw = [(np.array(img, dtype=np.uint8, order="C"),  # (PIL's arrays are read-only: own copies)
                np.zeros(img.shape[:2], np.uint8) if lab is None else np.array(lab, dtype=np.uint8, order="C"),
                lab is not None) for img, lab in raw]
        self.decode_seconds = time.perf_counter() - t0
        self.sizes = [tuple(int(v) for v in img.shape[:2]) for img, _, _ in raw]

        if self.device.type == "cpu":
            self._raw = raw
            self.device_bytes = 0
        else:
            self._to_device(dataset, raw)
        log.info("ResidentTrainSetLoader: %d samples decoded in %.2f s, %.1f MB held on %s"
                 % (n, self.decode_seconds, self.device_bytes / 2 ** 20, self.device))

    def _to_device(self, dataset, raw) -> None:
        dev = self.device
        # one uint8 buffer of frames and one of masks (sizes may differ from sample to sample)
        self._offsets, f_total, m_total = [], 0, 0
        for img, lab, _ in raw:
            self._offsets.append((f_total, m_total))
            f_total += -(-img.size // _ALIGN) * _ALIGN
            m_total += -(-lab.size // _ALIGN) * _ALIGN
        self._frames = torch.empty(f_total, dtype=torch.uint8, device=dev)
        self._masks = torch.empty(m_total, dtype=torch.uint8, device=dev)
        gt_luts = np.zeros((len(raw), 256), dtype=np.float32)
        for i, ((img, lab, labelled), (fo, mo)) in enumerate(zip(raw, self._offsets)):
            self._frames[fo:fo + img.size].copy_(torch.from_numpy(img.reshape(-1)))
            self._masks[mo:mo + lab.size].copy_(torch.from_numpy(lab.reshape(-1)))
            if labelled:  # DAVIS2016.convert_raw: label / float32(max(label.max(), 1e-8)); hidden annotations stay 0
                gt_luts[i] = np.arange(256, dtype=np.float32) / np.float32(max(float(lab.max()), 1e-8))
        self._gt_luts = torch.from_numpy(gt_luts).to(dev)
        # DAVIS2016.convert_raw on every byte value of every channel: u8 - mean
        ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
        img_lut, _ = dataset.convert_raw(ramp, None)
        self._img_lut = torch.from_numpy(np.ascontiguousarray(img_lut.reshape(256, 3))).to(dev)
        # resampling tables per (source size, scale), all built here: none crosses to the device while iterating
        self._plans: Dict[tuple, tuple] = {}
        for (h, w) in sorted(set(self.sizes)):
            for si, sc in enumerate(self.scales):
                plan = custom_transforms.resize_plan(h, w, sc, sc)
                tables = None
                if not plan["copy"]:
                    tables = tuple(torch.from_numpy(np.ascontiguousarray(plan[k], dtype=dt)).to(dev) for k, dt in (
                        ("col_taps", np.int32), ("col_w", np.float32), ("row_taps", np.int32), ("row_w", np.float32),
                        ("col_near", np.int32), ("row_near", np.int32)))
                self._plans[(h, w, si)] = (plan["oh"], plan["ow"], tables)
        self.device_bytes = sum(t.numel() * t.element_size() for t in
                                [self._frames, self._masks, self._gt_luts, self._img_lut] +
                                [t for _, _, tabs in self._plans.values() for t in (tabs or ())])

    def __len__(self) -> int:
        return len(self.sampler)

    def __iter__(self):
        # _BaseDataLoaderIter.__init__: the workers' base seed, from torch's default generator
        base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        rng = random.Random(base_seed + 0)        # worker 0: random.seed(base_seed + worker_id)
        for idx in self.sampler:                  # a RandomSampler draws its own seed at the first index
            flip = rng.random() < 0.5             # RandomHorizontalFlip.__call__
            si = rng.randint(0, len(self.scales) - 1)  # Resize.__call__
            yield self.sample(idx, flip, si)

    def sample(self, idx: int, flip: bool, si: int) -> dict:
        """The minibatch of sample ``idx`` with the draws (flip, scale index) fixed."""
        seq, fname = self._meta[idx]
        if self.device.type == "cpu":
            img, lab, labelled = self._raw[idx]
            image, gt = self.dataset.convert_raw(img, lab if labelled else None)
            sample = {"image": image, "gt": gt}
            if flip:  # custom_transforms.RandomHorizontalFlip with the draw fixed
                sample = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in sample.items()}
            sc = self.scales[si]
            sample = custom_transforms.ToTensor()({k: custom_transforms.resize(v, sc, sc) for k, v in sample.items()})
            return {"image": sample["image"].unsqueeze(0), "gt": sample["gt"].unsqueeze(0), "seq_name": list(seq),
                    "fname": list(fname)}
        from fosvos_hip import ops
        h, w = self.sizes[idx]
        fo, mo = self._offsets[idx]
        oh, ow, tables = self._plans[(h, w, si)]
        image = torch.empty((1, 3, oh, ow), dtype=torch.float32, device=self.device)
        gt = torch.empty((1, 1, oh, ow), dtype=torch.float32, device=self.device)
        ops.augment_sample(self._frames[fo:fo + h * w * 3].view(h, w, 3), self._masks[mo:mo + h * w].view(h, w), flip,
                           self._img_lut, self._gt_luts[idx], image, gt, tables)
        return {"image": image, "gt": gt, "seq_name": list(seq), "fname": list(fname)}
