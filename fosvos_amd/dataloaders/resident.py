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

``rotate=RotateOptions(...)`` (opt-in, both loaders): ``ScaleNRotate`` stands in place of ``Resize``.  Its draw is continuous,
so nothing can be precomputed: both loaders keep the uint8 sample(s) and the lookup tables on the device, replay per draw
the flip's ``random()`` and then ScaleNRotate's two draws (``random()`` twice for ranges, ``randint`` twice for lists), and
launch fosvos_hip.ops.warp_sample (bit for bit custom_transforms.warp_affine) into fresh tensors of the frame's own size.

``lucid=LucidOptions(...)`` (opt-in, the one-shot loader only, not together with ``rotate``): the object moves against its
background (dataloaders/lucid.py).  The loader paints the object out once on the host, keeps frame, filled background, mask
and tables on the device, replays per epoch the flip's ``random()`` and the eleven draws of ``LucidDream.draw``, and launches
fosvos_hip.ops.lucid_sample (bit for bit ``lucid.compose``) into fresh tensors.  There is no host DataLoader to replay: the
definition is this loader on a CPU device.
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


def _value_tables(dataset, labels):
    """(img_lut [256,3], gt_luts [n,256]) fp32 on the host: DAVIS2016.convert_raw on every byte value - u8 - mean per channel,
    u8 / max(label) per sample; ``labels``: each sample's uint8 mask, or None where the annotation is hidden (gt stays 0)."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut, _ = dataset.convert_raw(ramp, None)
    gt_luts = np.zeros((len(labels), 256), dtype=np.float32)
    for i, lab in enumerate(labels):
        if lab is not None:  # label / float32(max(label.max(), 1e-8))
            gt_luts[i] = np.arange(256, dtype=np.float32) / np.float32(max(float(lab.max()), 1e-8))
    return np.ascontiguousarray(img_lut.reshape(256, 3)), gt_luts


def _rotated_on_host(dataset, img, lab, transform, flip: bool, rot: float, sc: float) -> Dict[str, torch.Tensor]:
    """RandomHorizontalFlip, ScaleNRotate and ToTensor with the draws fixed, in numpy: ``image`` [1,3,h,w], ``gt`` [1,1,h,w]."""
    image, gt = dataset.convert_raw(img, lab)
    sample = {"image": image, "gt": gt}
    if flip:
        sample = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in sample.items()}
    sample = custom_transforms.ToTensor()(transform.apply(sample, rot, sc))
    return {k: v.unsqueeze(0) for k, v in sample.items()}


def _rotated_on_device(frame, mask, img_lut, gt_lut, transform, workspace, flip: bool, rot: float, sc: float):
    """The same two tensors from the resident bytes: one ops.warp_sample call (two launches with ``renormalize``)."""
    from fosvos_hip import ops
    h, w = int(frame.shape[0]), int(frame.shape[1])
    image = torch.empty((1, 3, h, w), dtype=torch.float32, device=frame.device)
    gt = torch.empty((1, 1, h, w), dtype=torch.float32, device=frame.device)
    ops.warp_sample(frame, mask, flip, custom_transforms.rotation_matrix((w / 2, h / 2), rot, sc), img_lut, gt_lut, image, gt,
                    renormalize=transform.renormalize, workspace=workspace)
    return {"image": image, "gt": gt}


def _warp_workspace(transform, sizes, device) -> Optional[torch.Tensor]:
    """The one workspace of a rotating loader (only the reference's renormalisation needs one): the largest frame's."""
    if not transform.renormalize:
        return None
    from fosvos_hip import ops
    return torch.empty(max(ops.warp_workspace_bytes(h, w) for h, w in sizes), dtype=torch.uint8, device=device)


class ResidentOneShotLoader(object):
    """Drop-in for the training DataLoader of a one-sample dataset: ``len() == 1``, each ``iter()`` yields one minibatch
    dict (``image`` [1,3,h,w], ``gt`` [1,1,h,w] on ``device``, ``seq_name`` / ``fname`` lists as default_collate builds them)."""

    def __init__(self, dataset, device: Optional[torch.device] = None, scales: Sequence[float] = (0.5, 0.8, 1),
                 rotate=None, lucid=None):
        """rotate: a fosvos_hip.options.RotateOptions - ScaleNRotate in place of the rescale.  The loader then keeps the
        sample as bytes and warps it per draw (``draws`` records (flip, rot, sc)); ``variants`` holds the one tensor pair
        that is still fixed, the unaugmented frame ((False, 0), ``scales == [1]``), which online adaptation trains on.
        lucid: a fosvos_hip.options.LucidOptions (not together with ``rotate``) - the object moves against its background
        (dataloaders/lucid.py).  The loader paints the object out once on the host (``lucid.fill_background``), keeps frame,
        filled background, mask and the tables on the device, replays per epoch the flip's ``random()`` and then the eleven
        draws of ``LucidDream.draw``, and composes with one fosvos_hip.ops.lucid_sample call (on a CPU device:
        ``lucid.compose``, the same bits); ``draws`` records (flip, draws) and ``variants`` holds the unaugmented frame."""
        if len(dataset) != 1:
            raise ValueError("ResidentOneShotLoader holds the single sample of a one-shot sequence run, got %d samples"
                             % len(dataset))
        if dataset.transform is not None:
            raise ValueError("pass the dataset without its transform: the loader applies flip / rescale / ToTensor itself")
        if rotate is not None and lucid is not None:
            raise ValueError("ResidentOneShotLoader: rotate and lucid both stand in place of the rescale: pass one of them")
        self.dataset = dataset
        self.scales = list(scales)
        self.device = device if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.rotate = rotate
        self.lucid = lucid
        self.draws: List[tuple] = []  # (flip, scale index) of every epoch so far; rotating: (flip, rot, sc); lucid: (flip, draws)
        self.variants: Dict[tuple, Dict[str, torch.Tensor]] = {}
        to_tensor = custom_transforms.ToTensor()
        if rotate is not None or lucid is not None:
            self.device = torch.device(self.device)
            self.scales = [1]
            img, lab = dataset.read_raw(0)  # decoded once
            self._raw = (np.array(img, dtype=np.uint8, order="C"),
                         None if lab is None else np.array(lab, dtype=np.uint8, order="C"))
            self._meta = {"seq_name": [dataset.seq_list[0]], "fname": [dataset.fname_list[0]]}
            plain = to_tensor(dict(zip(("image", "gt"), dataset.convert_raw(*self._raw))))
            self.variants[(False, 0)] = {k: v.unsqueeze(0).to(self.device) for k, v in plain.items()}
            img, lab = self._raw
            img_lut, gt_luts = _value_tables(dataset, [lab])
            mask = np.zeros(img.shape[:2], np.uint8) if lab is None else lab
            if rotate is not None:
                self._transform = rotate.transform()
            else:
                from dataloaders import lucid as lucid_rules
                self._dream = lucid.dream()
                self._host = (img, lucid_rules.fill_background(img, mask, lucid.dilate, lucid.smooth), mask, img_lut, gt_luts[0])
                box = lucid_rules.mask_box(mask)  # None: an empty or hidden annotation - no object
                self._boxes = {False: box, True: lucid_rules.mirrored_box(box, img.shape[1])}
            if self.device.type != "cpu":
                self._frame = torch.from_numpy(img).to(self.device)
                self._mask = torch.from_numpy(mask).to(self.device)
                self._img_lut, self._gt_lut = torch.from_numpy(img_lut).to(self.device), torch.from_numpy(gt_luts[0]).to(self.device)
                if rotate is not None:
                    self._workspace = _warp_workspace(self._transform, [img.shape[:2]], self.device)
                else:
                    self._background = torch.from_numpy(self._host[1]).to(self.device)
            return
        base = dataset[0]  # decoded once
        self._meta = {k: [base[k]] for k in ("seq_name", "fname") if k in base}
        for flip in (False, True):
            for si, sc in enumerate(self.scales):
                sample = {"image": base["image"], "gt": base["gt"]}
                if flip:  # custom_transforms.RandomHorizontalFlip with the draw fixed
                    sample = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in sample.items()}
                sample = {k: custom_transforms.resize(v, sc, sc) for k, v in sample.items()}  # custom_transforms.Resize
                sample = to_tensor(sample)
                self.variants[(flip, si)] = {k: v.unsqueeze(0).to(self.device) for k, v in sample.items()}

    def __len__(self) -> int:
        return 1

    def __iter__(self):
        # _BaseDataLoaderIter.__init__: the workers' base seed, from torch's default generator
        base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        rng = random.Random(base_seed + 0)        # worker 0: random.seed(base_seed + worker_id)
        flip = rng.random() < 0.5                 # RandomHorizontalFlip.__call__
        if self.rotate is not None:
            rot, sc = self._transform.draw(rng)   # ScaleNRotate.__call__: the angle's draw, then the zoom's
            torch.empty((), dtype=torch.int64).random_()  # RandomSampler.__iter__ (below)
            self.draws.append((flip, rot, sc))
            yield self.sample(flip, rot, sc)
            return
        if self.lucid is not None:
            draws = self._dream.draw(rng)         # the eleven draws, in lucid.DRAWS' order
            torch.empty((), dtype=torch.int64).random_()  # RandomSampler.__iter__ (below)
            self.draws.append((flip, draws))
            yield self.composed(flip, draws)
            return
        si = rng.randint(0, len(self.scales) - 1)  # Resize.__call__
        torch.empty((), dtype=torch.int64).random_()  # RandomSampler.__iter__: its own seed, drawn at the first index
        self.draws.append((flip, si))
        batch = dict(self.variants[(flip, si)])
        batch.update(self._meta)
        yield batch

    def sample(self, flip: bool, rot: float, sc: float) -> dict:
        """The minibatch of a rotating loader with the draws (flip, angle, zoom) fixed."""
        if self.device.type == "cpu":
            batch = _rotated_on_host(self.dataset, *self._raw, self._transform, flip, rot, sc)
        else:
            batch = _rotated_on_device(self._frame, self._mask, self._img_lut, self._gt_lut, self._transform,
                                       self._workspace, flip, rot, sc)
        batch.update({k: list(v) for k, v in self._meta.items()})
        return batch

    def composed(self, flip: bool, draws) -> dict:
        """The minibatch of a lucid loader with the draws (flip, the eleven of ``lucid.DRAWS``) fixed."""
        h, w = self._host[0].shape[:2]
        m_bg, m_fg, gain, bias = self._dream.matrices(draws, self._boxes[bool(flip)], (h, w))
        if self.device.type == "cpu":
            from dataloaders import lucid as lucid_rules
            image, gt = lucid_rules.compose(*self._host[:3], *self._host[3:], flip, m_bg, m_fg, gain, bias)
            batch = {k: v.unsqueeze(0) for k, v in custom_transforms.ToTensor()({"image": image, "gt": gt}).items()}
        else:
            from fosvos_hip import ops
            batch = {"image": torch.empty((1, 3, h, w), dtype=torch.float32, device=self.device),
                     "gt": torch.empty((1, 1, h, w), dtype=torch.float32, device=self.device)}
            ops.lucid_sample(self._frame, self._background, self._mask, flip, m_bg, m_fg, gain, bias, self._img_lut,
                             self._gt_lut, batch["image"], batch["gt"])
        batch.update({k: list(v) for k, v in self._meta.items()})
        return batch


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
    transforms run on the cached decoded arrays instead of the kernel (the same values; that path needs no GPU).

    rotate: a fosvos_hip.options.RotateOptions - ScaleNRotate in place of the rescale, one ops.warp_sample call per draw;
    every sample keeps its own size and ``draws`` records (flip, rot, sc)."""

    def __init__(self, dataset, device: Optional[torch.device] = None, shard: Optional[Tuple[int, int]] = None,
                 batch_size: int = 1, scales: Sequence[float] = (0.5, 0.8, 1), threads: int = 16, rotate=None, lucid=None):
        if lucid is not None:
            raise ValueError("ResidentTrainSetLoader: lucid is built for the one-shot sample only (ResidentOneShotLoader); the "
                             "offline set would need a filled background per training frame")
        if batch_size != 1:
            raise ValueError("ResidentTrainSetLoader yields batches of one sample (frames of different scales cannot be "
                             "collated), got batch_size=%d" % batch_size)
        if dataset.transform is not None:
            raise ValueError("pass the dataset without its transform: the loader applies flip / rescale / ToTensor itself")
        n = len(dataset)
        self.dataset = dataset
        self.scales = list(scales)
        self.rotate = rotate
        self._transform = None if rotate is None else rotate.transform()
        self.draws: List[tuple] = []  # rotating: (flip, rot, sc) of every draw so far
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
        for (img, lab, _), (fo, mo) in zip(raw, self._offsets):
            self._frames[fo:fo + img.size].copy_(torch.from_numpy(img.reshape(-1)))
            self._masks[mo:mo + lab.size].copy_(torch.from_numpy(lab.reshape(-1)))
        # DAVIS2016.convert_raw on every byte value: u8 - mean per channel, u8 / max(label) per frame (hidden: gt stays 0)
        img_lut, gt_luts = _value_tables(dataset, [lab if labelled else None for _, lab, labelled in raw])
        self._gt_luts = torch.from_numpy(gt_luts).to(dev)
        self._img_lut = torch.from_numpy(img_lut).to(dev)
        # resampling tables per (source size, scale), all built here: none crosses to the device while iterating
        self._plans: Dict[tuple, tuple] = {}
        self._workspace = None
        if self._transform is not None:  # a warp reads no table; the reference's renormalisation needs a workspace
            self._workspace = _warp_workspace(self._transform, set(self.sizes), dev)
        for (h, w) in sorted(set(self.sizes)) if self._transform is None else ():
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
                                ([] if self._workspace is None else [self._workspace]) +
                                [t for _, _, tabs in self._plans.values() for t in (tabs or ())])

    def __len__(self) -> int:
        return len(self.sampler)

    def __iter__(self):
        # _BaseDataLoaderIter.__init__: the workers' base seed, from torch's default generator
        base_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        rng = random.Random(base_seed + 0)        # worker 0: random.seed(base_seed + worker_id)
        for idx in self.sampler:                  # a RandomSampler draws its own seed at the first index
            flip = rng.random() < 0.5             # RandomHorizontalFlip.__call__
            if self._transform is not None:
                rot, sc = self._transform.draw(rng)  # ScaleNRotate.__call__: the angle's draw, then the zoom's
                self.draws.append((flip, rot, sc))
                yield self.sample_rotated(idx, flip, rot, sc)
                continue
            si = rng.randint(0, len(self.scales) - 1)  # Resize.__call__
            yield self.sample(idx, flip, si)

    def sample_rotated(self, idx: int, flip: bool, rot: float, sc: float) -> dict:
        """The minibatch of sample ``idx`` of a rotating loader with the draws (flip, angle, zoom) fixed."""
        seq, fname = self._meta[idx]
        if self.device.type == "cpu":
            img, lab, labelled = self._raw[idx]
            batch = _rotated_on_host(self.dataset, img, lab if labelled else None, self._transform, flip, rot, sc)
        else:
            h, w = self.sizes[idx]
            fo, mo = self._offsets[idx]
            batch = _rotated_on_device(self._frames[fo:fo + h * w * 3].view(h, w, 3), self._masks[mo:mo + h * w].view(h, w),
                                       self._img_lut, self._gt_luts[idx], self._transform, self._workspace, flip, rot, sc)
        batch.update({"seq_name": list(seq), "fname": list(fname)})
        return batch

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
