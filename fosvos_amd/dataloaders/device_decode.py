"""The test pass's loader with the JPEG decode on the device (opt-in: ``io_helper.get_data_loader_test(device_decode=True)``,
``train_online.py --device-decode``).

``DeviceDecodeLoader`` iterates a ``DAVIS2016(mode='test', transform=None, inputRes=None)`` in order and yields the minibatch
dicts of ``DataLoader(dataset with ToTensor, shuffle=False)``: ``image`` float32 [b,3,H,W] - here ON THE DEVICE -, ``gt``
float32 [b,1,H,W] on the host, ``seq_name`` and ``fname`` lists.  The file bytes are read on the host and probed
(util/jpeg_read.probe); consecutive files the device decoder takes, of one shape and sampling, go to ``ops.jpeg_decode`` +
``ops.frame_prep`` on a stream of the loader's own, up to ``files_per_launch`` a call, one window ahead of the frames being
handed out; the consumer's stream waits for the window's event before a frame of it is yielded.  Every window has tensors
of its own, so a yielded tensor stays valid for as long as the caller holds it.

A file without restart markers is decoded by ONE wave, and a launch takes as long as its longest file whether it holds 8
files or 64 (measured: 67 ms for a 480x854 4:2:0 file of quality 92), so throughput comes from
the number of files in flight: ``files_per_launch`` defaults to 64, and consecutive windows alternate between two streams,
so that the window being decoded ahead runs beside the one in front of it instead of behind it.

The host path as it is (``dataset[idx]``, ``ToTensor``, moved to the device) takes every file whose probe is ``None``, grey
files (``read_bgr`` makes three channels of them), and files whose decode status comes back non-zero - so whatever PIL does
with a damaged file, raising included, happens here as well, when that frame's turn comes.  ``ops.frame_prep`` is bit for
bit ``convert_raw`` + ``ToTensor`` and the decoder byte for byte PIL's, so every ``image`` equals the host path's bit for bit.
Annotations stay with PIL on the host.
"""
import os

import numpy as np
import torch

from dataloaders import custom_transforms
from dataloaders.davis_2016 import MEANVAL, read_gray
from util import jpeg_read


def _key(plan):
    return plan.height, plan.width, plan.subsampling


class DeviceDecodeLoader(object):
    def __init__(self, dataset, batch_size: int = 1, device=None, files_per_launch: int = 64):
        if getattr(dataset, 'inputRes', None) is not None:
            raise ValueError('DeviceDecodeLoader: inputRes resizes on the host; the device decode takes frames as they are')
        if getattr(dataset, 'transform', None) is not None:
            raise ValueError('DeviceDecodeLoader: the dataset must come without a transform (the loader makes the tensors)')
        if tuple(np.float32(v) for v in dataset.meanval) != tuple(np.float32(v) for v in MEANVAL):
            raise ValueError('DeviceDecodeLoader: ops.frame_prep subtracts the DAVIS mean, the dataset another')
        if int(batch_size) < 1 or int(files_per_launch) < 1:
            raise ValueError('DeviceDecodeLoader: batch_size and files_per_launch must be at least 1')
        if not torch.cuda.is_available():
            raise RuntimeError('DeviceDecodeLoader: needs a GPU (the HIP path has no CPU fallback)')
        self.dataset, self.batch_size, self.files_per_launch = dataset, int(batch_size), int(files_per_launch)
        device = torch.device('cuda' if device is None else device)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device.index is None else device
        self._streams = [torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)]
        self._windows = 0
        self._to_tensor = custom_transforms.ToTensor()
        self.decoded = self.fallbacks = 0     # frames of the last iteration by path

    def __len__(self):
        return -(-len(self.dataset) // self.batch_size)

    # ---------------------------------------------------------------------------------------------- one window
    def _launch(self, first: int):
        """Read, probe and launch frames first .. first + files_per_launch: [(index, group or None, slot)] and the groups."""
        from fosvos_hip import ops
        ds = self.dataset
        last = min(first + self.files_per_launch, len(ds))
        blobs, plans = [], []
        for idx in range(first, last):
            path = os.path.join(ds.db_root_dir, ds.img_list[idx])
            blob = None
            if path.lower().endswith(('.jpg', '.jpeg')):
                try:
                    with open(path, 'rb') as f:
                        blob = f.read()
                except OSError:
                    blob = None               # the host path reports it when the frame's turn comes
            plan = jpeg_read.probe(blob) if blob else None
            blobs.append(blob)
            plans.append(plan if plan is not None and plan.components == 3 else None)
        frames, groups, k = [], [], 0
        stream = self._streams[self._windows % 2]
        self._windows += 1
        while k < len(plans):
            if plans[k] is None:
                frames.append((first + k, None, 0))
                k += 1
                continue
            e = k + 1
            while e < len(plans) and plans[e] is not None and _key(plans[e]) == _key(plans[k]):
                e += 1
            with torch.cuda.stream(stream):
                raw, status = ops.jpeg_decode(blobs[k:e], device=self.device, plans=plans[k:e])
                image = ops.frame_prep(raw)
                status_host = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
                status_host.copy_(status, non_blocking=True)
                done = torch.cuda.Event()
                done.record(stream)
            groups.append({'image': image, 'status': status_host, 'done': done, 'waited': False})
            frames += [(first + k + j, len(groups) - 1, j) for j in range(e - k)]
            k = e
        return frames, groups

    def _host_image(self, idx: int) -> torch.Tensor:
        sample = self._to_tensor(self.dataset[idx])
        return sample['image'].to(self.device)

    def _gt(self, idx: int, h: int, w: int) -> torch.Tensor:
        """``convert_raw``'s mask of frame ``idx`` as ``ToTensor`` leaves it: float32 [1,H,W]."""
        ds = self.dataset
        if ds.labels[idx] is None:
            return torch.zeros((1, h, w), dtype=torch.float32)
        _, gt = ds.convert_raw(np.zeros((1, 1, 3), dtype=np.uint8), read_gray(os.path.join(ds.db_root_dir, ds.labels[idx])))
        return torch.from_numpy(np.ascontiguousarray(gt[None]))

    def _frames(self):
        """(index, image [3,H,W] on the device, ready on the consumer's current stream) in dataset order."""
        n = len(self.dataset)
        ahead = self._launch(0) if n else None
        first = 0
        while ahead is not None:
            frames, groups = ahead
            first += len(frames)
            ahead = self._launch(first) if first < n else None      # the next window decodes while this one is handed out
            for idx, g, slot in frames:
                if g is not None:
                    group = groups[g]
                    if not group['waited']:
                        group['done'].synchronize()
                        group['codes'] = group['status'].tolist()
                        consumer = torch.cuda.current_stream(self.device)
                        consumer.wait_event(group['done'])
                        group['image'].record_stream(consumer)
                        group['waited'] = True
                    if group['codes'][slot] == 0:
                        self.decoded += 1
                        yield idx, group['image'][slot]
                        continue
                self.fallbacks += 1
                yield idx, self._host_image(idx)

    def __iter__(self):
        self.decoded = self.fallbacks = 0
        ds = self.dataset
        held = []
        for idx, image in self._frames():
            held.append((idx, image))
            if len(held) == self.batch_size or idx == len(ds) - 1:
                images = held[0][1][None] if len(held) == 1 else torch.stack([im for _, im in held])
                h, w = int(images.shape[2]), int(images.shape[3])
                gts = [self._gt(i, h, w) for i, _ in held]
                yield {'image': images, 'gt': gts[0][None] if len(gts) == 1 else torch.stack(gts),
                       'seq_name': [ds.seq_list[i] for i, _ in held], 'fname': [ds.fname_list[i] for i, _ in held]}
                held = []
