"""Synthetic stand-in for a DAVIS sequence (no dataset ships offline): frames with the layout, value
range and mean subtraction of ``DAVIS2016.__getitem__`` after ``ToTensor`` (reference:
src/dataloaders/davis_2016.py:101-134) - image [3,H,W] fp32 = noisy BGR frame with a brighter elliptical object, minus
the dataset mean; gt [1,H,W] in {0,1} (the ellipse, ~10 % foreground)."""
import torch
from torch.utils.data import Dataset

MEANVAL = (104.00699, 116.66877, 122.67892)  # src/dataloaders/davis_2016.py:28


def make_gt(h: int, w: int, index: int = 0):
    yy = torch.arange(h, dtype=torch.float32).view(h, 1)
    xx = torch.arange(w, dtype=torch.float32).view(1, w)
    cy, cx = h * (0.45 + 0.02 * (index % 5)), w * (0.5 - 0.02 * (index % 7))
    return ((((yy - cy) / (h * 0.2)) ** 2 + ((xx - cx) / (w * 0.16)) ** 2) <= 1.0).float().unsqueeze(0)


def make_frame(h: int, w: int, seed: int = 1234, index: int = 0):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed + 7919 * index)
    noise = torch.rand((3, h, w), generator=g)
    gt = make_gt(h, w, index)
    # brighter, lower-contrast object on a darker noisy background, then the dataset mean comes off
    img = gt * (150.0 + 100.0 * noise) + (1.0 - gt) * (150.0 * noise) - torch.tensor(MEANVAL).view(3, 1, 1)
    return img, gt


class SyntheticSequence(Dataset):
    """mode='train': one annotated frame (as DAVIS2016(train=True, seq_name=...) yields only frame 0);
    mode='test': ``n_frames`` frames of the same sequence."""

    def __init__(self, seq_name: str = 'synthetic', height: int = 480, width: int = 854, n_frames: int = 1,
                 seed: int = 1234):
        self.seq_name, self.h, self.w, self.n, self.seed = seq_name, height, width, n_frames, seed

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        img, gt = make_frame(self.h, self.w, self.seed, idx)
        return {'image': img, 'gt': gt, 'seq_name': self.seq_name, 'fname': '%05d' % idx}

    def annotation(self, seq_name, fname):
        """The ground truth of frame ``fname`` as the scorer takes it: uint8 [H,W], 1 = object; None for a frame this
        sequence does not hold."""
        idx = int(fname)
        if seq_name != self.seq_name or not 0 <= idx < self.n:
            return None
        return (make_gt(self.h, self.w, idx)[0] >= 0.5).to(torch.uint8).numpy()


def make_ids(h: int, w: int, n_objects: int, index: int = 0):
    """uint8 [H,W] object ids of frame ``index``: K ellipses side by side at distinct centres that drift with the frame index
    (odd and even ids in opposite directions, so neighbours meet); where two overlap the higher id is on top."""
    yy = torch.arange(h, dtype=torch.float32).view(h, 1)
    xx = torch.arange(w, dtype=torch.float32).view(1, w)
    ids = torch.zeros((h, w), dtype=torch.uint8)
    for k in range(1, n_objects + 1):
        side = 1.0 if k % 2 else -1.0
        cy = h * (0.4 + 0.2 * (k % 2) + 0.01 * (index % 5))
        cx = w * (k / (n_objects + 1.0) + side * 0.012 * (index % 7))
        inside = (((yy - cy) / (h * 0.24)) ** 2 + ((xx - cx) / (w * 0.62 / (n_objects + 1.0))) ** 2) <= 1.0
        ids[inside] = k
    return ids


def object_colour(k: int):
    """The BGR offset of object k: distinct for k = 1..16."""
    return (55.0 + (k * 67) % 200, 55.0 + (k * 101) % 200, 55.0 + (k * 151) % 200)


class SyntheticObjectsSequence(Dataset):
    """A synthetic sequence of ``n_objects`` objects (DAVIS 2017 style): noisy BGR frames with one ellipse of its own colour
    per object, minus the dataset mean.  ``object_id=k``: ``gt`` is object k against everything else (what net k is
    fine-tuned on); None: every object against the background.  ``annotation(seq, fname)`` is the id map the scorer takes."""

    def __init__(self, seq_name: str = 'synthetic', height: int = 480, width: int = 854, n_frames: int = 1,
                 n_objects: int = 2, object_id=None, seed: int = 1234):
        if not 1 <= n_objects <= 16:
            raise ValueError('SyntheticObjectsSequence: n_objects {} outside [1, 16]'.format(n_objects))
        if object_id is not None and not 1 <= object_id <= n_objects:
            raise ValueError('SyntheticObjectsSequence: object_id {} outside [1, {}]'.format(object_id, n_objects))
        self.seq_name, self.h, self.w, self.n, self.seed = seq_name, height, width, n_frames, seed
        self.n_objects, self.object_id = n_objects, object_id

    def __len__(self):
        return self.n

    def __getitem__(self, idx):
        g = torch.Generator(device='cpu')
        g.manual_seed(self.seed + 7919 * idx)
        noise = torch.rand((3, self.h, self.w), generator=g)
        ids = make_ids(self.h, self.w, self.n_objects, idx)
        img = 110.0 * noise
        for k in range(1, self.n_objects + 1):
            colour = torch.tensor(object_colour(k)).view(3, 1, 1)
            img = torch.where((ids == k).unsqueeze(0), colour + 40.0 * noise, img)
        img = img - torch.tensor(MEANVAL).view(3, 1, 1)
        gt = (ids != 0) if self.object_id is None else (ids == self.object_id)
        return {'image': img, 'gt': gt.float().unsqueeze(0), 'seq_name': self.seq_name, 'fname': '%05d' % idx}

    def annotation(self, seq_name, fname):
        """uint8 [H,W] object ids of frame ``fname``; None for a frame this sequence does not hold."""
        idx = int(fname)
        if seq_name != self.seq_name or not 0 <= idx < self.n:
            return None
        return make_ids(self.h, self.w, self.n_objects, idx).numpy()
