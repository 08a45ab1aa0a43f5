"""DAVIS 2017: several annotated objects a sequence.  One object of one sequence at a time, as the one-shot loop takes it:
a ``DAVIS2016`` whose ``gt`` is "this object against everything else".

On-disk layout (``db_root_dir``):
    ImageSets/2017/{train,val}.txt            one sequence name a line
    JPEGImages/480p/<seq>/<f>.jpg             frames (the sorted directory listing is the sequence)
    Annotations/480p/<seq>/<f>.png            palette PNGs: a pixel's INDEX is its object id, 0 = background

An annotation is read WITHOUT ``convert``: PIL hands out the indices of a mode-``P`` file, and those are the ids (``convert('L')``,
which the 2016 reader applies, would turn them into the luminance of their palette colours).  A mode-``L`` file is taken as
ids too.  The sample dict is the parent's; ``ResidentOneShotLoader`` and ``DeviceDecodeLoader`` take the dataset through
``read_raw`` / ``convert_raw``.
"""
import os
from pathlib import Path as P

import numpy as np
from PIL import Image

from dataloaders.davis_2016 import DAVIS2016, MEANVAL, _imresize, read_bgr
from util.logger import get_logger

log = get_logger(__file__)


def read_ids(path: str) -> np.ndarray:
    """uint8 H x W object ids of an annotation file: the indices of a palette file, the values of a greyscale one."""
    with Image.open(path) as im:
        if im.mode not in ('P', 'L'):
            raise ValueError('{}: an annotation must be a palette (P) or greyscale (L) PNG, got mode {}'.format(path, im.mode))
        return np.array(im, dtype=np.uint8)


def sequence_names(db_root_dir, split: str):
    with open(str(P(str(db_root_dir)) / 'ImageSets' / '2017' / (split + '.txt'))) as f:
        return [line.strip() for line in f if line.strip()]


def _annotation_files(db_root_dir, seq_name: str):
    folder = os.path.join(str(db_root_dir), 'Annotations', '480p', seq_name)
    return sorted(f for f in os.listdir(folder) if f.endswith('.png'))


def n_objects(db_root_dir, seq_name: str) -> int:
    """The largest id in the first frame's annotation."""
    files = _annotation_files(db_root_dir, seq_name)
    if not files:
        raise RuntimeError('sequence {} has no annotation'.format(seq_name))
    return int(read_ids(os.path.join(str(db_root_dir), 'Annotations', '480p', seq_name, files[0])).max())


class Davis2017Annotations:
    """``annotations(seq_name, fname)`` for ``experiment_helper.test_objects``: uint8 [H,W] object ids, or None where the
    tree has no such file."""

    def __init__(self, db_root_dir):
        self.db_root_dir = str(db_root_dir)

    def __call__(self, seq_name, fname):
        path = os.path.join(self.db_root_dir, 'Annotations', '480p', seq_name, fname + '.png')
        if not os.path.exists(path):
            return None
        return read_ids(path)


class DAVIS2017(DAVIS2016):
    """Object ``object_id`` of sequence ``seq_name``.  mode 'train': the first frame only; 'test': every frame.  ``gt`` is
    (id == object_id) as 0 / 1, all zeros behind the first frame (the annotations are hidden, as in the parent class)."""

    def __init__(self, mode='train', db_root_dir='/path/to/DAVIS-2017', seq_name=None, object_id=1, transform=None,
                 meanval=MEANVAL, inputRes=None):
        self.mode = mode.lower()
        if self.mode not in ('train', 'test'):
            raise Exception("Mode {} does not exist. Must be one of ['train', 'test']".format(mode))
        if seq_name is None:
            raise ValueError('DAVIS2017: a sequence name is needed (one object of one sequence at a time)')
        self.inputRes = inputRes
        self.db_root_dir = str(db_root_dir)
        self.transform = transform
        self.meanval = meanval
        self.seq_name = seq_name
        self.object_id = int(object_id)
        known = [s for split in ('train', 'val') if (P(self.db_root_dir) / 'ImageSets' / '2017' / (split + '.txt')).exists()
                 for s in sequence_names(self.db_root_dir, split)]
        if seq_name not in known:
            raise RuntimeError('sequence {} is not listed in ImageSets/2017'.format(seq_name))
        frames = sorted(f for f in os.listdir(os.path.join(self.db_root_dir, 'JPEGImages', '480p', seq_name))
                        if f.endswith('.jpg'))
        if not frames:
            raise RuntimeError('sequence {} has no frames'.format(seq_name))
        count = n_objects(self.db_root_dir, seq_name)
        if not 1 <= self.object_id <= count:
            raise ValueError('DAVIS2017: sequence {} has objects 1..{}, got object_id {}'.format(seq_name, count, object_id))
        if self.mode == 'train':
            frames = frames[:1]
        stems = [f[:-len('.jpg')] for f in frames]
        self.seq_list = [seq_name] * len(frames)
        self.fname_list = stems
        self.img_list = [os.path.join('JPEGImages', '480p', seq_name, f) for f in frames]
        self.labels = [os.path.join('Annotations', '480p', seq_name, s + '.png') if k == 0 else None
                       for k, s in enumerate(stems)]
        log.info('Done initializing {} object {} Dataset'.format(seq_name, self.object_id))

    def read_raw(self, idx):
        """uint8 H x W x 3 BGR frame and the object's uint8 H x W mask (0 / 1), or None where the annotation is hidden."""
        img = read_bgr(os.path.join(self.db_root_dir, self.img_list[idx]))
        label = None
        if self.labels[idx] is not None:
            label = (read_ids(os.path.join(self.db_root_dir, self.labels[idx])) == self.object_id).astype(np.uint8)
        if self.inputRes is not None:
            img = _imresize(img, self.inputRes)
            if label is not None:
                label = _imresize(label, self.inputRes, nearest=True)
        return img, label
