"""Host plumbing around the loops (reference: src/util/io_helper.py): DataLoader factories, an
optional tensorboard writer and the YAML settings dump.  ``synthetic=(H, W)`` selects the synthetic sequence
instead of a DAVIS tree on disk."""
import dataclasses
from pathlib import Path
from typing import Optional, Tuple

import yaml
from torch.utils.data import DataLoader

from dataloaders import custom_transforms
from dataloaders.davis_2016 import DAVIS2016, DavisAnnotations
from dataloaders.synthetic import SyntheticSequence
from util.logger import get_logger

log = get_logger(__file__)


class NullSummaryWriter:
    """Stands in for tensorboardX.SummaryWriter when it is not installed."""

    def add_scalar(self, *a, **k):
        pass

    def close(self):
        pass


def get_summary_writer(path, comment: str = ''):
    try:
        from tensorboardX import SummaryWriter
    except ImportError:
        return NullSummaryWriter()
    return SummaryWriter(log_dir=str(path), comment=comment)


def write_settings(save_dir: Path, name: str, settings, variant_offline: Optional[int] = None,
                   variant_online: Optional[int] = None) -> None:
    save_dir = Path(save_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    stem = name + ('' if variant_offline is None else '_' + str(variant_offline)) + \
        ('' if variant_online is None else '_' + str(variant_online))
    with open(str(save_dir / (stem + '_settings.yml')), 'w') as f:
        yaml.safe_dump(dataclasses.asdict(settings), f, default_flow_style=False)


def results_dir(root: Path, name: str, stage: str, variant_offline, variant_online=None) -> Path:
    """Where a test pass writes: ``<root>/<name>/<stage>`` (stage 'online' or 'offline') for the plain net, for a variant
    ``<root>/<name>/<variant_offline>/`` and then 'offline' (its parent network) or the online variant."""
    if variant_offline is None:
        return root / name / stage
    return root / name / str(variant_offline) / ('offline' if stage == 'offline' else str(variant_online))


def get_data_loader_train(db_root_dir, batch_size: int, seq_name: Optional[str] = None,
                          synthetic: Optional[Tuple[int, int]] = None,
                          shard: Optional[Tuple[int, int]] = None, resident: bool = True,
                          resident_set: bool = False, rotate=None, lucid=None) -> DataLoader:
    """shard = (rank, world): this process draws its own 1/world of every epoch (data-parallel OFFLINE training, where
    the ranks split each iteration's batch); None: the reference's single-process loader.
    resident: a sequence run (``seq_name``: ONE training sample, src/dataloaders/davis_2016.py:72-83) gets the loader that
    keeps the sample's six flip / scale variants on the device and draws them with the reference pipeline's random numbers
    (dataloaders/resident.py: same tensors, same order as the DataLoader below under the same torch seed); False: that
    DataLoader itself (one worker start + decode + resample per iteration).
    resident_set (opt-in): the whole training set (no ``seq_name``, no ``synthetic``) gets the loader that decodes every
    sample once, keeps the uint8 frames and masks on the device and flips / rescales each draw there in one HIP launch
    (dataloaders/resident.py: ResidentTrainSetLoader, same tensors in the same order as the DataLoader below under the
    same torch seed, ``shard`` included).  It yields batches of one sample only and raises for any other batch_size.
    rotate (opt-in): a fosvos_hip.options.RotateOptions.  ``ScaleNRotate(rots, scales, renormalize)`` stands in place of
    ``Resize``, as in the reference's commented line; the DataLoader below then warps in numpy on the host (about 0.16 s for
    a 480x854 sample) and is the yardstick the resident loaders replay with one HIP launch per draw.  The synthetic loader
    augments nothing and refuses it.
    lucid (opt-in): a fosvos_hip.options.LucidOptions - the object moves against its background (dataloaders/lucid.py).  Only
    the resident one-shot loader composes it (one HIP launch per draw); every other loader, ``rotate`` beside it and the
    synthetic loader are refused."""
    if lucid is not None:
        if synthetic is not None:
            raise ValueError('get_data_loader_train: lucid augments DAVIS samples; the synthetic loader augments nothing')
        if rotate is not None:
            raise ValueError('get_data_loader_train: rotate and lucid both stand in place of the rescale: pass one of them')
        if seq_name is None:
            raise ValueError('get_data_loader_train: lucid is built for the one-shot sample of a sequence run; the offline '
                             'training set would need a filled background per training frame')
        if not (resident and shard is None and batch_size == 1):
            raise ValueError('get_data_loader_train: lucid composes from the bytes the resident one-shot loader keeps on the '
                             'device (resident=True, no shard, batch_size 1); the host DataLoader has none to fill from')
        from dataloaders.resident import ResidentOneShotLoader
        return ResidentOneShotLoader(DAVIS2016(mode='train', db_root_dir=str(db_root_dir), transform=None, seq_name=seq_name),
                                     lucid=lucid)
    if synthetic is not None:
        if rotate is not None:
            raise ValueError('get_data_loader_train: rotate augments DAVIS samples; the synthetic loader augments nothing')
        ds = SyntheticSequence(seq_name or 'synthetic', synthetic[0], synthetic[1], n_frames=1,
                               seed=1234 + (shard[0] if shard else 0))
        return DataLoader(ds, batch_size=batch_size, shuffle=True, num_workers=0)
    # src/util/io_helper.py:62-70: random flip, random rescale (ScaleNRotate stays disabled as in the reference unless
    # ``rotate`` asks for it: it then stands where Resize stood, as in the reference's commented line), ToTensor
    composed = custom_transforms.Compose([custom_transforms.RandomHorizontalFlip(),
                                          custom_transforms.Resize() if rotate is None else rotate.transform(),
                                          custom_transforms.ToTensor()])
    if resident and seq_name is not None and shard is None and batch_size == 1:
        from dataloaders.resident import ResidentOneShotLoader
        return ResidentOneShotLoader(DAVIS2016(mode='train', db_root_dir=str(db_root_dir), transform=None, seq_name=seq_name),
                                     rotate=rotate)
    if resident_set and seq_name is None:
        from dataloaders.resident import ResidentTrainSetLoader
        return ResidentTrainSetLoader(DAVIS2016(mode='train', db_root_dir=str(db_root_dir), transform=None),
                                      shard=shard, batch_size=batch_size, rotate=rotate)
    db_train = DAVIS2016(mode='train', db_root_dir=str(db_root_dir), transform=composed, seq_name=seq_name)
    if shard is not None:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(db_train, num_replicas=shard[1], rank=shard[0], shuffle=True)
        return DataLoader(db_train, batch_size=batch_size, sampler=sampler, num_workers=1)
    return DataLoader(db_train, batch_size=batch_size, shuffle=True, num_workers=1)


def get_data_loader_test(db_root_dir, batch_size: int, seq_name: Optional[str] = None,
                         synthetic: Optional[Tuple[int, int]] = None, n_frames: int = 4, device_decode: bool = False):
    """``device_decode`` (opt-in): the frames' JPEG files are decoded on the device - a
    dataloaders.device_decode.DeviceDecodeLoader, which yields the same minibatches with ``image`` on the GPU."""
    if device_decode:
        if synthetic is not None:
            raise ValueError('get_data_loader_test: device_decode decodes JPEG files; the synthetic sequence has none')
        from dataloaders.device_decode import DeviceDecodeLoader
        return DeviceDecodeLoader(DAVIS2016(mode='test', db_root_dir=str(db_root_dir), transform=None, seq_name=seq_name),
                                  batch_size=batch_size)
    if synthetic is not None:
        ds = SyntheticSequence(seq_name or 'synthetic', synthetic[0], synthetic[1], n_frames=n_frames)
        return DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=0)
    db_test = DAVIS2016(mode='test', db_root_dir=str(db_root_dir), transform=custom_transforms.ToTensor(),
                        seq_name=seq_name)
    return DataLoader(db_test, batch_size=batch_size, shuffle=False, num_workers=2)


def get_annotations(db_root_dir, data_loader: DataLoader, synthetic: Optional[Tuple[int, int]] = None):
    """The ground truth source of the scored test pass for a loader of ``get_data_loader_test``:
    ``annotations(seq_name, fname)`` -> uint8 [H,W] or None."""
    if synthetic is not None:
        return data_loader.dataset.annotation
    return DavisAnnotations(db_root_dir)
