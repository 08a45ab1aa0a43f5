"""The device-resident offline training set (dataloaders/resident.py: ResidentTrainSetLoader) on the CPU: it replays the
per-iteration DataLoader of src/util/io_helper.py:62-70 (shuffled order, flip, one of three scales) draw for draw, and the
table recipe of the HIP kernel (fosvos_augment_sample: host-built taps and weights, value lookup tables, fp32 products
summed in numpy's order) reproduces custom_transforms.resize + flip + mean + gt normalisation bit for bit."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fosvos_amd"))

from dataloaders import custom_transforms as T  # noqa: E402
from dataloaders.davis_2016 import DAVIS2016, MEANVAL  # noqa: E402

# three training sequences, one of another size (the loader must not assume one frame size), one validation sequence
SEQS = {"bear": (3, 24, 40), "camel": (2, 24, 40), "cows": (2, 19, 33), "dog": (2, 24, 40)}
TRAIN = ["bear", "camel", "cows"]
N_EPOCHS = 8


def _frame(seq, k, h, w):
    rng = np.random.RandomState(zlib.crc32(("%s/%d" % (seq, k)).encode()))
    return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _mask(k, h, w, peak):
    m = np.zeros((h, w), dtype=np.uint8)
    m[3 + k:12 + k, 8:21] = peak
    return m


def write_davis_tree(root, seqs=SEQS, train=TRAIN):
    lines = {"train": [], "val": []}
    for si, (seq, (n, h, w)) in enumerate(seqs.items()):
        (root / "JPEGImages" / "480p" / seq).mkdir(parents=True)
        (root / "Annotations" / "480p" / seq).mkdir(parents=True)
        for k in range(n):
            Image.fromarray(_frame(seq, k, h, w)).save(str(root / "JPEGImages" / "480p" / seq / ("%05d.jpg" % k)),
                                                       quality=95)
            # masks of 0/255 and one of 0/7 (the gt scale is per frame)
            Image.fromarray(_mask(k, h, w, 7 if (si, k) == (1, 1) else 255)).save(
                str(root / "Annotations" / "480p" / seq / ("%05d.png" % k)))
            lines["train" if seq in train else "val"].append(
                "/JPEGImages/480p/%s/%05d.jpg /Annotations/480p/%s/%05d.png \n" % (seq, k, seq, k))
    (root / "ImageSets" / "480p").mkdir(parents=True)
    for split in ("train", "val"):
        (root / "ImageSets" / "480p" / (split + ".txt")).write_text("".join(lines[split]))
    (root / "ImageSets" / "480p" / "trainval.txt").write_text("".join(lines["train"] + lines["val"]))
    return root


@pytest.fixture(scope="module")
def davis_root(tmp_path_factory):
    return write_davis_tree(tmp_path_factory.mktemp("davis_set"))


def _epochs(loader, n_epochs, set_epoch=False):
    seen = []
    for epoch in range(n_epochs):
        if set_epoch:
            loader.sampler.set_epoch(epoch)
        seen.append(list(loader))
    return seen, torch.rand(4)  # (the default generator's state afterwards shows in the next draw)


def assert_same_epochs(a, b):
    """Two loaders' epochs: the same sample order, shapes and tensors (b may live on the device)."""
    (ea, ra), (eb, rb) = a, b
    assert torch.equal(ra, rb)
    assert len(ea) == len(eb)
    shapes = set()
    for xa, xb in zip(ea, eb):
        assert [(m["seq_name"], m["fname"]) for m in xa] == [(m["seq_name"], m["fname"]) for m in xb]
        for ma, mb in zip(xa, xb):
            for key in ("image", "gt"):
                assert ma[key].dtype == mb[key].dtype and tuple(ma[key].shape) == tuple(mb[key].shape), key
                assert torch.equal(ma[key], mb[key].cpu()), (key, ma["seq_name"], ma["fname"])
            shapes.add(tuple(ma["image"].shape))
    assert len(shapes) >= 4  # several scales and both frame sizes came up


def test_cpu_loader_replays_the_dataloader(davis_root):
    from util import io_helper
    from dataloaders.resident import ResidentTrainSetLoader
    runs = []
    for resident_set in (False, True):
        torch.manual_seed(123)
        if resident_set:
            loader = ResidentTrainSetLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root)), device="cpu")
        else:
            loader = io_helper.get_data_loader_train(str(davis_root), 1, resident=False)
        assert len(loader) == 7
        runs.append(_epochs(loader, N_EPOCHS))
    assert_same_epochs(*runs)
    orders = {tuple(tuple(m["fname"] + m["seq_name"]) for m in ep) for ep in runs[0][0]}
    assert len(orders) > 1  # a new order each epoch


@pytest.mark.parametrize("rank", [0, 1])
def test_cpu_loader_replays_the_sharded_dataloader(davis_root, rank):
    from util import io_helper
    from dataloaders.resident import ResidentTrainSetLoader
    runs = []
    for resident_set in (False, True):
        torch.manual_seed(9)
        if resident_set:
            loader = ResidentTrainSetLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root)), device="cpu",
                                            shard=(rank, 2))
        else:
            loader = io_helper.get_data_loader_train(str(davis_root), 1, shard=(rank, 2))
        assert len(loader) == 4  # ceil(7 / 2): the last shard is padded
        runs.append(_epochs(loader, N_EPOCHS, set_epoch=True))
    assert_same_epochs(*runs)


def emulate_kernel(ds, img_u8, lab_u8, flip, sc):
    """The recipe of fosvos_augment_sample on the host: resize_plan's tables, the value lookup tables, and per output value
    ((((0 + a0*w0) + a1*w1) + a2*w2) + a3*w3) in fp32, horizontal taps first, vertical taps over their fp32 results."""
    h, w = lab_u8.shape
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)
    img_lut = ds.convert_raw(ramp, None)[0].reshape(256, 3)
    gt_lut = np.arange(256, dtype=np.float32) / np.float32(max(float(lab_u8.max()), 1e-8))
    plan = T.resize_plan(h, w, sc, sc)
    mirror = (lambda c: w - 1 - c) if flip else (lambda c: c)
    chans = np.arange(3)[None, None, :]
    if plan["copy"]:
        cols = mirror(np.arange(w))
        return img_lut[img_u8[:, cols], chans], gt_lut[lab_u8[:, cols]]
    col_taps, col_w = plan["col_taps"].astype(np.int32), plan["col_w"]
    row_taps, row_w = plan["row_taps"].astype(np.int32), plan["row_w"]
    assert col_w.dtype == np.float32 and row_w.dtype == np.float32
    acc = np.zeros((plan["oh"], plan["ow"], 3), dtype=np.float32)
    for k in range(4):
        hk = np.zeros_like(acc)
        for j in range(4):
            a = img_lut[img_u8[row_taps[:, k][:, None], mirror(col_taps[:, j])[None, :]], chans]
            hk = hk + a * col_w[:, j][None, :, None]
        acc = acc + hk * row_w[:, k][:, None, None]
    gt = gt_lut[lab_u8[plan["row_near"][:, None], mirror(plan["col_near"])[None, :]]]
    return acc, gt


@pytest.mark.parametrize("size", [(61, 107), (24, 40), (480, 854)])
def test_kernel_recipe_is_the_numpy_pipeline_bit_for_bit(size):
    h, w = size
    ds = DAVIS2016.__new__(DAVIS2016)
    ds.meanval = MEANVAL
    rng = np.random.RandomState(h * 1000 + w)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    lab = np.where(rng.rand(h, w) > 0.6, 200, 0).astype(np.uint8)
    lab[0, 0] = 201
    for sc in (0.5, 0.8, 1):
        for flip in (False, True):
            image, gt = ds.convert_raw(img, lab)
            if flip:
                image, gt = np.ascontiguousarray(image[:, ::-1]), np.ascontiguousarray(gt[:, ::-1])
            want_img, want_gt = T.resize(image, sc, sc), T.resize(gt, sc, sc)
            got_img, got_gt = emulate_kernel(ds, img, lab, flip, sc)
            assert got_img.shape == want_img.shape and got_gt.shape == want_gt.shape, (sc, flip)
            assert np.array_equal(got_img.view(np.uint32), want_img.view(np.uint32)), (size, sc, flip)
            assert np.array_equal(got_gt.view(np.uint32), want_gt.view(np.uint32)), (size, sc, flip)


def test_resize_plan_matches_resize_sizes():
    for h, w in ((61, 107), (480, 854), (1, 1), (3, 5)):
        for sc in (0.5, 0.8, 1):
            try:
                out = T.resize(np.zeros((h, w), np.float32), sc, sc)
            except ValueError:
                with pytest.raises(ValueError):
                    T.resize_plan(h, w, sc, sc)
                continue
            plan = T.resize_plan(h, w, sc, sc)
            assert (plan["oh"], plan["ow"]) == out.shape
            assert plan["copy"] == (out.shape == (h, w))
            if not plan["copy"]:
                for k in ("col_taps", "col_near"):
                    assert plan[k].min() >= 0 and plan[k].max() <= w - 1
                for k in ("row_taps", "row_near"):
                    assert plan[k].min() >= 0 and plan[k].max() <= h - 1


def test_factory_defaults_and_batch_size(davis_root):
    from torch.utils.data import DataLoader
    from util import io_helper
    from dataloaders.resident import ResidentOneShotLoader, ResidentTrainSetLoader
    assert type(io_helper.get_data_loader_train(str(davis_root), 1)) is DataLoader
    assert type(io_helper.get_data_loader_train(str(davis_root), 1, shard=(0, 2))) is DataLoader
    assert isinstance(io_helper.get_data_loader_train(str(davis_root), 1, "bear"), ResidentOneShotLoader)
    # a sequence run keeps its own loaders whatever resident_set says
    assert isinstance(io_helper.get_data_loader_train(str(davis_root), 1, "bear", resident_set=True), ResidentOneShotLoader)
    assert type(io_helper.get_data_loader_train(str(davis_root), 1, "bear", resident=False, resident_set=True)) is DataLoader
    loader = io_helper.get_data_loader_train(str(davis_root), 1, resident_set=True)
    assert isinstance(loader, ResidentTrainSetLoader) and len(loader) == 7
    assert loader.decode_seconds >= 0 and loader.sizes.count((19, 33)) == 2
    with pytest.raises(ValueError):
        io_helper.get_data_loader_train(str(davis_root), 2, resident_set=True)
    with pytest.raises(ValueError):
        ResidentTrainSetLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root)), device="cpu", batch_size=2)
    with pytest.raises(ValueError):  # the loader applies the transforms itself
        ResidentTrainSetLoader(DAVIS2016(mode="train", db_root_dir=str(davis_root), transform=T.ToTensor()), device="cpu")


def test_resident_train_set_flag_is_offline_only():
    from util import args_helper
    assert args_helper.parse_args(is_online=False, argv=["--resident-train-set"]).resident_train_set is True
    assert args_helper.parse_args(is_online=False, argv=[]).resident_train_set is False
    assert not hasattr(args_helper.parse_args(is_online=True, argv=[]), "resident_train_set")
    with pytest.raises(SystemExit):
        args_helper.parse_args(is_online=True, argv=["--resident-train-set"])


def test_offline_main_passes_the_flag(monkeypatch, tmp_path):
    import train_offline
    seen = {}

    def fake_train_and_test(prov, settings):
        seen["flag"] = train_offline.resident_train_set

    monkeypatch.setattr(train_offline, "train_and_test", fake_train_and_test)
    monkeypatch.setattr(train_offline.gpu_handler, "select_gpu", lambda *a, **k: None)
    monkeypatch.setattr(train_offline, "resident_train_set", False)
    monkeypatch.setattr(train_offline, "save_dir_models", tmp_path / "models")
    monkeypatch.setattr(train_offline, "save_dir_results", tmp_path / "results")
    train_offline.main(["--resident-train-set", "--no-testing"])
    assert seen["flag"] is True
    train_offline.main(["--no-testing"])
    assert seen["flag"] is False
